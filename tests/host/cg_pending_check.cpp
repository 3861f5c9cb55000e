// CPU check of csrc/hdg_cg_pending.hpp (compiled by tests/test_cg_pending_host.py with g++ -fsanitize=address,undefined): the
// queue of deferred p / x updates of the condensed CG, driven the way Engine::trace_cg_sr drives it.  For every ring size
// M <= 8, every iteration count <= 40 and every position of a forced flush (none, or after any iteration):
//   every iteration's update is applied exactly once and in order, from the slot that still holds ITS z and scalars;
//   no slot is overwritten while its update is queued;
//   the newest update is dropped only at a normal exit (and only if a flush has not applied it already);
//   an exception applies nothing more.
#include <cstdio>
#include <vector>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_cg_pending.hpp"

namespace {

struct Sim {
  hdg::CgPending q;
  std::vector<long> owner;    // which iteration's z a slot holds (-1: none)
  std::vector<long> applied;  // the updates in the order they were applied
  bool ok = true;
  explicit Sim(int M) : owner((size_t)M, -1) { q.reset(M); }
  void apply(const hdg::CgBatch& b) {
    if (b.count < 0 || b.count > q.M) ok = false;
    for (int j = 0; j < b.count; j++) {
      const long it = b.first + j;
      if (owner[(size_t)q.slot(it)] != it) ok = false;  // its z has been overwritten
      applied.push_back(it);
    }
  }
  void iteration(long it) {
    if (q.full()) { apply(q.all()); q.applied(); }  // the cycle of the preconditioner carries the batch
    if (q.next != it) ok = false;
    const int s = q.write_slot();
    if (s < 0 || s >= q.M) { ok = false; return; }
    for (long p = q.first; p < q.next; p++)
      if (q.slot(p) == s) ok = false;  // the post kernel would overwrite a queued z
    owner[(size_t)s] = it;
    q.push();
    if (q.count() < 1 || q.count() > q.M) ok = false;
  }
  void flush() { apply(q.all()); q.applied(); }
};

bool in_order(const std::vector<long>& a, long n) {
  if ((long)a.size() != n) return false;
  for (long i = 0; i < n; i++) if (a[(size_t)i] != i) return false;
  return true;
}

}  // namespace

int main() {
  long cases = 0;
  for (int M = 1; M <= 8; M++) {
    for (int nit = 1; nit <= 40; nit++) {
      for (int flush = -1; flush < nit; flush++) {  // a true residual / projection / |x| after iteration `flush`
        for (int exit_kind = 0; exit_kind < 2; exit_kind++) {  // 0: normal exit, 1: exception
          Sim s(M);
          for (long it = 0; it < nit; it++) {
            s.iteration(it);
            if (it == flush) s.flush();
          }
          long expect = nit;
          if (exit_kind == 0) {
            s.apply(s.q.all_but_newest());
            s.q.drop();
            if (flush != nit - 1) expect = nit - 1;  // the newest is dropped, unless the flush has applied it
          } else {
            s.q.drop();
            expect = (long)s.applied.size();  // nothing more; what was applied is a prefix
            if (expect > nit) s.ok = false;
          }
          if (s.q.count() != 0) s.ok = false;
          if (!s.ok || !in_order(s.applied, expect)) {
            std::printf("error M=%d iterations=%d flush=%d exit=%d applied=%zu\n", M, nit, flush, exit_kind, s.applied.size());
            return 1;
          }
          cases++;
        }
      }
    }
  }
  // the ring size is clamped
  hdg::CgPending q;
  q.reset(0);
  if (q.M != 1) { std::printf("error clamp low\n"); return 1; }
  q.reset(1000);
  if (q.M != hdg::CG_XP_MAX_BATCH) { std::printf("error clamp high\n"); return 1; }
  std::printf("ok %ld\n", cases);
  return 0;
}
