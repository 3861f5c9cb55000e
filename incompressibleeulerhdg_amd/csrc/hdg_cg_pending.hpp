// Which p / x updates of the condensed CG are queued (Engine::XpRide, Engine::trace_cg_sr; kernels: k_cg_sr_update_xp, side_xp).
// The p / x half of iteration j's update -- p = (z_j - c_j n) + beta_j p ; x += alpha_j p -- is read by nothing before the next
// such update, so up to M consecutive ones are applied in ONE pass over p and x, entry by entry and in order: the same bits as
// M passes.  What a queued update needs is kept in a ring of M slots: iteration j has its z in trace vector j mod M and its
// (alpha, beta, c) at the same slot of a small device array.  This header is the bookkeeping, functions of integers only
// (plain C++, no HIP): tests/host/cg_pending_check.cpp walks every (ring size, iteration count, forced flush).
//   before the preconditioner of iteration j writes z_j:  full()  -> slot j mod M is still queued: apply all() first
//   once iteration j has formed its scalars:              push()
//   a true residual, the explicit projection of z, |x|:   apply all(), then applied()
//   normal exit:                                          apply all_but_newest(), then drop() -- the newest queued update is the
//                                                         step beyond the tested iterate
//   exception:                                            drop()
#pragma once

namespace hdg {

constexpr int CG_XP_MAX_BATCH = 16;  // largest ring (HDG_CG_XP_BATCH is clamped to it)

struct CgBatch {
  long first;  // iterations first .. first + count - 1, oldest first
  int count;
};

struct CgPending {
  int M = 1;       // ring size = largest batch
  long next = 0;   // the iteration whose z is written next
  long first = 0;  // the oldest queued iteration (== next: nothing queued)

  void reset(int m) { M = m < 1 ? 1 : (m > CG_XP_MAX_BATCH ? CG_XP_MAX_BATCH : m); next = first = 0; }
  int count() const { return (int)(next - first); }
  int slot(long j) const { return (int)(j % M); }
  int write_slot() const { return slot(next); }  // where z and the scalars of iteration `next` go
  bool full() const { return count() == M; }     // write_slot() holds a queued update
  void push() { next++; }
  CgBatch all() const { return CgBatch{first, count()}; }
  CgBatch all_but_newest() const { return CgBatch{first, count() > 0 ? count() - 1 : 0}; }
  void applied() { first = next; }  // all() has been applied
  void drop() { first = next; }     // whatever is queued is given up
};

}  // namespace hdg
