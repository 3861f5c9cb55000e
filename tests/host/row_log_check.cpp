// csrc/hdg_row_log.hpp on the host: offsets, the drop count, clear_counts and a log that is switched off.
#include <cstdio>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_row_log.hpp"

#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("failed line %d: %s\n", __LINE__, #cond);      \
      return 1;                                                  \
    }                                                            \
  } while (0)

int main() {
  hdg::RowLog L;
  CHECK(L.next() == hdg::RowLog::DROPPED && L.n == 0 && L.dropped == 0);  // never sized: switched off
  L.alloc = 6;
  L.reset(3, 2);
  CHECK(L.width == 3 && L.cap == 2 && L.n == 0 && L.dropped == 0 && L.alloc == 6);
  CHECK(L.next() == 0);
  CHECK(L.next() == 3);
  CHECK(L.next() == hdg::RowLog::DROPPED);
  CHECK(L.n == 2 && L.dropped == 1);
  L.clear_counts();
  CHECK(L.cap == 2 && L.width == 3 && L.alloc == 6 && L.n == 0 && L.dropped == 0);
  CHECK(L.next() == 0 && L.n == 1);
  L.reset(3, 0);  // switched off: next() is a no-op that counts nothing
  for (int i = 0; i < 3; i++) CHECK(L.next() == hdg::RowLog::DROPPED);
  CHECK(L.n == 0 && L.dropped == 0 && L.alloc == 6);
  std::printf("ok\n");
  return 0;
}
