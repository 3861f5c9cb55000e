// Bookkeeping of a per-step output: rows of `width` doubles appended to a device buffer, one per completed step, with no
// host synchronisation; rows beyond the capacity are counted and reported when the rows are fetched.  Plain C++: the
// device pointer and its allocation stay in the Engine (log_size / log_fetch / log_get, hdg_engine.hip).
// Lifetime of the buffer, the same for every log: one that is large enough is reused, one that must grow is freed and
// reallocated; switching a recorder off (capacity 0) keeps the buffer for the next use, the engine frees it at its end.
#pragma once

namespace hdg {

struct RowLog {
  static constexpr long DROPPED = -1;
  long width = 0;    // doubles per row
  long cap = 0;      // rows the log may hold; 0: switched off
  long n = 0;        // rows written
  long dropped = 0;  // rows that found the log full
  long alloc = 0;    // doubles in the device buffer
  void reset(long width_, long cap_) { width = width_; cap = cap_; n = 0; dropped = 0; }
  void clear_counts() { n = 0; dropped = 0; }
  // offset (in doubles) of the next row, or DROPPED: counted when the log is full, not when it is switched off
  long next() {
    if (cap <= 0) return DROPPED;
    if (n >= cap) { dropped++; return DROPPED; }
    return (n++) * width;
  }
};

}  // namespace hdg
