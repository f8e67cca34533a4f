// The parts of the host table one ragged call builds in a slot of the handle's pinned ring and uploads behind the call.  No
// handle and no HIP here (api_common.hpp's ring_take and ring_upload move the bytes).  A call lists its parts once, each as
// add<T>(count); the total, the host pointers it fills and the device pointers it hands to the launcher all come from that list,
// so the three cannot disagree.
#pragma once
#include <stddef.h>

// One part: elements of T from byte `off` of the table, on the host and on the device alike.
template <typename T>
struct HostPart {
  size_t off = 0;
  T* host(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
  const T* dev(const void* base) const { return reinterpret_cast<const T*>(static_cast<const char*>(base) + off); }
};

struct HostTable {
  static constexpr int kMax = 8;       // the largest table has 7 parts; ring_take refuses a list that overflowed
  size_t off[kMax], len[kMax];         // every part's first byte and byte count, in list order
  int n = 0;
  size_t end = 0;

  // parts go in list order, each from the next 16-byte boundary; a part of count 0 takes no bytes, and nothing pads the last part
  template <typename T>
  HostPart<T> add(size_t count) {
    static_assert(alignof(T) <= 16, "a part starts on a 16-byte boundary");
    if (n >= kMax) { ++n; return {}; }
    off[n] = (end + 15) / 16 * 16;
    len[n] = count * sizeof(T);
    end = off[n] + len[n];
    return {off[n++]};
  }
  bool overflowed() const { return n > kMax; }
  size_t bytes() const { return end; }
};
