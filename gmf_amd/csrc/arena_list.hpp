// The list of device buffers one call takes from the handle's workspace.  No handle and no HIP here: the launcher headers
// name ArenaList so that a scratch struct can append its own buffers, and api_common.hpp's arena_carve places the list.
#pragma once
#include <stddef.h>

#include <initializer_list>

// One buffer of a call's workspace: `count` elements of T into `*slot` (count 0: no buffer, *slot = null).  A call lists its buffers
// once, in arena_carve: the reservation is the sum of the list and the carving follows it, so the two cannot disagree.
struct ArenaBuf { void* slot; size_t count, elem; void (*set)(void* slot, char* p); };
template <typename T>
ArenaBuf arena_buf(T*& slot, size_t count) {
  return {&slot, count, sizeof(T), [](void* sl, char* p) { *static_cast<T**>(sl) = reinterpret_cast<T*>(p); }};
}

struct ArenaList {
  static constexpr int kMax = 32;      // the largest call lists 22; arena_carve refuses a list that overflowed
  ArenaBuf v[kMax];
  int n = 0;
  ArenaList() = default;
  ArenaList(std::initializer_list<ArenaBuf> bufs) { for (const ArenaBuf& b : bufs) add(b); }
  void add(const ArenaBuf& b) { if (n < kMax) v[n] = b; ++n; }
  template <typename T>
  void add(T*& slot, size_t count) { add(arena_buf(slot, count)); }
  bool overflowed() const { return n > kMax; }

  // every buffer starts on a 256-byte boundary and is reserved with 256 bytes of slack behind it
  static size_t align256(size_t v) { return (v + 255) / 256 * 256; }
  size_t bytes() const {
    size_t need = 0;
    for (int i = 0; i < n && i < kMax; ++i) need += v[i].count ? align256(v[i].count * v[i].elem) + 256 : 0;
    return need;
  }
  // base: 256-byte aligned, bytes() long
  void place(void* base) const {
    size_t used = 0;
    for (int i = 0; i < n && i < kMax; ++i) {
      const ArenaBuf& b = v[i];
      const size_t off = align256(used);
      if (b.count) used = off + b.count * b.elem;
      b.set(b.slot, b.count ? static_cast<char*>(base) + off : nullptr);
    }
  }
};
