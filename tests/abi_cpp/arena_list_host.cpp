// Host-only check of the workspace list (gmf_amd/csrc/arena_list.hpp), meant to be built with
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all arena_list_host.cpp
// A made-up scratch struct appends its buffers, some with count 0; a second struct follows it in the same list, as in a call
// that needs two.  The sizing pass gives the block, the carving pass fills the pointers: every buffer must be 256-byte
// aligned, inside the block with its slack, and apart from every other; every byte of every buffer is then written, so an
// under-reservation is a heap overflow the sanitizer reports.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../gmf_amd/csrc/arena_list.hpp"

namespace {

struct Grid {
  int* slot;
  float* pts;
  char* tmp;
};
struct Solver {
  unsigned long long* key;
  double* T;
  unsigned char* board;
  int* optional;
  short* odd;
};

void grid_list(size_t n, size_t tmp_bytes, Grid& g, ArenaList& bufs) {
  bufs.add(g.slot, n);
  bufs.add(g.pts, n * 4);
  bufs.add(g.tmp, tmp_bytes);
}

void solver_list(size_t n, int B, bool with_optional, Solver& s, ArenaList& bufs) {
  bufs.add(s.key, n);
  bufs.add(s.T, (size_t)B * 12);
  bufs.add(s.board, (size_t)B * 13);
  bufs.add(s.optional, with_optional ? n : 0);
  bufs.add(s.odd, n + 1);
}

struct Span { const char* p; size_t bytes; };

int fails = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++fails; } \
  } while (0)

template <typename T>
void touch(std::vector<Span>& spans, T* p, size_t count) {
  if (!p) return;
  std::memset(p, 0x5A, count * sizeof(T));
  spans.push_back({reinterpret_cast<const char*>(p), count * sizeof(T)});
}

void run(size_t n, int B, size_t tmp_bytes, bool with_optional) {
  Solver s;
  Grid g;
  ArenaList bufs;
  solver_list(n, B, with_optional, s, bufs);
  grid_list(n, tmp_bytes, g, bufs);
  CHECK(!bufs.overflowed());
  const size_t need = bufs.bytes();
  char* block = static_cast<char*>(std::aligned_alloc(256, need ? need : 256));
  bufs.place(block);

  CHECK((s.optional != nullptr) == with_optional);
  CHECK((g.tmp != nullptr) == (tmp_bytes != 0));
  std::vector<Span> spans;
  touch(spans, s.key, n);
  touch(spans, s.T, (size_t)B * 12);
  touch(spans, s.board, (size_t)B * 13);
  touch(spans, s.optional, with_optional ? n : 0);
  touch(spans, s.odd, n + 1);
  touch(spans, g.slot, n);
  touch(spans, g.pts, n * 4);
  touch(spans, g.tmp, tmp_bytes);
  for (size_t i = 0; i < spans.size(); ++i) {
    CHECK((reinterpret_cast<uintptr_t>(spans[i].p) & 255) == 0);
    CHECK(spans[i].p >= block && spans[i].p + spans[i].bytes <= block + need);
    // list order is address order
    if (i) CHECK(spans[i - 1].p + spans[i - 1].bytes <= spans[i].p);
  }
  std::free(block);
}

}  // namespace

int main() {
  for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1000})
    for (int B : {1, 3})
      for (size_t tmp : {(size_t)0, (size_t)1, (size_t)256, (size_t)4097})
        for (bool opt : {false, true}) run(n, B, tmp, opt);

  // an empty list and a list of empty buffers need nothing and set null
  {
    ArenaList none;
    CHECK(none.bytes() == 0);
    int* a = reinterpret_cast<int*>(1);
    ArenaList empty{arena_buf(a, 0)};
    CHECK(empty.bytes() == 0);
    empty.place(nullptr);
    CHECK(a == nullptr);
  }
  // one buffer too many is remembered, not written past the array
  {
    int* p[ArenaList::kMax + 1];
    ArenaList full;
    for (int i = 0; i <= ArenaList::kMax; ++i) full.add(p[i], 1);
    CHECK(full.overflowed());
  }
  std::printf(fails ? "arena_list_host: %d checks failed\n" : "arena_list_host: ok\n", fails);
  return fails ? 1 : 0;
}
