// The chunk table of the correspondence chain (correspondence_kernels.hip): every pair's source rows cut into chunks of kCorrChunk
// rows, counted from the pair's first row, so that a chunk never holds rows of two pairs and a pair's chunks do not depend on its
// neighbours in the batch.  No handle and no HIP here: the plan is plain host code, compiled and tested on its own
// (tests/abi_cpp/corr_plan_host.cpp).
#pragma once
#include <stddef.h>

namespace gmf {

constexpr int kCorrChunk = 256;      // rows per chunk = threads of the workgroup that owns it

// rows [row0, row0 + n) of the packed source rows, all of pair `pair`; `first`: 1 on the pair's first chunk
struct CorrChunk { int pair, row0, n, first; };

// the number of chunks of a batch: off0 [B + 1] ascending row offsets from 0
inline long corr_chunk_count(const int* off0, int B) {
  long n = 0;
  for (int b = 0; b < B; ++b) n += ((long)off0[b + 1] - off0[b] + kCorrChunk - 1) / kCorrChunk;
  return n;
}

// chunks [corr_chunk_count] in row order and pair_chunk0 [B + 1]: pair b owns chunks [pair_chunk0[b], pair_chunk0[b + 1]) (none for a
// pair without rows).  Returns the number of chunks written.
inline long corr_plan_chunks(const int* off0, int B, CorrChunk* chunks, int* pair_chunk0) {
  long c = 0;
  for (int b = 0; b < B; ++b) {
    pair_chunk0[b] = (int)c;
    for (long r = off0[b]; r < off0[b + 1]; r += kCorrChunk) {
      const int left = (int)(off0[b + 1] - r);
      chunks[c++] = CorrChunk{b, (int)r, left < kCorrChunk ? left : kCorrChunk, r == off0[b] ? 1 : 0};
    }
  }
  pair_chunk0[B] = (int)c;
  return c;
}

}  // namespace gmf
