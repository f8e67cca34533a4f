// The hypothesis sampler of gmf_ransac_correspondence: counter-based, so that hypothesis h of pair b draws the same rows whatever
// the launch shape, the batch it runs in or the order workgroups run in.  tests/test_solvers_host.py and tests/test_gpu_solvers.py
// restate it in numpy; a change here is a change of the public contract.
//
//   key   = seed ^ splitmix64((uint64)pair << 32 | h)
//   u(c)  = splitmix64(key ^ c * 0x9E3779B97F4A7C15)          c = 0, 1, 2, ... one counter for the whole sample
//   row   = (u >> 32) * M >> 32                                M = the pair's participating rows
// Slot k takes draws until its row differs from slots 0 .. k-1; after 64 redraws (65 draws) the repeat is kept.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmf {

__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

constexpr int kRansacRedraws = 64;

template <int NS>
__host__ __device__ inline void ransac_draw(uint64_t seed, uint32_t pair, uint32_t h, uint32_t M, int* rows) {
  const uint64_t key = seed ^ splitmix64(((uint64_t)pair << 32) | h);
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    int row = 0;
    for (int r = 0; r <= kRansacRedraws; ++r) {
      const uint64_t u = splitmix64(key ^ (c * 0x9E3779B97F4A7C15ull));
      ++c;
      row = (int)(((u >> 32) * (uint64_t)M) >> 32);
      bool rep = false;
#pragma unroll
      for (int j = 0; j < k; ++j) rep |= rows[j] == row;
      if (!rep) break;
    }
    rows[k] = row;
  }
}

}  // namespace gmf
