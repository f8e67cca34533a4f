// Shared by match_kernels.hip and correspondence_kernels.hip: the pair lookup of the batched matching kernels and the two halves of
// launch_nn_match_batched (launchers.hpp) that the correspondence chain runs on its own.
#pragma once
#include "mfma_core.hpp"
#include "launchers.hpp"

namespace gmf {

// the pair whose range holds v: the largest b < B with begin(b) <= v (pairs with an empty range share their begin with the next)
template <typename F>
GMF_DEVINL int match_pair_of(int B, long v, F begin) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((long)begin(mid) <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// k_match_prep_batched: the images, the key norms and best = all ones; with `colbest`, its n_col words (one per key row of the batch)
// are set to all ones as well, in the same launch
hipError_t launch_match_prep_batched(const float* F0, const float* F1, float* f0_img, float* f1_img, float* norm2, unsigned long long* best,
                                     unsigned long long* colbest, int n_col, const MatchPair* tab, int B, const MatchTotals& tot, int d,
                                     int mode, hipStream_t s);
// k_nn_match_batched over the prepared images
hipError_t launch_match_sweep_batched(const float* f0_img, const float* f1_img, const float* norm2, unsigned long long* best,
                                      const MatchPair* tab, int B, const MatchTotals& tot, int d, hipStream_t s);

}  // namespace gmf
