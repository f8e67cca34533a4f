// Internal C++ launch entry point of the spectral-matching baseline (spectral_kernels.hip).
// Public C ABI: include/gmf_hip.h (gmf_spectral_matching).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace gmf {

constexpr int kSmTile = 128;        // rows per workgroup of the sweep = columns per LDS tile
constexpr int kSmMaxSplits = 32;    // column splits of one pair, at most

// How the column tiles of a pair of n rows are dealt to workgroups: `eff` splits of `chunk` consecutive tiles each (the last may
// be shorter).  From n alone (forced = 0), or from n and the forced count: never from the batch, so a pair's partial sums, and
// with them its bits, are the same alone and in any batch.  n >= 1.
struct SmSplit { int chunk, eff; };
__host__ __device__ inline SmSplit sm_split_plan(int n, int forced) {
  const int tiles = (n + kSmTile - 1) / kSmTile;
  int s = forced > 0 ? forced : (1024 + tiles - 1) / tiles;      // about 1024 workgroups per pair
  const int cap = tiles < kSmMaxSplits ? tiles : kSmMaxSplits;
  s = s < cap ? s : cap;
  SmSplit p;
  p.chunk = (tiles + s - 1) / s;
  p.eff = (tiles + p.chunk - 1) / p.chunk;
  return p;
}
// The largest `eff` any pair of up to max_n rows can have: sizes the partial sums and the grid.
inline int sm_max_splits(int max_n, int forced) {
  const int tiles = (max_n + kSmTile - 1) / kSmTile;
  const int cap = tiles < kSmMaxSplits ? tiles : kSmMaxSplits;
  const int s = forced > 0 && forced < cap ? forced : cap;
  return s < 1 ? 1 : s;
}

inline size_t sm_scratch_floats(long long total_rows, int max_n, int forced) {
  return (size_t)total_rows * (size_t)sm_max_splits(max_n, forced);
}

// corr [total_rows,6], src / tgt [total_rows,3], offsets [B+1] and topk [B] on the device; partial: sm_scratch_floats floats.
// 2 * iterations + 2 launches on `s`, no host synchronisation.
hipError_t launch_spectral_matching(const float* corr, const float* src, const float* tgt, const int* offsets, int B,
                                    long long total_rows, int max_n, float inlier_threshold, const int* topk, int iterations,
                                    int forced_splits, float* partial, float* eig, float* labels, float* T_out,
                                    hipStream_t s);

// k_sm_pose alone, for every caller of rigid_transform_3d with per-row weights eig * labels (the maximum-clique baseline passes
// its 0 / 1 labels as both): T_out [B,16].  One launch.
hipError_t launch_sm_pose(const float* src, const float* tgt, float* eig, float* labels, const int* offsets, int B,
                          long long total_rows, int max_n, float* T_out, hipStream_t s);

}  // namespace gmf
