// Internal C++ launch entry points of the correspondence RANSAC and point-to-point ICP solvers (solver_kernels.hip).
// Public C ABI: include/gmf_hip.h (gmf_ransac_correspondence, gmf_icp_point_to_point, gmf_icp_point_to_point_ex).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launchers_pointcloud.hpp"

namespace gmf {

// Device scratch of one RANSAC call (taken from the handle's workspace by the caller).
struct RansacScratch {
  float4* cs;                 // [total_rows] compacted participating source rows of each pair (pair b from offsets[b])
  float4* cq;                 // [total_rows] the matching target rows
  int* cidx;                  // [total_rows] row number within the pair of each compacted row
  int* m;                     // [B] participating rows per pair
  unsigned* cnt;              // [B * H] inlier count per hypothesis
  unsigned long long* sq;     // [B * H] sum of the inliers' d^2 in units of tau^2 / 2^24 (integer: order-free)
  unsigned char* valid;       // [B * H] 1 = the hypothesis's fit succeeded
  float* thyp;                // [B * H * 12] the hypothesis's [R | t] as scored
};

size_t ransac_scratch_bytes(long long total_rows, int B, int H);
void ransac_scratch_carve(void* base, long long total_rows, int B, int H, RansacScratch& s);
hipError_t launch_ransac(const float* src, const float* tgt, const int* offsets, const unsigned char* mask, int B,
                         long long total_rows, int max_rows, int ransac_n, int H, float tau, uint64_t seed, int first_pair,
                         const RansacScratch& ws, float* T_out, unsigned char* inliers, float* fitness, float* rmse,
                         long long* hypothesis, long long* sample, hipStream_t s);

// Device scratch of one ICP call.
struct IcpScratch {
  unsigned long long* key;    // [total_src] packed (d^2 bits | target row) of each source row's nearest target
  double* T;                  // [B * 12] current [R | t] of each pair in fp64
  double* prev;               // [B * 2] fitness and rmse of the previous pass
  int* done;                  // [B]
};

size_t icp_scratch_bytes(long long total_src, int B);
void icp_scratch_carve(void* base, long long total_src, int B, IcpScratch& s);
// grid: null = the brute-force search (k_icp_nn).  Otherwise a KnnScratch carved for total_tgt rows (all targets of the batch):
// the call builds the hashed grid over the targets first (launch_grid_build) and searches it (k_icp_nn_grid), bit-identically.
hipError_t launch_icp(const float* src, const int* src_off, const float* tgt, const int* tgt_off, int B, long long total_src,
                      int max_src, int max_tgt, const float* init, float tau, int max_iter, double rel_fitness, double rel_rmse,
                      const IcpScratch& ws, float* T_out, float* fitness, float* rmse, int* iterations, long long* nn,
                      hipStream_t s, const KnnScratch* grid = nullptr, long long total_tgt = 0);

}  // namespace gmf
