// Internal C++ launch entry points of the correspondence RANSAC, point-to-point ICP and feature-matching RANSAC solvers
// (solver_kernels.hip).
// Public C ABI: include/gmf_hip.h (gmf_ransac_correspondence, gmf_icp_point_to_point, gmf_icp_point_to_point_ex,
// gmf_icp_point_to_plane, gmf_icp_colored, gmf_ransac_feature_matching).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "icp_plane_plan.hpp"
#include "launchers_pointcloud.hpp"

namespace gmf {

// Device scratch of one RANSAC call (taken from the handle's workspace by the caller).
struct RansacScratch {
  float4* cs;                 // [total_rows] compacted participating source rows of each pair (pair b from offsets[b])
  float4* cq;                 // [total_rows] the matching target rows
  int* cidx;                  // [total_rows] row number within the pair of each compacted row
  int* m;                     // [B] participating rows per pair
  unsigned char* board;       // the scoreboard of the B * H hypotheses, cleared by one memset (RansacBoard, solver_kernels.hip)
  float* thyp;                // [B * H * 12] the hypothesis's [R | t] as scored
};

// Appends the scratch to a call's workspace list (arena_carve then fills the pointers).
void ransac_scratch_list(long long total_rows, int B, int H, RansacScratch& s, ArenaList& bufs);
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

// What the point-to-plane estimator adds to an ICP call: the targets' normals, the plan of its split step and the partials.
struct IcpPlaneScratch {
  const float* normals;       // [total_tgt, 3] the caller's, used as given
  IcpPlanePlan plan;
  double* part;               // [plan.partial_doubles]
};

// What coloured ICP adds to a point-to-plane call: one intensity per source and per target row, the targets' colour gradients
// (launch_color_gradient), and the square roots of the two weights, taken on the host in double.
struct IcpColorTerms {
  const float* src_intensity;   // [total_src]
  const float* tgt_intensity;   // [total_tgt]
  const float* tgt_gradients;   // [total_tgt, 3]
  double sqrt_geometric;        // sqrt(lambda_geometric)
  double sqrt_photometric;      // sqrt(1 - lambda_geometric)
};

void icp_scratch_list(long long total_src, int B, IcpScratch& s, ArenaList& bufs);
void icp_plane_scratch_list(IcpPlaneScratch& s, ArenaList& bufs);    // s.plan filled by icp_plane_plan
// grid: null = the brute-force search (k_icp_nn).  Otherwise a KnnScratch listed for total_tgt rows (all targets of the batch):
// the call builds the hashed grid over the targets first (launch_grid_build) and searches it (k_icp_nn_grid), bit-identically.
// plane: null = point-to-point (k_icp_step).  Otherwise each pass ends with k_icp_plane_partials and k_icp_plane_solve instead,
// and max_src must bound every pair's source rows (a pair that exceeds it comes back with NaN in T_out and iterations -1).
// color (with plane): coloured ICP, k_icp_color_partials in the place of k_icp_plane_partials.
hipError_t launch_icp(const float* src, const int* src_off, const float* tgt, const int* tgt_off, int B, long long total_src,
                      int max_src, int max_tgt, const float* init, float tau, int max_iter, double rel_fitness, double rel_rmse,
                      const IcpScratch& ws, float* T_out, float* fitness, float* rmse, int* iterations, long long* nn,
                      hipStream_t s, const KnnScratch* grid = nullptr, long long total_tgt = 0,
                      const IcpPlaneScratch* plane = nullptr, const IcpColorTerms* color = nullptr);

// Device scratch of one feature-matching RANSAC call.  H = max_iteration, V = max_validation.
struct FmScratch {
  unsigned char* pass;        // [B, H rounded up to 4] 1 = hypothesis h passed the checkers (zeroed by the launcher)
  float* thyp;                // [B * H * 12] the fp32 [R | t] of a passing hypothesis
  int* hyp;                   // [B * V] the validated h in increasing order, -1 padded (the caller may point it at an output)
  unsigned* cnt;              // [B * V] |C| of each validated hypothesis (likewise)
  unsigned long long* sq;     // [B * V] sum over C of d^2 in units of tau^2 / 2^24 (likewise)
  float* tval;                // [B * V * 12] the validated hypotheses' poses
  int* win;                   // [B] list position of the winner, -1: none
  unsigned long long* key;    // [total_src] the winner's packed (d^2 bits | target row) per source row
};

void fm_scratch_list(long long total_src, int B, int H, int V, FmScratch& s, ArenaList& bufs);
// nn [total_src]: the feature-space nearest target row of every source row, numbered within the pair.  checker_distance < 0 and
// edge_length <= 0 switch the checkers off.  grid: null = every target streams through LDS; otherwise a KnnScratch listed for
// total_tgt rows, built here (launch_grid_build) and searched, bit-identically.  validated [B]: hypotheses evaluated per pair.
hipError_t launch_ransac_feature_matching(const float* src, const int* src_off, const float* tgt, const int* tgt_off,
                                          const long long* nn, int B, long long total_src, long long total_tgt, int max_src,
                                          int ransac_n, int H, int V, float tau, float checker_distance, float edge_length,
                                          uint64_t seed, int first_pair, const FmScratch& ws, const KnnScratch* grid, float* T_out,
                                          float* fitness, float* rmse, long long* hypothesis, long long* sample, long long* nn_out,
                                          int* validated, hipStream_t s);

}  // namespace gmf
