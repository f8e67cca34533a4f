// Internal C++ launch entry points of correspondence_kernels.hip: PointDSC's correspondence set from descriptors and keypoints
// (mutual nearest neighbours, compaction, labels, centring) for B ragged pairs.
// Public C ABI: include/gmf_hip.h (gmf_nn_match_mutual_batched, gmf_build_correspondences).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "corr_plan.hpp"
#include "launchers.hpp"

namespace gmf {

struct CorrArgs {
  // inputs: the packed descriptors and (build only) keypoints of the batch, the matching tables of plan_nn_match_batched and the
  // chunk table of corr_plan_chunks, all on the device
  const float* F0 = nullptr;
  const float* F1 = nullptr;
  const float* kp0 = nullptr;            // [rows0, 3]; null: flags only (gmf_nn_match_mutual_batched)
  const float* kp1 = nullptr;            // [rows1, 3]
  const MatchPair* tab = nullptr;        // [B + 1]
  const CorrChunk* chunks = nullptr;     // [n_chunks]
  const int* pair_chunk0 = nullptr;      // [B + 1]
  int B = 0, d = 0, n_chunks = 0, n_keys = 0;   // n_keys: key rows of the batch (off1[B])
  int use_mutual = 1, in_dim = 6;
  const float* gt_trans = nullptr;       // [B, 4, 4] row-major; null: no labels
  float inlier_threshold = 0.f;
  // workspace
  float* f0_img = nullptr;
  float* f1_img = nullptr;
  float* norm2 = nullptr;
  unsigned long long* best = nullptr;    // [rows0]
  unsigned long long* colbest = nullptr; // [n_keys] (use_mutual)
  int* rank = nullptr;                   // [rows0] a flagged row's position among its chunk's flagged rows
  int* chunk_cnt = nullptr;              // [n_chunks]
  float* chunk_sum = nullptr;            // [n_chunks, 6]
  int* chunk_excl = nullptr;             // [n_chunks] exclusive offsets inside the pair
  float* mean = nullptr;                 // [B, 6]
  // per source row
  int* idx = nullptr;                    // [rows0] local to the pair
  float* dist = nullptr;                 // [rows0]
  unsigned char* mutual = nullptr;       // [rows0]
  // outputs of capacity rows0 (build only)
  int* out_offsets = nullptr;            // [B + 1]
  long long* corr = nullptr;             // [., 2]
  float* src_out = nullptr;              // [., 3]
  float* tgt_out = nullptr;              // [., 3]
  float* corr_pos = nullptr;             // [., in_dim]
  float* src_desc_out = nullptr;         // [., d] or null
  float* tgt_desc_out = nullptr;
  float* labels = nullptr;               // [.] or null
};

// prep, sweep (two-sided with use_mutual) and k_corr_flag: idx, dist, mutual and, with keypoints, the chunk partials
hipError_t launch_corr_match(const CorrArgs& a, const MatchTotals& tot, hipStream_t s);
// k_corr_scan and k_corr_emit behind launch_corr_match
hipError_t launch_corr_emit(const CorrArgs& a, hipStream_t s);

}  // namespace gmf
