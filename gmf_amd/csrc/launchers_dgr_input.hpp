// Internal C++ launch entry points of dgr_input_kernels.hip: the ground-truth pair search and the assembly of the inlier
// network's batched input (rows, features, labels) of DGR's training step.
// Public C ABI: include/gmf_hip.h (gmf_matching_indices_count, gmf_matching_indices_fill, gmf_inlier_input).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace gmf {

constexpr int kInlierMaxFeat = 64;      // widest descriptor of the 'feats' inlier features (FCGF's head: out_channels <= 64)

size_t matching_indices_scan_bytes(long long n0);
// count pass, exclusive scan and the per-pair ranges: cnt [n0 + 1] int (scratch), row_start [n0 + 1] and pair_offsets [B + 1] int64
hipError_t launch_matching_indices_count(const float* xyz0, const int* off0, const float* xyz1, const int* off1, int B, long long n0,
                                         const double* T, double r2, int* cnt, void* scan_tmp, size_t scan_bytes, long long* row_start,
                                         long long* pair_offsets, hipStream_t s);
// fill pass: pairs [row_start[n0], 2] int64
hipError_t launch_matching_indices_fill(const float* xyz0, const int* off0, const float* xyz1, const int* off1, int B, long long n0,
                                        const double* T, double r2, const long long* row_start, long long* pairs, hipStream_t s);

struct InlierInput {
  // the predicted pairs of the batch, M rows in all: `nn` [M] (row m of pair b is source row m - off0[b], its match nn[m], local to
  // the pair; pred_out [M, 2] int64 then receives the pairs), or else `pred` [M, 2] int64 as given
  const int* nn = nullptr;
  const long long* pred = nullptr;
  const int* off0 = nullptr;            // [B + 1] rows of the pairs in M (and, with `nn`, in the source tensors)
  const int* off1 = nullptr;            // [B + 1] rows of the pairs in the target tensors
  int B = 0;
  long long M = 0;
  long long* pred_out = nullptr;
  // rows and features (coords_out null: neither)
  const int* c0 = nullptr;              // [*, 4] (batch, x, y, z)
  const int* c1 = nullptr;
  int* coords_out = nullptr;            // [M, 7]
  int feat_type = 0;                    // 0 ones [M, 1]; 1 feats [M, 2 c]; 2 coords [M, 6]
  const float* a0 = nullptr;            // feats: F0 [*, c], F1 [*, c]; coords: xyz0, xyz1 [*, 3]
  const float* a1 = nullptr;
  int c = 0;
  float* feats_out = nullptr;
  // labels (labels_out null: none)
  const long long* pos_keys = nullptr;  // the positive keys, sorted inside each pair's range
  const long long* pos_off = nullptr;   // [B + 1]
  const long long* seeds = nullptr;     // [B]
  unsigned char* labels_out = nullptr;  // [M] 0 / 1
};
hipError_t launch_inlier_input(const InlierInput& in, hipStream_t s);

}  // namespace gmf
