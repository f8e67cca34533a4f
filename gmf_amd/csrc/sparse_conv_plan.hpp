// What decides the geometry of a sparse launch (sparse_kernels.hip, sparse_train_kernels.hip): the offset slices and output-row
// groups of k_sparse_conv, the lane-group width, grid and weight placement of the narrow-input kernels, the head's grid, the slot
// count and chunk length of the weight gradients, the row chunks of the masked BatchNorm.  No HIP here: plain integer functions,
// compiled for the device too when a HIP compiler reads them, and tested as host code on their own
// (tests/abi_cpp/sparse_plan_host.cpp over tests/golden/sparse_forms_table.txt).  None of them changes a result, only which
// workgroup computes it - except nsplit, P and the BatchNorm chunks, which fix the grouping of a sum and are functions of the
// shape alone.
#pragma once

#if defined(__HIPCC__)
#define GMF_PLAN_FN __host__ __device__ inline
#else
#define GMF_PLAN_FN inline
#endif

namespace gmf {

constexpr int kSparseWgThreads = 256;                       // every sparse kernel but the narrow wgrad (one wave)
constexpr int kSparseWgWaves = kSparseWgThreads / 64;
constexpr int kSparseConvTile = 64;                         // k_sparse_conv: 64 pairs x 64 output channels per tile

// ---- k_sparse_conv -------------------------------------------------------------------------------------------------------------

// offset slices: slice(d) = d nsplit / K, so slice s holds d in [ceil(K s / nsplit), ceil(K (s + 1) / nsplit))
GMF_PLAN_FN int slice_of(int d, int nsplit, int K) { return (int)((long long)d * nsplit / K); }
GMF_PLAN_FN int slice_begin(int s, int nsplit, int K) { return (int)(((long long)K * s + nsplit - 1) / nsplit); }

// Output-row groups of one convolution (gridDim.z).  A kernel of more than 16 MiB is read once (one row group); a smaller one may
// be re-read per group, from the caches, to fill the device.  The grouping decides only which workgroup computes a row.
GMF_PLAN_FN int sparse_conv_row_groups(int K, int cin, int cout, int nsplit, long long cap_out) {
  if ((long long)K * cin * cout * 4 > (16LL << 20)) return 1;
  const long long wgs = (long long)nsplit * ((cout + kSparseConvTile - 1) / kSparseConvTile);
  long long g = (512 + wgs - 1) / wgs;
  const long long rows = (cap_out + 127) / 128;
  if (g > rows) g = rows;
  return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}
// group grp of `groups` owns the output rows [begin(grp), begin(grp + 1)) of the n_out valid ones (none when n_out < groups)
GMF_PLAN_FN int sparse_conv_group_begin(int n_out, int grp, int groups) { return (int)((long long)n_out * grp / groups); }

// ---- k_sparse_conv_narrow, k_sparse_wgrad_narrow ----------------------------------------------------------------------------------

constexpr long long kSparseNarrowLdsBytes = 64 << 10;
// lanes per output row (forward) or per pair group (wgrad): the fewest of 16, 32, 64 that cover cout
GMF_PLAN_FN int sparse_narrow_lanes(int cout) { return cout <= 16 ? 16 : (cout <= 32 ? 32 : 64); }
GMF_PLAN_FN int sparse_narrow_rows_per_wg(int cout) { return kSparseWgWaves * (64 / sparse_narrow_lanes(cout)); }
// W [K][cin][cout] staged in LDS (true) or read from global memory
GMF_PLAN_FN bool sparse_narrow_lds(int K, int cin, int cout) { return (long long)K * cin * cout * 4 <= kSparseNarrowLdsBytes; }
// Workgroups walk the rows in strides; with W in LDS each one stages it once, so the grid stays near 3 per CU (3 x 43 KiB for
// FCGF's conv1 fit the 160 KiB of a CU).
GMF_PLAN_FN int sparse_narrow_grid(long long cap_out, int K, int cin, int cout) {
  const int per = sparse_narrow_rows_per_wg(cout);
  const long long g = (cap_out + per - 1) / per, cap = sparse_narrow_lds(K, cin, cout) ? 768 : 4096;
  return (int)(g > cap ? cap : g);
}

// ---- k_sparse_head_l2: one wave per row, strided ----------------------------------------------------------------------------------

GMF_PLAN_FN int sparse_head_grid(long long cap_out) {
  const long long g = (cap_out + kSparseWgWaves - 1) / kSparseWgWaves;
  return (int)(g > 1024 ? 1024 : g);
}

// ---- weight gradients -------------------------------------------------------------------------------------------------------------

constexpr int kWgradMinChunk = 64;
GMF_PLAN_FN int sparse_wgrad_slots(int K) { return K + (K > 256 ? K : 256); }
GMF_PLAN_FN int sparse_wgrad_narrow_slots(int K) { return K + 2048; }
// pairs per chunk of a map of nnz pairs: sum over d of ceil(n_d / P) <= nnz / P + K <= nslots
GMF_PLAN_FN int sparse_wgrad_chunk(long long nnz, int K, int nslots) {
  const long long extra = nslots - K;
  const long long P = (nnz + extra - 1) / extra;
  return (int)(P < kWgradMinChunk ? kWgradMinChunk : P);
}

// ---- BatchNorm over a level's valid rows ------------------------------------------------------------------------------------------

// fixed row chunks of the cap row slots: chunk ch covers the rows [begin(ch), begin(ch + 1)), cut at the valid-row count
GMF_PLAN_FN int bnm_chunks(long long cap) {
  const long long c = (cap + 255) / 256;
  return (int)(c > 64 ? 64 : c);
}
GMF_PLAN_FN long long bnm_chunk_begin(long long cap, int ch, int nch) { return cap * ch / nch; }

}  // namespace gmf
