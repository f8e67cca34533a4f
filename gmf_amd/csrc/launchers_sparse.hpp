// Internal C++ launch entry points of the sparse coordinate engine and the sparse convolution (sparse_kernels.hip).
// Public C ABI: include/gmf_hip.h (gmf_sparse_plan_bytes, gmf_sparse_build_plan, gmf_sparse_conv, gmf_sparse_conv_narrow,
// gmf_sparse_head_l2, gmf_sparse_pack_resunet).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sparse_conv_plan.hpp"

namespace gmf {

constexpr int kSparseMaxD = 6;          // spatial dimensions (the batch index is column 0 on top)
constexpr int kSparseMaxK = 1024;       // kernel volume k^D (the per-tile offset bitmap is 1024 bits)
constexpr int kSparseMaxLevels = 8;     // tensor strides 1, 2, 4, ..., 2^(levels - 1)
constexpr int kSparseMaxMaps = 16;
constexpr int kSparseKeyInts = 8;       // a row of a level: (batch, c_1 .. c_D, 0 ...), 8 int32

// One kernel map of a plan: output rows of level `out` read input rows of level `in` (|out - in| <= 1) through a hypercube of
// edge k.  Same level: o + d t.  Down (out = in + 1): o + d t, t the input stride.  Transposed (out = in - 1): o - d t, t the
// output stride, so fine output p reads coarse input o when p = o + d t.
struct SparseMapDesc { int k, out, in; };

// Byte offsets of the pieces of one plan inside its device block; a pure function of (M, D, levels, maps).
struct SparsePlanLayout {
  long long M = 0, T = 0;                  // rows of every level's buffers (the input row count), hash-table slots
  int D = 0, levels = 0, nmaps = 0;
  SparseMapDesc maps[kSparseMaxMaps];
  int K[kSparseMaxMaps];
  size_t counts = 0;                       // int [16]: rows of level l at [l]
  size_t coords[kSparseMaxLevels];         // int [M][8] each
  size_t table[kSparseMaxLevels];          // int [T] each (row index, -1 empty)
  size_t keys = 0, idx_a = 0, idx_b = 0, flags = 0, pos = 0, tmp = 0, tmp_bytes = 0;
  size_t row_ptr[kSparseMaxMaps];          // int [M + 1] each (CSR over output rows)
  size_t pairs[kSparseMaxMaps];            // int2 [M * K] each: (offset index, input row), ascending offset per output row
  size_t by_off[kSparseMaxMaps];           // int [M * K] each: CSR pair indices sorted by offset, ascending row within one
  size_t off_start[kSparseMaxMaps];        // int [K + 1] each: offset d's pairs are by_off[off_start[d] .. off_start[d + 1])
  size_t skeys_a = 0, skeys_b = 0, svals = 0;   // the offset sort's keys and values (M * max K each)
  size_t total = 0;
};

bool sparse_plan_layout(long long M, int D, int levels, int nmaps, const SparseMapDesc* maps, SparsePlanLayout& lay);
// Builds every level and every kernel map of `lay` in `base` from coords [M, 1 + D] int32.  A duplicate input row ORs
// `dup_bit` into *status.  No host synchronisation.
hipError_t launch_sparse_build_plan(const int* coords, const SparsePlanLayout& lay, char* base, int* status, int dup_bit,
                                    hipStream_t s);

// y[o] = epilogue(sum over the pairs (d, i) of row o, d ascending, of [xa | xb][i] W[d]).  row_ptr == nullptr: the identity map
// (K = 1, row o reads row o).  n_out: device row count; rows cap_out and beyond are never touched.  Otherwise the offsets are cut
// into nsplit fixed slices; each slice's workgroups walk the offset-major pair lists (by_off, off_start) and write per-slice
// partial rows (`partial`: nsplit * cap_out * cout floats), which k_split_reduce adds in slice order before the epilogue.
struct SparseConvArgs {
  const int* row_ptr; const int2* pairs; const int* by_off; const int* off_start; int K;
  const int* n_out; long long cap_out;
  const float* xa; int ca; const float* xb; int cb;
  const float* W; int cout;
  const float* scale; const float* shift; const float* residual; int relu;
  int nsplit; float* partial;
  float* y;
};
// grid: (nsplit, 64-channel blocks, sparse_conv_row_groups(..)) - sparse_conv_plan.hpp
hipError_t launch_sparse_conv(const SparseConvArgs& a, hipStream_t s);

// Narrow-input convolution (FCGF's conv1: Cin = 1, k = 7): y[o] = epilogue(one fma chain over the CSR pairs (d, i) of row o,
// d ascending, input channels in order within a pair, of x[i][k] W[d][k][c]).  Each output row is computed whole by one group
// of lanes; W sits in LDS when it fits (sparse_narrow_lds, sparse_conv_plan.hpp), else it is read from global memory.
constexpr int kSparseNarrowMaxCin = 8;
constexpr int kSparseNarrowMaxCout = 64;
struct SparseNarrowArgs {
  const int* row_ptr; const int2* pairs; int K;
  const int* n_out; long long cap_out;
  const float* x; int cin;
  const float* W; int cout;
  const float* scale; const float* shift; const float* residual; int relu;
  float* y;
};
hipError_t launch_sparse_conv_narrow(const SparseNarrowArgs& a, hipStream_t s);

// Fused FCGF head: per row h = relu([xa | xb] W1) (W1 [ca + cb, hid]), y = h W2 + bias (W2 [hid, cout]), then, if normalize,
// y / (||y||_2 + 1e-8).  One wave per row; both weight blocks in LDS.
constexpr int kSparseHeadMaxC = 64;     // ca, cb, hid and cout each
struct SparseHeadArgs {
  const int* n_out; long long cap_out;
  const float* xa; int ca; const float* xb; int cb;
  const float* W1; int hid; const float* W2; int cout; const float* bias;
  int normalize;
  float* y;
};
hipError_t launch_sparse_head_l2(const SparseHeadArgs& a, hipStream_t s);

}  // namespace gmf
