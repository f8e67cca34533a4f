// Internal C++ launch entry points of the sparse network's training kernels (sparse_train_kernels.hip).
// Public C ABI: include/gmf_hip.h (gmf_sparse_conv_wgrad, gmf_batchnorm_masked_forward, gmf_batchnorm_masked_backward; FCGF's
// training: gmf_sparse_conv_narrow_wgrad, gmf_rownorm_eps, gmf_hardest_contrastive_forward / _backward, gmf_rows_sum_by_dest).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "sparse_conv_plan.hpp"

namespace gmf {

// Weight gradient of one sparse convolution: dW[d] = sum over the pairs (d, i -> o) of map (row_ptr, pairs, by_off, off_start)
// of [xa | xb][i]^T dy[o], dW [K, ca + cb, cout].  row_ptr == nullptr: the identity map (K = 1, pair j = row j).
// k_wgrad_plan cuts every offset's pair list (by_off[off_start[d] ..]) into chunks of P pairs, P = max(kWgradMinChunk,
// ceil(nnz / (nslots - K))) with nnz the map's pair count, so the chunks fit the nslots slots; chunk_info[d] (d = 0..K) is the
// first slot of offset d.  k_sparse_wgrad gives each slot its own workgroups (64 x 64 tiles of dW[d]) and writes the chunk's
// sum into partial[slot]; k_wgrad_reduce adds an offset's chunks in chunk order (zero for an offset without pairs).  Every
// element's order depends only on the map and nslots (a function of K): bitwise repeatable, no float atomics.  kWgradMinChunk,
// sparse_wgrad_slots, sparse_wgrad_narrow_slots and the chunk length sparse_wgrad_chunk: sparse_conv_plan.hpp.
struct SparseWgradArgs {
  const int* row_ptr; const int2* pairs; const int* by_off; const int* off_start; int K;
  const int* n_out;
  const float* xa; int ca; const float* xb; int cb;
  const float* dy; int cout;
  int nslots; int* chunk_info; float* partial;
  float* dW;
};
hipError_t launch_sparse_wgrad(const SparseWgradArgs& a, hipStream_t s);

// Weight gradient of a narrow-input convolution (k_sparse_conv_narrow's counterpart; FCGF's conv1): a.ca = Cin <= 8, a.cb = 0,
// a.cout <= 64, a map of a plan (no identity form).  The chunks are k_wgrad_plan's over sparse_wgrad_narrow_slots(K) slots (a
// slot's partial is only Cin x Cout floats, so there are many and the chunks are short); one wave owns a slot: its 64 lanes
// resolve 64 pairs of the chunk at a time (output row by binary search in row_ptr, input row, the Cin input values), then walk
// them with lane = output channel, the dy row read coalesced and the input values broadcast, Cin accumulators per lane.  With
// Cout <= 32 (<= 16) the wave holds 2 (4) lane groups and group g takes pairs g, g + G, .. of the chunk.  Order of every
// element: one fma chain per group over its pairs in pair order, the groups added in group order, then k_wgrad_reduce adds an
// offset's chunks in chunk order.  No float atomics.
constexpr int kWgradNarrowMaxCin = 8;
constexpr int kWgradNarrowMaxCout = 64;
hipError_t launch_sparse_wgrad_narrow(const SparseWgradArgs& a, hipStream_t s);

// FCGF's row normalisation y = x / (||x||_2 + 1e-8) on x [rows, C] (resunet.py:647-648) and its backward, one wave per row.
// forward: nrm[r] = sqrt(sum_c x_c^2) (lane-strided fma chains, butterfly sum), out = y.  backward: out = dx = dy / s - x <x, dy> /
// (nrm s^2) with s = nrm + 1e-8; a row with nrm == 0 gets y = 0 and dx = 0.
hipError_t launch_rownorm_eps(bool backward, const float* x, const float* dy, float* nrm, float* out, long long rows, int C,
                              hipStream_t s);

// Hardest-contrastive loss of FCGF (include/gmf_hip.h: gmf_hardest_contrastive_forward).  k_hcl_mine: one workgroup per (sampled
// positive k, side); every thread scores its candidates s = tid, tid + 256, .. as one fma chain of squared differences over the
// channels in order and keeps its first minimum, the workgroup takes the minimum with the smaller position on a tie.  The winner's
// score is that chain, so D = sqrt(score + 1e-7) is the distance "recomputed from differences".  k_hcl_reduce: one workgroup,
// thread-strided sums added by a fixed tree.
struct HclArgs {
  const float* F0; const float* F1; int N0, N1, C;
  const long long* pairs; long long K; const long long* keys;      // keys: sorted i + j * max(N0, N1) of all K pairs
  const long long* pos_sel; int P;                                  // NULL: k -> pair k (P == K)
  const long long* sel0; int H0; const long long* sel1; int H1;
  float pos_thresh, neg_thresh;
  long long* h01; long long* h10; unsigned char* keep0; unsigned char* keep1; float* D01; float* D10;
  float* terms;                                                     // [3][P]: the positive hinge, side 0's and side 1's negative hinge^2
  float* out;                                                       // pos_loss, neg_loss, count of keep0, count of keep1
  int* status; int status_bit;
};
hipError_t launch_hcl_forward(const HclArgs& a, hipStream_t s);
// The loss's backward, first half: for every k three gradient rows per side and their destination rows.  rows0 [3P, C] / dest0
// [3P] (into F0): 3k the positive term -> i_k, 3k + 1 side 0's negative term -> i_k, 3k + 2 side 1's negative term -> h10_k; rows1
// / dest1 likewise (-> j_k, j_k, h01_k).  An inactive hinge or a dropped row writes a zero row.  g_pos / g_neg: device scalars.
struct HclBwdArgs {
  const float* F0; const float* F1; int N0, N1, C;
  const long long* pairs; long long K; const long long* pos_sel; int P;
  const long long* h01; const long long* h10; const unsigned char* keep0; const unsigned char* keep1;
  const float* D01; const float* D10; const float* terms; const float* out; float neg_thresh;
  const float* g_pos; const float* g_neg;
  float* rows0; long long* dest0; float* rows1; long long* dest1;
};
hipError_t launch_hcl_backward(const HclBwdArgs& a, hipStream_t s);
// out[r] = sum over e in [row_start[r], row_start[r + 1]) of rows[order[e]], added in that order (a CSR by destination row from
// a stable sort: bitwise repeatable, no float atomics).  rows [E, C], C <= 64, out [N, C].
hipError_t launch_rows_sum_by_dest(const float* rows, long long E, const long long* order, const long long* row_start, long long N,
                                   int C, float* out, hipStream_t s);

// BatchNorm1d in training mode over the first *n rows of x [cap, C] (the valid rows of a sparse level).  Forward: y =
// relu?(gamma (x - mean) rstd + beta + residual?) for rows < *n, 0 beyond; running statistics updated as torch does; *n < 2 ORs
// `status_bit` into *status and leaves the running statistics alone.  Column sums run over bnm_chunks(cap) fixed row chunks
// (sparse_conv_plan.hpp), the chunks added in order.  `part` holds bnm_part_floats(cap, C) floats.
inline size_t bnm_part_floats(long long cap, int C) { return (size_t)bnm_chunks(cap) * C * 2; }
hipError_t launch_bnm_forward(const float* x, const float* residual, const float* gamma, const float* beta, const int* n,
                              long long cap, int C, float eps, float momentum, int relu, float* y, float* mean, float* rstd,
                              float* running_mean, float* running_var, float* part, int* status, int status_bit, hipStream_t s);
// Backward: g = dy where the row is valid (and y_relu > 0 when the forward applied the ReLU), else 0 (all cap rows: the residual
// branch's gradient); dbeta = sum g, dgamma = sum g xhat; dx = gamma rstd (g - dbeta / n - xhat dgamma / n), 0 beyond *n.
hipError_t launch_bnm_backward(const float* dy, const float* x, const float* y_relu, const float* mean, const float* rstd,
                               const float* gamma, const int* n, long long cap, int C, float* g, float* dx, float* dgamma,
                               float* dbeta, float* part, hipStream_t s);

}  // namespace gmf
