// Internal C++ launch entry points of the sparse network's training kernels (sparse_train_kernels.hip).
// Public C ABI: include/gmf_hip.h (gmf_sparse_conv_wgrad, gmf_batchnorm_masked_forward, gmf_batchnorm_masked_backward).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace gmf {

// Weight gradient of one sparse convolution: dW[d] = sum over the pairs (d, i -> o) of map (row_ptr, pairs, by_off, off_start)
// of [xa | xb][i]^T dy[o], dW [K, ca + cb, cout].  row_ptr == nullptr: the identity map (K = 1, pair j = row j).
// k_wgrad_plan cuts every offset's pair list (by_off[off_start[d] ..]) into chunks of P pairs, P = max(kWgradMinChunk,
// ceil(nnz / (nslots - K))) with nnz the map's pair count, so the chunks fit the nslots slots; chunk_info[d] (d = 0..K) is the
// first slot of offset d.  k_sparse_wgrad gives each slot its own workgroups (64 x 64 tiles of dW[d]) and writes the chunk's
// sum into partial[slot]; k_wgrad_reduce adds an offset's chunks in chunk order (zero for an offset without pairs).  Every
// element's order depends only on the map and nslots (a function of K): bitwise repeatable, no float atomics.
constexpr int kWgradMinChunk = 64;
inline int sparse_wgrad_slots(int K) { return K + (K > 256 ? K : 256); }
struct SparseWgradArgs {
  const int* row_ptr; const int2* pairs; const int* by_off; const int* off_start; int K;
  const int* n_out;
  const float* xa; int ca; const float* xb; int cb;
  const float* dy; int cout;
  int nslots; int* chunk_info; float* partial;
  float* dW;
};
hipError_t launch_sparse_wgrad(const SparseWgradArgs& a, hipStream_t s);

// BatchNorm1d in training mode over the first *n rows of x [cap, C] (the valid rows of a sparse level).  Forward: y =
// relu?(gamma (x - mean) rstd + beta + residual?) for rows < *n, 0 beyond; running statistics updated as torch does; *n < 2 ORs
// `status_bit` into *status and leaves the running statistics alone.  Column sums run over kBnmChunks(cap) fixed row chunks, the
// chunks added in order.  `part` holds bnm_part_floats(cap, C) floats.
int bnm_chunks(long long cap);
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
