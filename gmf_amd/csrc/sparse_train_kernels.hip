// Training kernels of the sparse inlier network (DGR's ResUNetBN2C; the forward is sparse_kernels.hip).  Contract:
// launchers_sparse_train.hpp, include/gmf_hip.h.
//
// Weight gradient (k_wgrad_plan, k_sparse_wgrad, k_wgrad_reduce): dW[d] = sum over the pairs of offset d of x[i]^T dy[o].  The
// offset-major lists of the plan give each offset's pairs in ascending output row; k_wgrad_plan cuts every list into chunks of
// P pairs (P from the map's pair count and the slot count, so one long offset - the centre one, a pair per row - spreads over
// many workgroups instead of setting the critical path).  A workgroup owns (chunk slot, 64 input channels, 64 output channels):
// it walks its chunk 64 pairs at a time, recovers each pair's output row by binary search in row_ptr (as k_sparse_conv does),
// gathers the 64 input rows and the 64 gradient rows into LDS and accumulates the 64 x 64 product.  Order of every element:
// 16-pair fma chains added in pair order inside a chunk, then k_wgrad_reduce adds the chunks of an offset in chunk order.  No
// float atomics: two calls give bitwise-equal dW.
// BatchNorm over a level's valid rows (k_bnm_*): column sums over fixed row chunks of the cap row slots (4 row lanes per
// column, added in lane order, chunks added in chunk order), two passes for the variance (sum, then centred squares).
#include <hip/hip_runtime.h>

#include "launchers_sparse.hpp"
#include "launchers_sparse_train.hpp"

#define GMF_DEVINL __device__ __forceinline__

namespace gmf {

namespace {

constexpr int kThreads = 256;
constexpr int kWP = 64;              // pairs per LDS tile
constexpr int kWT = 64;              // dW tile: 64 input x 64 output channels
constexpr int kChain = 16;           // pairs per fma chain

int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

// chunk_info[d] = first slot of offset d (d = 0..K), chunk_info[K + 1] = P
__global__ __launch_bounds__(1024) void k_wgrad_plan(const SparseWgradArgs a) {
  __shared__ int cnt[kSparseMaxK];
  __shared__ int s_P;
  const int n = *a.n_out;
  const bool ident = a.row_ptr == nullptr;
  if (threadIdx.x == 0) {
    const long long nnz = ident ? n : a.row_ptr[n];
    const long long extra = a.nslots - a.K;
    long long P = (nnz + extra - 1) / extra;       // sum over d of ceil(n_d / P) <= nnz / P + K <= nslots
    s_P = (int)(P < kWgradMinChunk ? kWgradMinChunk : P);
  }
  __syncthreads();
  const int P = s_P;
  for (int d = threadIdx.x; d < a.K; d += blockDim.x) {
    const int nd = ident ? n : a.off_start[d + 1] - a.off_start[d];
    cnt[d] = (nd + P - 1) / P;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int d = 0; d < a.K; ++d) {
      a.chunk_info[d] = s;
      s += cnt[d];
    }
    a.chunk_info[a.K] = s;
    a.chunk_info[a.K + 1] = P;
  }
}

__global__ __launch_bounds__(kThreads) void k_sparse_wgrad(const SparseWgradArgs a) {
  __shared__ __align__(16) float Xs[kWP][kWT];     // [pair][input channel]
  __shared__ __align__(16) float Gs[kWP][kWT];     // [pair][output channel]
  __shared__ int s_o[kWP], s_i[kWP];
  const int* cs = a.chunk_info;
  const int slot = blockIdx.x;
  if (slot >= cs[a.K]) return;
  int l = 0, h = a.K - 1;                          // the offset of this slot: the last d with cs[d] <= slot
  while (l < h) {
    const int mid = (l + h + 1) >> 1;
    if (cs[mid] <= slot) l = mid; else h = mid - 1;
  }
  const int d = l, P = cs[a.K + 1];
  const int n = *a.n_out;
  const bool ident = a.row_ptr == nullptr;
  const int lo = (ident ? 0 : a.off_start[d]) + (slot - cs[d]) * P;
  const int end = ident ? n : a.off_start[d + 1];
  const int hi = lo + P < end ? lo + P : end;
  const int cin = a.ca + a.cb;
  const int ci0 = blockIdx.y * kWT, co0 = blockIdx.z * kWT;
  const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  for (int t0 = lo; t0 < hi; t0 += kWP) {
    __syncthreads();                               // the previous tile is done with Xs, Gs and s_*
    if (tid < kWP) {
      const int j = t0 + tid;
      int o = -1, i = -1;
      if (j < hi) {
        if (ident) {
          o = i = j;
        } else {
          const int p = a.by_off[j];
          int rl = 0, rh = n - 1;                  // the row of pair p: the last o with row_ptr[o] <= p
          while (rl < rh) {
            const int mid = (rl + rh + 1) >> 1;
            if (a.row_ptr[mid] <= p) rl = mid; else rh = mid - 1;
          }
          o = rl;
          i = a.pairs[p].y;
        }
      }
      s_o[tid] = o;
      s_i[tid] = i;
    }
    __syncthreads();
    for (int e = tid; e < kWP * kWT; e += kThreads) {
      const int pp = e / kWT, cc = e % kWT, c = ci0 + cc, oc = co0 + cc, ir = s_i[pp], orow = s_o[pp];
      float xv = 0.f, gv = 0.f;
      if (ir >= 0 && c < cin) xv = c < a.ca ? a.xa[(size_t)ir * a.ca + c] : a.xb[(size_t)ir * a.cb + (c - a.ca)];
      if (orow >= 0 && oc < a.cout) gv = a.dy[(size_t)orow * a.cout + oc];
      Xs[pp][cc] = xv;
      Gs[pp][cc] = gv;
    }
    __syncthreads();
    for (int k0 = 0; k0 < kWP; k0 += kChain) {
      float sk[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) sk[r][c] = 0.f;
#pragma unroll
      for (int kk = 0; kk < kChain; ++kk) {
        const float4 xv = *reinterpret_cast<const float4*>(&Xs[k0 + kk][tr * 4]);
        const float4 gv = *reinterpret_cast<const float4*>(&Gs[k0 + kk][tc * 4]);
        const float x4[4] = {xv.x, xv.y, xv.z, xv.w}, g4[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) sk[r][c] = fmaf(x4[r], g4[c], sk[r][c]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] += sk[r][c];
    }
  }
  float* part = a.partial + (size_t)slot * cin * a.cout;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ci = ci0 + tr * 4 + r;
    if (ci >= cin) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int oc = co0 + tc * 4 + c;
      if (oc < a.cout) part[(size_t)ci * a.cout + oc] = acc[r][c];
    }
  }
}

// dW[d] = the chunks of offset d added in chunk order (0 when the offset has no pairs)
__global__ __launch_bounds__(kThreads) void k_wgrad_reduce(const SparseWgradArgs a) {
  const long long per = (long long)(a.ca + a.cb) * a.cout;
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= a.K * per) return;
  const int d = (int)(e / per);
  const long long rem = e % per;
  float v = 0.f;
  for (int s = a.chunk_info[d], s1 = a.chunk_info[d + 1]; s < s1; ++s) v += a.partial[(size_t)s * per + rem];
  a.dW[e] = v;
}

// ---- BatchNorm over the valid rows of a level ----------------------------------------------------------------------------

// kMode 0: sum x; 1: sum (x - mean)^2; 2: [sum g | sum g (x - mean) rstd].  part [chunk][2C].
template <int kMode>
__global__ __launch_bounds__(kThreads) void k_bnm_colsum(const float* __restrict__ x, const float* __restrict__ g,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const int* __restrict__ n_ptr, long long cap, int C, int nch,
                                                         float* __restrict__ part) {
  __shared__ float s[2][4][64];
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane, ch = blockIdx.y;
  long long n = *n_ptr;
  if (n > cap) n = cap;
  const long long r0 = cap * ch / nch;
  long long r1 = cap * (ch + 1) / nch;
  if (r1 > n) r1 = n;
  float a0 = 0.f, a1 = 0.f;
  if (c < C) {
    const float m = mean ? mean[c] : 0.f, rs = rstd ? rstd[c] : 1.f;
    for (long long r = r0 + rl; r < r1; r += 4) {
      const float v = x[r * C + c];
      if (kMode == 0) {
        a0 += v;
      } else if (kMode == 1) {
        const float t = v - m;
        a0 = fmaf(t, t, a0);
      } else {
        const float gv = g[r * C + c];
        a0 += gv;
        a1 = fmaf(gv, (v - m) * rs, a1);
      }
    }
  }
  s[0][rl][lane] = a0;
  s[1][rl][lane] = a1;
  __syncthreads();
  if (rl == 0 && c < C) {
    float* p = part + (size_t)ch * 2 * C;
    p[c] = ((s[0][0][lane] + s[0][1][lane]) + s[0][2][lane]) + s[0][3][lane];
    if (kMode == 2) p[C + c] = ((s[1][0][lane] + s[1][1][lane]) + s[1][2][lane]) + s[1][3][lane];
  }
}

// kind 0: mean; 1: rstd and the running statistics (status bit when fewer than 2 rows); 2: dbeta (= o0), dgamma (= o1)
__global__ __launch_bounds__(kThreads) void k_bnm_finish(int kind, const float* __restrict__ part, int nch,
                                                         const int* __restrict__ n_ptr, long long cap, int C, float eps,
                                                         float momentum, float* mean, float* rstd, float* running_mean,
                                                         float* running_var, float* o0, float* o1, int* status, int bit) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  long long n = *n_ptr;
  if (n > cap) n = cap;
  float s0 = 0.f, s1 = 0.f;
  for (int ch = 0; ch < nch; ++ch) {
    s0 += part[(size_t)ch * 2 * C + c];
    if (kind == 2) s1 += part[(size_t)ch * 2 * C + C + c];
  }
  if (kind == 0) {
    mean[c] = n > 0 ? s0 / (float)n : 0.f;
  } else if (kind == 1) {
    if (n < 2) {                                   // torch: "Expected more than 1 value per channel when training"
      if (c == 0 && status) atomicOr(status, bit);
      rstd[c] = 0.f;
      return;
    }
    const float var = s0 / (float)n;
    rstd[c] = 1.f / sqrtf(var + eps);
    if (running_mean) {
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean[c];
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * (var * ((float)n / (float)(n - 1)));
    }
  } else {
    o0[c] = s0;
    o1[c] = s1;
  }
}

__global__ __launch_bounds__(kThreads) void k_bnm_apply(const float* __restrict__ x, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ residual,
                                                        int relu, const int* __restrict__ n_ptr, long long cap, int C,
                                                        float* __restrict__ y) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= cap * C) return;
  const long long r = e / C;
  const int c = (int)(e % C);
  float v = 0.f;
  if (r < *n_ptr) {
    v = fmaf((x[e] - mean[c]) * rstd[c], gamma[c], beta[c]);
    if (residual) v += residual[e];
    if (relu) v = fmaxf(v, 0.f);
  }
  y[e] = v;
}

__global__ __launch_bounds__(kThreads) void k_bnm_mask(const float* __restrict__ dy, const float* __restrict__ y_relu,
                                                       const int* __restrict__ n_ptr, long long cap, int C,
                                                       float* __restrict__ g) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= cap * C) return;
  const bool keep = e / C < *n_ptr && (!y_relu || y_relu[e] > 0.f);
  g[e] = keep ? dy[e] : 0.f;
}

__global__ __launch_bounds__(kThreads) void k_bnm_dx(const float* __restrict__ g, const float* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                     const float* __restrict__ dbeta, const int* __restrict__ n_ptr,
                                                     long long cap, int C, float* __restrict__ dx) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= cap * C) return;
  const long long r = e / C, n = *n_ptr;
  const int c = (int)(e % C);
  float v = 0.f;
  if (r < n && n > 0) {
    const float inv_n = 1.f / (float)n;
    const float xhat = (x[e] - mean[c]) * rstd[c];
    v = gamma[c] * rstd[c] * (g[e] - dbeta[c] * inv_n - xhat * dgamma[c] * inv_n);
  }
  dx[e] = v;
}

}  // namespace

hipError_t launch_sparse_wgrad(const SparseWgradArgs& a, hipStream_t s) {
  const int cin = a.ca + a.cb;
  k_wgrad_plan<<<1, 1024, 0, s>>>(a);
  k_sparse_wgrad<<<dim3(a.nslots, blocks(cin, kWT), blocks(a.cout, kWT)), kThreads, 0, s>>>(a);
  k_wgrad_reduce<<<blocks((long long)a.K * cin * a.cout, kThreads), kThreads, 0, s>>>(a);
  return hipGetLastError();
}

int bnm_chunks(long long cap) {
  const long long c = (cap + 255) / 256;
  return (int)(c > 64 ? 64 : c);
}

hipError_t launch_bnm_forward(const float* x, const float* residual, const float* gamma, const float* beta, const int* n,
                              long long cap, int C, float eps, float momentum, int relu, float* y, float* mean, float* rstd,
                              float* running_mean, float* running_var, float* part, int* status, int status_bit, hipStream_t s) {
  const int nch = bnm_chunks(cap);
  const dim3 grid(blocks(C, 64), nch);
  k_bnm_colsum<0><<<grid, kThreads, 0, s>>>(x, nullptr, nullptr, nullptr, n, cap, C, nch, part);
  k_bnm_finish<<<blocks(C, kThreads), kThreads, 0, s>>>(0, part, nch, n, cap, C, eps, momentum, mean, rstd, nullptr, nullptr,
                                                        nullptr, nullptr, nullptr, 0);
  k_bnm_colsum<1><<<grid, kThreads, 0, s>>>(x, nullptr, mean, nullptr, n, cap, C, nch, part);
  k_bnm_finish<<<blocks(C, kThreads), kThreads, 0, s>>>(1, part, nch, n, cap, C, eps, momentum, mean, rstd, running_mean,
                                                        running_var, nullptr, nullptr, status, status_bit);
  k_bnm_apply<<<blocks(cap * C, kThreads), kThreads, 0, s>>>(x, mean, rstd, gamma, beta, residual, relu, n, cap, C, y);
  return hipGetLastError();
}

hipError_t launch_bnm_backward(const float* dy, const float* x, const float* y_relu, const float* mean, const float* rstd,
                               const float* gamma, const int* n, long long cap, int C, float* g, float* dx, float* dgamma,
                               float* dbeta, float* part, hipStream_t s) {
  const int nch = bnm_chunks(cap);
  k_bnm_mask<<<blocks(cap * C, kThreads), kThreads, 0, s>>>(dy, y_relu, n, cap, C, g);
  k_bnm_colsum<2><<<dim3(blocks(C, 64), nch), kThreads, 0, s>>>(x, g, mean, rstd, n, cap, C, nch, part);
  k_bnm_finish<<<blocks(C, kThreads), kThreads, 0, s>>>(2, part, nch, n, cap, C, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr,
                                                        dbeta, dgamma, nullptr, 0);
  k_bnm_dx<<<blocks(cap * C, kThreads), kThreads, 0, s>>>(g, x, mean, rstd, gamma, dgamma, dbeta, n, cap, C, dx);
  return hipGetLastError();
}

}  // namespace gmf
