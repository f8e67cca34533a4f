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
// FCGF's training ends (launchers_sparse_train.hpp has each one's order): k_sparse_wgrad_narrow, the weight gradient of a
// narrow-input convolution (conv1: Cin <= 8), one wave per chunk with lane = output channel; k_rownorm_eps, y = x / (||x|| +
// 1e-8) and its backward; k_hcl_*, the hardest-contrastive loss (mining, reduction, per-term gradient rows) and
// k_rows_sum_by_dest, which adds gradient rows per destination row in the order of a CSR.
// BatchNorm over a level's valid rows (k_bnm_*): column sums over fixed row chunks of the cap row slots (4 row lanes per
// column, added in lane order, chunks added in chunk order), two passes for the variance (sum, then centred squares).
#include <hip/hip_runtime.h>

#include "launchers_sparse.hpp"
#include "launchers_sparse_train.hpp"

#define GMF_DEVINL __device__ __forceinline__

namespace gmf {

namespace {

constexpr int kThreads = kSparseWgThreads;
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
    s_P = sparse_wgrad_chunk(nnz, a.K, a.nslots);  // sparse_conv_plan.hpp: the chunks fit the nslots slots
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

// ---- narrow-input weight gradient (FCGF's conv1) -------------------------------------------------------------------------

// One wave per chunk slot; see launchers_sparse_train.hpp.  Lane l resolves pair t0 + l of the chunk, then the wave walks the tile:
// lane = (group g, output channel c), group g takes the tile's pairs g, g + G, ..
__global__ __launch_bounds__(64) void k_sparse_wgrad_narrow(const SparseWgradArgs a) {
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
  const int lo = a.off_start[d] + (slot - cs[d]) * P;
  const int end = a.off_start[d + 1];
  const int hi = lo + P < end ? lo + P : end;
  const int cin = a.ca, cout = a.cout;
  const int L = sparse_narrow_lanes(cout);
  const int G = 64 / L;
  const int lane = threadIdx.x, c = lane % L, g = lane / L;
  const int cc = c < cout ? c : cout - 1;          // lanes past cout compute a copy of the last channel and store nothing
  float acc[kWgradNarrowMaxCin];
#pragma unroll
  for (int k = 0; k < kWgradNarrowMaxCin; ++k) acc[k] = 0.f;
  for (int t0 = lo; t0 < hi; t0 += 64) {
    const int j = t0 + lane;
    int o = -1;
    float xv[kWgradNarrowMaxCin];
#pragma unroll
    for (int k = 0; k < kWgradNarrowMaxCin; ++k) xv[k] = 0.f;
    if (j < hi) {
      const int p = a.by_off[j];
      int rl = 0, rh = n - 1;                      // the row of pair p: the last o with row_ptr[o] <= p
      while (rl < rh) {
        const int mid = (rl + rh + 1) >> 1;
        if (a.row_ptr[mid] <= p) rl = mid; else rh = mid - 1;
      }
      o = rl;
      const float* xr = a.xa + (size_t)a.pairs[p].y * cin;
#pragma unroll
      for (int k = 0; k < kWgradNarrowMaxCin; ++k)
        if (k < cin) xv[k] = xr[k];
    }
    const int jn = hi - t0 < 64 ? hi - t0 : 64;
    for (int jj = 0; jj < jn; jj += G) {           // uniform in the wave; a source lane past jn holds o = -1, x = 0
      const int src = jj + g;
      const int oj = __shfl(o, src);
      const float gv = oj >= 0 ? a.dy[(size_t)oj * cout + cc] : 0.f;
#pragma unroll
      for (int k = 0; k < kWgradNarrowMaxCin; ++k)
        if (k < cin) acc[k] = fmaf(__shfl(xv[k], src), gv, acc[k]);
    }
  }
  float* part = a.partial + (size_t)slot * cin * cout;
#pragma unroll
  for (int k = 0; k < kWgradNarrowMaxCin; ++k) {
    if (k >= cin) break;
    float v = __shfl(acc[k], c);
    for (int gg = 1; gg < G; ++gg) v += __shfl(acc[k], c + gg * L);
    if (g == 0 && c < cout) part[k * cout + c] = v;
  }
}

// ---- FCGF's row normalisation y = x / (||x|| + 1e-8) ---------------------------------------------------------------------

GMF_DEVINL float wave_sum(float v) {               // butterfly: every lane ends with the same bits
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

template <bool kBackward>
__global__ __launch_bounds__(kThreads) void k_rownorm_eps(const float* __restrict__ x, const float* __restrict__ dy,
                                                          float* __restrict__ nrm, float* __restrict__ out, long long rows,
                                                          int C) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                           // whole waves leave together
  const float* xr = x + r * C;
  float* orow = out + r * C;
  if (!kBackward) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(xr[c], xr[c], s);
    const float nr = sqrtf(wave_sum(s));
    if (lane == 0) nrm[r] = nr;
    const float inv = nr > 0.f ? 1.f / (nr + 1e-8f) : 0.f;
    for (int c = lane; c < C; c += 64) orow[c] = xr[c] * inv;
  } else {
    const float* gr = dy + r * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(xr[c], gr[c], s);
    const float dot = wave_sum(s);
    const float nr = nrm[r], sden = nr + 1e-8f;
    const float inv = nr > 0.f ? 1.f / sden : 0.f;
    const float k2 = nr > 0.f ? dot / (nr * sden * sden) : 0.f;
    for (int c = lane; c < C; c += 64) orow[c] = gr[c] * inv - xr[c] * k2;
  }
}

// ---- hardest-contrastive loss --------------------------------------------------------------------------------------------

// an index of the caller's, held inside [0, n): a bad one ORs the status bit and reads row 0
GMF_DEVINL long long hcl_index(long long v, long long n, int* status, int bit) {
  if (v >= 0 && v < n) return v;
  if (status) atomicOr(status, bit);
  return 0;
}

GMF_DEVINL bool hcl_is_positive(const long long* __restrict__ keys, long long K, long long key) {
  long long lo = 0, hi = K;                        // the first index with keys[index] >= key
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo < K && keys[lo] == key;
}

__global__ __launch_bounds__(kThreads) void k_hcl_mine(const HclArgs a) {
  __shared__ float s_a[64];
  __shared__ float s_best[kThreads];
  __shared__ int s_pos[kThreads];
  const int k = blockIdx.x, side = blockIdx.y, tid = threadIdx.x, C = a.C;
  const long long kk = a.pos_sel ? hcl_index(a.pos_sel[k], a.K, a.status, a.status_bit) : k;
  const long long i = hcl_index(a.pairs[2 * kk], a.N0, a.status, a.status_bit);
  const long long j = hcl_index(a.pairs[2 * kk + 1], a.N1, a.status, a.status_bit);
  const float* anchor = side == 0 ? a.F0 + i * C : a.F1 + j * C;
  const float* cand = side == 0 ? a.F1 : a.F0;
  const long long* sel = side == 0 ? a.sel1 : a.sel0;
  const int H = side == 0 ? a.H1 : a.H0;
  const long long ncand = side == 0 ? a.N1 : a.N0;
  if (tid < C) s_a[tid] = anchor[tid];
  __syncthreads();
  float best = INFINITY;
  int bpos = 0x7fffffff;
  for (int s = tid; s < H; s += kThreads) {
    const float* row = cand + hcl_index(sel[s], ncand, a.status, a.status_bit) * C;
    float d2 = 0.f;
    for (int c = 0; c < C; ++c) {
      const float t = s_a[c] - row[c];
      d2 = fmaf(t, t, d2);
    }
    if (d2 < best) {
      best = d2;
      bpos = s;
    }
  }
  s_best[tid] = best;
  s_pos[tid] = bpos;
  __syncthreads();
  for (int off = kThreads / 2; off >= 1; off >>= 1) {
    if (tid < off) {
      const float b2 = s_best[tid + off];
      const int p2 = s_pos[tid + off];
      if (b2 < s_best[tid] || (b2 == s_best[tid] && p2 < s_pos[tid])) {
        s_best[tid] = b2;
        s_pos[tid] = p2;
      }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const int pos = s_pos[0] < H ? s_pos[0] : 0;     // every score NaN: position 0 (the loss is NaN then, as it should be)
  const long long hrow = hcl_index(sel[pos], ncand, a.status, a.status_bit);
  const float D = sqrtf(s_best[0] + 1e-7f);
  const long long nmax = a.N0 > a.N1 ? a.N0 : a.N1;
  const long long key = side == 0 ? i + hrow * nmax : hrow + j * nmax;
  const bool keep = !hcl_is_positive(a.keys, a.K, key);
  const float r = fmaxf(a.neg_thresh - D, 0.f);
  (side == 0 ? a.h01 : a.h10)[k] = hrow;
  (side == 0 ? a.keep0 : a.keep1)[k] = keep ? 1 : 0;
  (side == 0 ? a.D01 : a.D10)[k] = D;
  a.terms[(size_t)(1 + side) * a.P + k] = keep ? r * r : 0.f;
  if (side == 0) {
    const float* b = a.F1 + j * C;
    float d2 = 0.f;
    for (int c = 0; c < C; ++c) {
      const float t = s_a[c] - b[c];
      d2 = fmaf(t, t, d2);
    }
    a.terms[k] = fmaxf(d2 - a.pos_thresh, 0.f);
  }
}

__global__ __launch_bounds__(kThreads) void k_hcl_reduce(const HclArgs a) {
  __shared__ float s[5][kThreads];
  const int tid = threadIdx.x, P = a.P;
  float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = tid; k < P; k += kThreads) {
    v[0] += a.terms[k];
    v[1] += a.terms[(size_t)P + k];
    v[2] += a.terms[(size_t)2 * P + k];
    v[3] += (float)a.keep0[k];
    v[4] += (float)a.keep1[k];
  }
  for (int q = 0; q < 5; ++q) s[q][tid] = v[q];
  __syncthreads();
  for (int off = kThreads / 2; off >= 1; off >>= 1) {
    if (tid < off)
      for (int q = 0; q < 5; ++q) s[q][tid] += s[q][tid + off];
    __syncthreads();
  }
  if (tid != 0) return;
  const float c0 = s[3][0], c1 = s[4][0];
  a.out[0] = s[0][0] / (float)P;
  a.out[1] = 0.5f * ((c0 > 0.f ? s[1][0] / c0 : 0.f) + (c1 > 0.f ? s[2][0] / c1 : 0.f));
  a.out[2] = c0;
  a.out[3] = c1;
}

GMF_DEVINL long long hcl_clamp(long long v, long long n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// one wave per k, lane = channel
__global__ __launch_bounds__(64) void k_hcl_backward_rows(const HclBwdArgs a) {
  const int k = blockIdx.x, c = threadIdx.x, C = a.C;
  const long long kk = a.pos_sel ? hcl_clamp(a.pos_sel[k], a.K) : k;
  const long long i = hcl_clamp(a.pairs[2 * kk], a.N0), j = hcl_clamp(a.pairs[2 * kk + 1], a.N1);
  const long long h01 = hcl_clamp(a.h01[k], a.N1), h10 = hcl_clamp(a.h10[k], a.N0);
  if (c == 0) {
    a.dest0[3 * (size_t)k] = i;
    a.dest0[3 * (size_t)k + 1] = i;
    a.dest0[3 * (size_t)k + 2] = h10;
    a.dest1[3 * (size_t)k] = j;
    a.dest1[3 * (size_t)k + 1] = j;
    a.dest1[3 * (size_t)k + 2] = h01;
  }
  if (c >= C) return;
  const float gp = *a.g_pos, gn = *a.g_neg;
  const float a0 = a.F0[i * C + c], b1 = a.F1[j * C + c];
  // relu(sum (a - b)^2 - pos_thresh) / P
  const float wp = a.terms[k] > 0.f ? gp * (2.f / (float)a.P) : 0.f;
  const float vp = wp * (a0 - b1);
  // 1/2 relu(neg_thresh - D)^2 / count, D = sqrt(sum (a - b)^2 + 1e-7): d/da = -relu(.) (a - b) / (D count)
  const float D0 = a.D01[k], D1 = a.D10[k], r0 = a.neg_thresh - D0, r1 = a.neg_thresh - D1;
  const float w0 = a.keep0[k] && r0 > 0.f ? -gn * r0 / (D0 * a.out[2]) : 0.f;
  const float w1 = a.keep1[k] && r1 > 0.f ? -gn * r1 / (D1 * a.out[3]) : 0.f;
  const float v0 = w0 * (a0 - a.F1[h01 * C + c]);
  const float v1 = w1 * (b1 - a.F0[h10 * C + c]);
  float* q0 = a.rows0 + 3 * (size_t)k * C + c;
  float* q1 = a.rows1 + 3 * (size_t)k * C + c;
  q0[0] = vp;
  q0[C] = v0;
  q0[2 * C] = -v1;
  q1[0] = -vp;
  q1[C] = v1;
  q1[2 * C] = -v0;
}

__global__ __launch_bounds__(kThreads) void k_rows_sum_by_dest(const float* __restrict__ rows, long long E,
                                                               const long long* __restrict__ order,
                                                               const long long* __restrict__ row_start, long long N, int C,
                                                               float* __restrict__ out) {
  const int c = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (r >= N || c >= C) return;
  long long e0 = row_start[r], e1 = row_start[r + 1];
  if (e0 < 0) e0 = 0;
  if (e1 > E) e1 = E;
  float acc = 0.f;
  for (long long e = e0; e < e1; ++e) acc += rows[hcl_clamp(order[e], E) * C + c];
  out[r * C + c] = acc;
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
  const long long r0 = bnm_chunk_begin(cap, ch, nch);
  long long r1 = bnm_chunk_begin(cap, ch + 1, nch);
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
    if (relu) v = v <= 0.f ? 0.f : v;              // keeps a NaN, as torch.relu does; fmaxf(v, 0) returns 0 for it (sparse_kernels.hip)
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

hipError_t launch_sparse_wgrad_narrow(const SparseWgradArgs& a, hipStream_t s) {
  k_wgrad_plan<<<1, 1024, 0, s>>>(a);
  k_sparse_wgrad_narrow<<<a.nslots, 64, 0, s>>>(a);
  k_wgrad_reduce<<<blocks((long long)a.K * a.ca * a.cout, kThreads), kThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_rownorm_eps(bool backward, const float* x, const float* dy, float* nrm, float* out, long long rows, int C,
                              hipStream_t s) {
  const int g = blocks(rows, kThreads / 64);
  if (backward)
    k_rownorm_eps<true><<<g, kThreads, 0, s>>>(x, dy, nrm, out, rows, C);
  else
    k_rownorm_eps<false><<<g, kThreads, 0, s>>>(x, dy, nrm, out, rows, C);
  return hipGetLastError();
}

hipError_t launch_hcl_forward(const HclArgs& a, hipStream_t s) {
  k_hcl_mine<<<dim3(a.P, 2), kThreads, 0, s>>>(a);
  k_hcl_reduce<<<1, kThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_hcl_backward(const HclBwdArgs& a, hipStream_t s) {
  k_hcl_backward_rows<<<a.P, 64, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_rows_sum_by_dest(const float* rows, long long E, const long long* order, const long long* row_start, long long N,
                                   int C, float* out, hipStream_t s) {
  k_rows_sum_by_dest<<<blocks(N, kThreads / 64), kThreads, 0, s>>>(rows, E, order, row_start, N, C, out);
  return hipGetLastError();
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
