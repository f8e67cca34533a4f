// The spectral-matching baseline SM(...) of the reference's evaluation (GMF_PointDSC/baseline_scripts/baseline_3DMatch.py:19-53;
// called with top_ratio = 0.05 at baseline_KITTI.py:51), batched over ragged pairs and matrix-free:
//   d_ij = |c_i[0:3] - c_j[0:3]| - |c_i[3:6] - c_j[3:6]|,  m_ij = max(0, 4.5 - d_ij^2 / (2 sigma^2)),  m_ii = 0,  sigma = tau / 3
//   v = 1;  `iterations` times  v <- M v,  v <- v / (|v| + 1e-6)
//   labels = the topk rows of largest v (ties to the smaller row);  T = rigid_transform_3d(src, tgt, v * labels)
// M [N,N] is never formed: every product M v recomputes its entries (a dozen flops on seven floats per column).
//
//   k_sm_sweep      rows on lanes; the columns of the workgroup's split stream through LDS in tiles of kSmTile
//                   (6 coordinates + v_j, read by every lane at the same address: broadcast); partial sums to [split][row]
//   k_sm_normalise  per pair: u_i = the partial sums added in split order, |u|^2 in a fixed tree, v = u / (|u| + 1e-6)
//   k_sm_rank       rank_i = #{j : v_j > v_i or (v_j == v_i and j < i)} by the same streaming; label_i = rank_i < topk
//   k_sm_pose       per pair: the weighted moments in fp64 in a fixed tree, kabsch.hpp's rotation, T [4,4]
// No floating-point atomics; the split of a pair's columns depends on its own N alone (launchers_spectral.hpp), so a pair has the
// same bits alone, in any batch and on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kabsch.hpp"
#include "launchers_spectral.hpp"

namespace gmf {

namespace {

// ---------------------------------------------------------------------------------------
// One column tile against the lane's row.  DIAG: the tile holds the row's own column (row and column tiles are aligned), whose
// raw entry 4.5 is zeroed.  The square roots are v_sqrt_f32 as it comes (1 ulp): DESIGN.md section 4k.
// ---------------------------------------------------------------------------------------
GMF_DEVINL float sm_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

template <bool DIAG>
GMF_DEVINL float sm_tile(const float4* __restrict__ sa, const float4* __restrict__ sb, const float (&c)[6], int self, float inv2s2,
                         float acc) {
#pragma unroll 8
  for (int j = 0; j < kSmTile; ++j) {
    const float4 a = sa[j], b = sb[j];      // (x, y, z, x'), (y', z', v_j, -)
    const float dx = c[0] - a.x, dy = c[1] - a.y, dz = c[2] - a.z;
    const float ex = c[3] - a.w, ey = c[4] - b.x, ez = c[5] - b.y;
    const float d = sm_sqrt(dx * dx + dy * dy + dz * dz) - sm_sqrt(ex * ex + ey * ey + ez * ez);
    float m = fmaxf(0.f, 4.5f - d * d * inv2s2);
    if (DIAG) m = (j == self) ? 0.f : m;
    acc += m * b.z;
  }
  return acc;
}

}  // namespace

// grid (row tiles of the largest pair, splits of the largest pair, B), block kSmTile.  v == nullptr: v = ones (the first sweep).
__global__ void __launch_bounds__(kSmTile)
k_sm_sweep(const float* __restrict__ corr, const float* __restrict__ v, const int* __restrict__ offsets,
           float* __restrict__ partial, long long total_rows, int max_n, int forced, float inv2s2) {
  __shared__ float4 sa[kSmTile], sb[kSmTile];
  const int pair = blockIdx.z, tid = threadIdx.x;
  const int r0 = offsets[pair], n = offsets[pair + 1] - r0;
  const int rt = blockIdx.x;
  // n > max_n, or rows past B max_n: the caller's bound was wrong, and `partial` is sized by it (k_sm_pose writes such a pair's outputs)
  if (rt * kSmTile >= n || n > max_n || offsets[pair + 1] > total_rows) return;
  const SmSplit plan = sm_split_plan(n, forced);
  if ((int)blockIdx.y >= plan.eff) return;
  const int tiles = (n + kSmTile - 1) / kSmTile;
  const int ct0 = blockIdx.y * plan.chunk, ct1 = min(tiles, ct0 + plan.chunk);
  const int row = rt * kSmTile + tid;
  float c[6];
  {
    const float* p = corr + (size_t)(r0 + min(row, n - 1)) * 6;
#pragma unroll
    for (int e = 0; e < 6; ++e) c[e] = p[e];
  }
  // the next tile's column of this thread waits in registers while the current tile is swept
  float nx[7];
  auto fetch = [&](int ct) {
    const int j = ct * kSmTile + tid;
    if (j < n) {
      const float* p = corr + (size_t)(r0 + j) * 6;
#pragma unroll
      for (int e = 0; e < 6; ++e) nx[e] = p[e];
      nx[6] = v ? v[r0 + j] : 1.f;
    } else {                       // past the pair's end: a finite entry times v_j = 0
#pragma unroll
      for (int e = 0; e < 7; ++e) nx[e] = 0.f;
    }
  };
  fetch(ct0);
  float acc = 0.f;
  for (int ct = ct0; ct < ct1; ++ct) {
    __syncthreads();               // the previous tile has been read by every wave
    sa[tid] = make_float4(nx[0], nx[1], nx[2], nx[3]);
    sb[tid] = make_float4(nx[4], nx[5], nx[6], 0.f);
    __syncthreads();
    if (ct + 1 < ct1) fetch(ct + 1);
    acc = (ct == rt) ? sm_tile<true>(sa, sb, c, tid, inv2s2, acc) : sm_tile<false>(sa, sb, c, tid, inv2s2, acc);
  }
  if (row < n) partial[(size_t)blockIdx.y * total_rows + r0 + row] = acc;
}

// grid (B), block 1024.  Adds the partial sums of every row in split order, takes |u| over the pair in a fixed order (per thread
// over its rows, butterfly over the wave, the 16 waves in turn) and writes v = u / (|u| + 1e-6).
__global__ void __launch_bounds__(1024)
k_sm_normalise(const float* __restrict__ partial, const int* __restrict__ offsets, float* __restrict__ eig, long long total_rows,
               int max_n, int forced) {
  __shared__ double sh[16];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int r0 = offsets[pair], n = offsets[pair + 1] - r0;
  if (n <= 0 || n > max_n || offsets[pair + 1] > total_rows) return;
  const int eff = sm_split_plan(n, forced).eff;
  double ss = 0.0;
  for (int i = tid; i < n; i += 1024) {
    float u = partial[r0 + i];
    for (int s = 1; s < eff; ++s) u += partial[(size_t)s * total_rows + r0 + i];
    eig[r0 + i] = u;
    ss += (double)u * (double)u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if ((tid & 63) == 0) sh[tid >> 6] = ss;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int w = 0; w < 16; ++w) tot += sh[w];
  const float den = (float)sqrt(tot) + 1e-6f;
  for (int i = tid; i < n; i += 1024) eig[r0 + i] = eig[r0 + i] / den;      // (the thread's own stores)
}

// An unsigned key with the order of (v, then the smaller row first): larger key = earlier in the descending order.
GMF_DEVINL unsigned long long sm_key(float v, int j) {
  const unsigned u = __float_as_uint(v);
  const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)ord << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)j);
}

// grid (64-row tiles of the largest pair, B), block 256: lane = row, the four waves take a quarter of every 1024-column tile each.
__global__ void __launch_bounds__(256)
k_sm_rank(const float* __restrict__ eig, const int* __restrict__ offsets, const int* __restrict__ topk, float* __restrict__ labels,
          long long total_rows, int max_n) {
  __shared__ unsigned long long sk[1024];
  __shared__ int cnt[4][64];
  const int pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int r0 = offsets[pair], n = offsets[pair + 1] - r0;
  if ((int)blockIdx.x * 64 >= n || n > max_n || offsets[pair + 1] > total_rows) return;
  const int row = blockIdx.x * 64 + lane;
  const unsigned long long mine = sm_key(eig[r0 + min(row, n - 1)], min(row, n - 1));
  int rank = 0;
  for (int c0 = 0; c0 < n; c0 += 1024) {
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int j = c0 + m * 256 + tid;
      sk[m * 256 + tid] = j < n ? sm_key(eig[r0 + j], j) : 0ull;      // 0: below every real key
    }
    __syncthreads();
    const unsigned long long* mykeys = sk + q * 256;
#pragma unroll 8
    for (int j = 0; j < 256; ++j) rank += mykeys[j] > mine ? 1 : 0;
  }
  cnt[q][lane] = rank;
  __syncthreads();
  if (q == 0 && row < n) {
    const int r = cnt[0][lane] + cnt[1][lane] + cnt[2][lane] + cnt[3][lane];
    labels[r0 + row] = r < topk[pair] ? 1.f : 0.f;
  }
}

// grid (B), block 256.  rigid_transform_3d (GMF_PointDSC/models/common.py:10-50) with w = v * labels, not normalised: the raw
// moments sum w, sum w a, sum w b, sum w a b^T in fp64 (fixed order: per thread over its rows, butterfly, the 4 waves in turn),
// the centroids over sum w + 1e-6, H about them, R = V diag(1, 1, det) U^T, t = cb - R ca.  H == 0 (no labels, or an empty
// pair): the identity, as the reference's SVD of a zero matrix gives.  A pair beyond the caller's max_n gets the identity and zeros.
__global__ void __launch_bounds__(256)
k_sm_pose(const float* __restrict__ src, const float* __restrict__ tgt, float* __restrict__ eig, float* __restrict__ labels,
          const int* __restrict__ offsets, float* __restrict__ T_out, long long total_rows, int max_n) {
  __shared__ double sh[16][4];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int r0 = offsets[pair], n = offsets[pair + 1] - r0;
  if (n > max_n || offsets[pair + 1] > total_rows) {      // the caller's bound did not hold: the pair was not computed
    for (int i = tid; i < n; i += 256) { eig[r0 + i] = 0.f; labels[r0 + i] = 0.f; }
    if (tid < 16) T_out[(size_t)pair * 16 + tid] = (tid % 5 == 0) ? 1.f : 0.f;
    return;
  }
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double w = (double)(eig[r0 + i] * labels[r0 + i]);
    if (w == 0.0) continue;
    const float* ap = src + (size_t)(r0 + i) * 3;
    const float* bp = tgt + (size_t)(r0 + i) * 3;
    const double a[3] = {ap[0], ap[1], ap[2]}, b[3] = {bp[0], bp[1], bp[2]};
    acc[0] += w;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      acc[1 + r] += w * a[r];
      acc[4 + r] += w * b[r];
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) acc[7 + 3 * r + cc] += w * a[r] * b[cc];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < 16; ++k) sh[k][tid >> 6] = acc[k];
  __syncthreads();
  if (tid != 0) return;
  double m[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) m[k] = ((sh[k][0] + sh[k][1]) + sh[k][2]) + sh[k][3];
  const double den = m[0] + 1e-6;
  const double ca[3] = {m[1] / den, m[2] / den, m[3] / den};
  const double cb[3] = {m[4] / den, m[5] / den, m[6] / den};
  double H[9], R[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc)
      H[3 * r + cc] = m[7 + 3 * r + cc] - ca[r] * m[4 + cc] - m[1 + r] * cb[cc] + m[0] * ca[r] * cb[cc];
  kabsch_rotation_from_H(H, R);
  float* T = T_out + (size_t)pair * 16;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double t = cb[r] - (R[3 * r] * ca[0] + R[3 * r + 1] * ca[1] + R[3 * r + 2] * ca[2]);
    T[4 * r + 0] = (float)R[3 * r]; T[4 * r + 1] = (float)R[3 * r + 1]; T[4 * r + 2] = (float)R[3 * r + 2];
    T[4 * r + 3] = (float)t;
  }
  T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

hipError_t launch_sm_pose(const float* src, const float* tgt, float* eig, float* labels, const int* offsets, int B,
                          long long total_rows, int max_n, float* T_out, hipStream_t s) {
  hipLaunchKernelGGL(k_sm_pose, dim3(B), dim3(256), 0, s, src, tgt, eig, labels, offsets, T_out, total_rows, max_n);
  return hipGetLastError();
}

hipError_t launch_spectral_matching(const float* corr, const float* src, const float* tgt, const int* offsets, int B,
                                    long long total_rows, int max_n, float inlier_threshold, const int* topk, int iterations,
                                    int forced_splits, float* partial, float* eig, float* labels, float* T_out,
                                    hipStream_t s) {
  if (max_n > 0 && total_rows > 0) {
    const double sigma = (double)inlier_threshold / 3.0;
    const float inv2s2 = (float)(1.0 / (2.0 * sigma * sigma));
    const dim3 sweep_grid((max_n + kSmTile - 1) / kSmTile, sm_max_splits(max_n, forced_splits), B);
    for (int it = 0; it < iterations; ++it) {
      const float* v = it ? eig : nullptr;
      hipLaunchKernelGGL(k_sm_sweep, sweep_grid, dim3(kSmTile), 0, s, corr, v, offsets, partial, total_rows, max_n, forced_splits,
                         inv2s2);
      hipLaunchKernelGGL(k_sm_normalise, dim3(B), dim3(1024), 0, s, partial, offsets, eig, total_rows, max_n, forced_splits);
    }
    hipLaunchKernelGGL(k_sm_rank, dim3((max_n + 63) / 64, B), dim3(256), 0, s, eig, offsets, topk, labels, total_rows, max_n);
  }
  return launch_sm_pose(src, tgt, eig, labels, offsets, B, total_rows, max_n, T_out, s);
}

}  // namespace gmf
