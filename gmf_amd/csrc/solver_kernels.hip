// Correspondence RANSAC and point-to-point ICP, batched over ragged pairs: the solvers the reference's evaluation scripts run on
// the CPU through open3d after the network (GMF_PointDSC/evaluation/test_3DMatch.py:76-96, benchmark_utils.py:40-56;
// GMF_DeepGlobalRegistration/*/core/deep_global_registration.py:57-85, 256-272, 385-405).  Contract: gmf_amd/solvers.py.
//
// RANSAC, three launches after one memset:
//   k_ransac_compact   one workgroup per pair: the participating rows (mask) packed to the front of the pair's slot.
//   k_ransac_score     one lane per hypothesis: draw (ransac_sampler.hpp), fp64 Kabsch in registers, then the pair's rows
//                      stream through an LDS tile that every lane reads at the same address (a broadcast).  The rows of a pair
//                      are split over gridDim.y; the partial counts and d^2 sums are integers (d^2 in units of tau^2 / 2^24),
//                      so the atomics that combine them give the same bits in any order and for any split.
//   k_ransac_finish    one workgroup per pair: argmax over (valid, count, -sum, -h), a total order, then the winner's inlier
//                      mask, fitness and rmse (fp64 sums in a fixed tree).
// ICP, 2 + 2 (max_iteration + 1) launches, none of which the host waits for:
//   k_icp_init         T = init in fp64, done = 0.
//   k_icp_nn           exact nearest target of every transformed source row by direct fp32 differences; the targets are split
//                      over gridDim.y and folded with a 64-bit atomicMin of (d^2 bits | target row): smallest d^2, then row.
//   k_icp_nn_grid      the same search on a hashed grid of cell edge tau (1 + 2^-10) over the targets, built once per call
//                      (launch_grid_build: four more launches): 32 lanes per source row, one per cell of the 3 x 3 x 3 block
//                      around it.  The same d^2 expression and the same (d^2 bits | row) minimum, so every row whose nearest
//                      target lies within tau gets k_icp_nn's key and the whole result is bit-identical.
//   k_icp_step         one workgroup per pair: C, fitness, rmse, the convergence test, then Umeyama over C and T <- dT T.
//   A finished pair's workgroups return at once.
// Point-to-plane ICP: the same launches with k_icp_step replaced by two, 2 + 3 (max_iteration + 1) in all:
//   k_icp_plane_partials  one workgroup per 512 source rows of ONE pair: C, nn and a partial of 29 fp64 sums in a fixed tree.
//   k_icp_plane_solve     one wave per pair: the partials in ascending order, fitness, rmse, the convergence test, then the
//                         6 x 6 LDL^T of the linearised step and T <- dT T.
// Coloured ICP: point-to-plane ICP's launches with k_icp_color_partials in the place of k_icp_plane_partials:
//   k_icp_color_partials  the same 29 sums, A and b holding lambda times the geometric and (1 - lambda) times the photometric
//                         term of every row (the target's colour gradients: pointcloud_kernels.hip, k_color_gradient).
// Feature-matching RANSAC (open3d's registration_ransac_based_on_feature_matching), three memsets, the grid build and seven
// launches, none of which the host waits for:
//   k_fm_propose       one lane per hypothesis: draw, pair each row with its feature-space match, edge-length test, fp64 Kabsch,
//                      distance test on the fp32 pose.  A flag and the pose per hypothesis.
//   k_fm_select        one workgroup per pair: the first max_validation passing hypotheses in increasing h (a prefix sum).
//   k_fm_eval          one lane per (validated hypothesis, source row): the nearest target of the transformed row on the hashed
//                      grid (or through an LDS tile), |C| and the fixed-point sum of d^2 per hypothesis by integer atomics; run
//                      once more on the winner alone to leave its keys.
//   k_fm_winner        one workgroup per pair: argmax over (count, -sum, -h).
//   k_fm_finish        one workgroup per pair: nn, fitness, rmse (fp64 sums in a fixed tree), pose, hypothesis, sample.
#include <algorithm>
#include <math.h>

#include "grid_hash.hpp"
#include "kabsch.hpp"
#include "launchers_solvers.hpp"
#include "ransac_sampler.hpp"

namespace gmf {

constexpr int kThreads = 256;

// |R s + t - q|^2 in fp32 with every rounding pinned by explicit fmas (the scoring and the finishing kernels must agree bitwise)
GMF_DEVINL float resid2(const float* T, float sx, float sy, float sz, float qx, float qy, float qz) {
  const float dx = fmaf(T[0], sx, fmaf(T[1], sy, fmaf(T[2], sz, T[3]))) - qx;
  const float dy = fmaf(T[4], sx, fmaf(T[5], sy, fmaf(T[6], sz, T[7]))) - qy;
  const float dz = fmaf(T[8], sx, fmaf(T[9], sy, fmaf(T[10], sz, T[11]))) - qz;
  return fmaf(dx, dx, fmaf(dy, dy, dz * dz));
}

// fixed-shape tree sum over the workgroup: the same bits whatever the timing.  sh: kThreads * D doubles.  Result in sh[0 .. D).
template <int D>
GMF_DEVINL void tree_sum(double* v, double* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int d = 0; d < D; ++d) sh[d * kThreads + tid] = v[d];
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int d = 0; d < D; ++d) sh[d * kThreads + tid] += sh[d * kThreads + tid + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int d = 0; d < D; ++d) v[d] = sh[d * kThreads];
  __syncthreads();
}

// unweighted Umeyama / Kabsch without scaling of NS rows in fp64: [R | t] row-major 3 x 4.  false: the SVD failed (H == 0, NaN).
template <int NS>
GMF_DEVINL bool fit_sample(const float4* __restrict__ cs, const float4* __restrict__ cq, const int* rows, double* Tout) {
  double ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const float4 a = cs[rows[k]], b = cq[rows[k]];
    ca[0] += a.x; ca[1] += a.y; ca[2] += a.z;
    cb[0] += b.x; cb[1] += b.y; cb[2] += b.z;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { ca[c] /= NS; cb[c] /= NS; }
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const float4 a = cs[rows[k]], b = cq[rows[k]];
    const double am[3] = {a.x - ca[0], a.y - ca[1], a.z - ca[2]};
    const double bm[3] = {b.x - cb[0], b.y - cb[1], b.z - cb[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) H[3 * r + c] = fma(am[r], bm[c], H[3 * r + c]);
  }
  KabschFrames f;
  kabsch_frames(H, f);
  if (!f.ok) return false;
  bool fin = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double t = cb[r];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double R = f.v[0][r] * f.u[0][c] + f.v[1][r] * f.u[1][c] + f.v[2][r] * f.u[2][c];
      Tout[4 * r + c] = R;
      t -= R * ca[c];
      fin = fin && isfinite(R);
    }
    Tout[4 * r + 3] = t;
    fin = fin && isfinite(t);
  }
  return fin;
}

// ---------------------------------------------------------------------------------------------------------------------------
// RANSAC
// ---------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads)
k_ransac_compact(const float* __restrict__ src, const float* __restrict__ tgt, const int* __restrict__ off,
                 const unsigned char* __restrict__ mask, float4* __restrict__ cs, float4* __restrict__ cq, int* __restrict__ cidx,
                 int* __restrict__ m_out) {
  __shared__ int wsum[kThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = off[b], n = off[b + 1] - r0;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += kThreads) {
    const int i = i0 + tid;
    const bool keep = i < n && (!mask || mask[r0 + i]);
    const unsigned long long bal = __ballot(keep);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      before += (w < wave) ? wsum[w] : 0;
      total += wsum[w];
    }
    if (keep) {
      const int pos = r0 + base + before + pre;
      const float* a = src + 3 * (size_t)(r0 + i);
      const float* q = tgt + 3 * (size_t)(r0 + i);
      cs[pos] = make_float4(a[0], a[1], a[2], 0.f);
      cq[pos] = make_float4(q[0], q[1], q[2], 0.f);
      cidx[pos] = i;
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) m_out[b] = base;
}

// grid (hb * B, Y): workgroup x scores hypotheses [256 (x % hb), +256) of pair x / hb over the y-th share of the pair's row tiles
template <int NS>
__global__ void __launch_bounds__(kThreads)
k_ransac_score(const float4* __restrict__ cs, const float4* __restrict__ cq, const int* __restrict__ off, const int* __restrict__ m_in,
               int H, int hb, unsigned long long seed, int first_pair, float tau2, float qscale, unsigned* __restrict__ cnt,
               unsigned long long* __restrict__ sq, unsigned char* __restrict__ valid, float* __restrict__ thyp) {
  __shared__ float4 tile[2 * kThreads];
  const int b = blockIdx.x / hb, tid = threadIdx.x;
  const int h = (blockIdx.x % hb) * kThreads + tid;
  const int r0 = off[b], M = m_in[b];
  if (M < NS) return;                                    // (uniform) no hypothesis: the pair reports identity
  const float4* ps = cs + r0;
  const float4* pq = cq + r0;
  const bool active = h < H;
  float T[12];
  bool ok = false;
  {
    double Td[12];
    if (active) {
      int rows[NS];
      ransac_draw<NS>(seed, (uint32_t)(first_pair + b), (uint32_t)h, (uint32_t)M, rows);
      ok = fit_sample<NS>(ps, pq, rows, Td);
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = ok ? (float)Td[e] : 0.f;
  }
  const size_t slot = (size_t)b * H + h;
  if (blockIdx.y == 0 && active) {
    valid[slot] = ok ? 1 : 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) thyp[slot * 12 + e] = T[e];
  }
  const int ntile = (M + kThreads - 1) / kThreads;
  const int t0 = (int)((long long)ntile * blockIdx.y / gridDim.y), t1 = (int)((long long)ntile * (blockIdx.y + 1) / gridDim.y);
  unsigned n_in = 0;
  unsigned long long sum = 0;
  for (int t = t0; t < t1; ++t) {
    const int rb = t * kThreads, nrow = min(kThreads, M - rb);
    __syncthreads();
    if (tid < nrow) {
      tile[tid] = ps[rb + tid];
      tile[kThreads + tid] = pq[rb + tid];
    }
    __syncthreads();
    unsigned part = 0;                                   // <= 256 rows of < 2^24 each: no overflow
    for (int j = 0; j < nrow; ++j) {
      const float4 a = tile[j], q = tile[kThreads + j];
      const float d2 = resid2(T, a.x, a.y, a.z, q.x, q.y, q.z);
      const bool in = d2 < tau2;
      n_in += in ? 1u : 0u;
      part += in ? min(__float2uint_rz(d2 * qscale), 0xFFFFFFu) : 0u;
    }
    sum += part;
  }
  if (active && ok && t1 > t0) {
    atomicAdd(cnt + slot, n_in);
    atomicAdd(sq + slot, sum);
  }
}

struct HypKey {
  unsigned valid, cnt;
  unsigned long long sq;
  int h;
};

GMF_DEVINL bool better(const HypKey& a, const HypKey& b) {
  if (a.valid != b.valid) return a.valid > b.valid;
  if (a.cnt != b.cnt) return a.cnt > b.cnt;
  if (a.sq != b.sq) return a.sq < b.sq;
  return a.h < b.h;
}

template <int NS>
__global__ void __launch_bounds__(kThreads)
k_ransac_finish(const float* __restrict__ src, const float* __restrict__ tgt, const int* __restrict__ off,
                const unsigned char* __restrict__ mask, const int* __restrict__ cidx, const int* __restrict__ m_in, int H,
                unsigned long long seed, int first_pair, float tau2, const unsigned* __restrict__ cnt,
                const unsigned long long* __restrict__ sq, const unsigned char* __restrict__ valid, const float* __restrict__ thyp,
                float* __restrict__ T_out, unsigned char* __restrict__ inliers, float* __restrict__ fitness, float* __restrict__ rmse,
                long long* __restrict__ hyp_out, long long* __restrict__ sample_out) {
  __shared__ double sh[kThreads * 2];
  __shared__ HypKey kk[kThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int r0 = off[b], n = off[b + 1] - r0, M = m_in[b];
  HypKey best = {0u, 0u, ~0ull, 0x7fffffff};
  if (M >= NS) {
    for (int h = tid; h < H; h += kThreads) {
      const size_t slot = (size_t)b * H + h;
      const HypKey c = {(unsigned)valid[slot], cnt[slot], sq[slot], h};
      if (better(c, best)) best = c;
    }
  }
  kk[tid] = best;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s && better(kk[tid + s], kk[tid])) kk[tid] = kk[tid + s];
    __syncthreads();
  }
  const HypKey w = kk[0];
  const bool have = w.valid != 0;
  float T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = have ? thyp[((size_t)b * H + w.h) * 12 + e] : ((e % 5 == 0) ? 1.f : 0.f);
  double v[2] = {0.0, 0.0};                              // inliers, sum d^2
  for (int i = tid; i < n; i += kThreads) {
    bool in = false;
    if (have && (!mask || mask[r0 + i])) {
      const float* a = src + 3 * (size_t)(r0 + i);
      const float* q = tgt + 3 * (size_t)(r0 + i);
      const float d2 = resid2(T, a[0], a[1], a[2], q[0], q[1], q[2]);
      in = d2 < tau2;
      if (in) { v[0] += 1.0; v[1] += (double)d2; }
    }
    inliers[r0 + i] = in ? 1 : 0;
  }
  tree_sum<2>(v, sh);
  if (tid == 0) {
    float* To = T_out + 16 * (size_t)b;
#pragma unroll
    for (int e = 0; e < 12; ++e) To[e] = T[e];
    To[12] = 0.f; To[13] = 0.f; To[14] = 0.f; To[15] = 1.f;
    fitness[b] = (have && M > 0) ? (float)(v[0] / M) : 0.f;
    rmse[b] = (have && v[0] > 0) ? (float)sqrt(v[1] / v[0]) : 0.f;
    hyp_out[b] = have ? w.h : -1;
    int rows[NS];
    if (have) ransac_draw<NS>(seed, (uint32_t)(first_pair + b), (uint32_t)w.h, (uint32_t)M, rows);
#pragma unroll
    for (int k = 0; k < NS; ++k) sample_out[(size_t)b * NS + k] = have ? cidx[r0 + rows[k]] : -1;
  }
}

// The scoreboard of a call's B * H hypotheses: one workspace buffer, so that one memset clears it.
struct RansacBoard {
  unsigned long long* sq;     // [B * H] sum of the inliers' d^2 in units of tau^2 / 2^24 (integer: order-free)
  unsigned* cnt;              // [B * H] inlier count per hypothesis
  unsigned char* valid;       // [B * H] 1 = the hypothesis's fit succeeded
  static constexpr size_t kBytesPerHyp = 8 + 4 + 1;
  RansacBoard(unsigned char* base, size_t BH)
      : sq(reinterpret_cast<unsigned long long*>(base)), cnt(reinterpret_cast<unsigned*>(sq + BH)),
        valid(reinterpret_cast<unsigned char*>(cnt + BH)) {}
};

void ransac_scratch_list(long long total_rows, int B, int H, RansacScratch& s, ArenaList& bufs) {
  const size_t BH = (size_t)B * H;
  bufs.add(s.cs, (size_t)total_rows);
  bufs.add(s.cq, (size_t)total_rows);
  bufs.add(s.cidx, (size_t)total_rows);
  bufs.add(s.m, (size_t)B);
  bufs.add(s.board, BH * RansacBoard::kBytesPerHyp);
  bufs.add(s.thyp, BH * 12);
}

template <int NS>
static void launch_ransac_n(const float* src, const float* tgt, const int* off, const unsigned char* mask, int B, int max_rows,
                            int H, float tau, uint64_t seed, int first_pair, const RansacScratch& ws, const RansacBoard& bd,
                            float* T_out, unsigned char* inliers, float* fitness, float* rmse, long long* hyp, long long* sample, hipStream_t s) {
  const int hb = (H + kThreads - 1) / kThreads;
  // split the rows when B * hb workgroups alone would leave CUs idle: about 2048 workgroups in all, every split >= 1 tile
  const long long wg = (long long)hb * B;
  const int tiles = std::max(1, (max_rows + kThreads - 1) / kThreads);
  const int Y = (int)std::max(1LL, std::min<long long>({(2048 + wg - 1) / wg, (long long)tiles, 64LL}));
  const float tau2 = tau * tau;
  const float qscale = 16777216.0f / tau2;
  hipLaunchKernelGGL(k_ransac_compact, dim3(B), dim3(kThreads), 0, s, src, tgt, off, mask, ws.cs, ws.cq, ws.cidx, ws.m);
  hipLaunchKernelGGL(k_ransac_score<NS>, dim3((unsigned)wg, Y), dim3(kThreads), 0, s, ws.cs, ws.cq, off, ws.m, H, hb,
                     (unsigned long long)seed, first_pair, tau2, qscale, bd.cnt, bd.sq, bd.valid, ws.thyp);
  hipLaunchKernelGGL(k_ransac_finish<NS>, dim3(B), dim3(kThreads), 0, s, src, tgt, off, mask, ws.cidx, ws.m, H,
                     (unsigned long long)seed, first_pair, tau2, bd.cnt, bd.sq, bd.valid, ws.thyp, T_out, inliers, fitness, rmse,
                     hyp, sample);
}

hipError_t launch_ransac(const float* src, const float* tgt, const int* offsets, const unsigned char* mask, int B,
                         long long total_rows, int max_rows, int ransac_n, int H, float tau, uint64_t seed, int first_pair,
                         const RansacScratch& ws, float* T_out, unsigned char* inliers, float* fitness, float* rmse,
                         long long* hypothesis, long long* sample, hipStream_t s) {
  const size_t BH = (size_t)B * H;
  const RansacBoard bd(ws.board, BH);
  hipError_t e = hipMemsetAsync(ws.board, 0, BH * RansacBoard::kBytesPerHyp, s);
  if (e != hipSuccess) return e;
  (void)total_rows;
#define GMF_RANSAC_CASE(n) \
  case n: launch_ransac_n<n>(src, tgt, offsets, mask, B, max_rows, H, tau, seed, first_pair, ws, bd, T_out, inliers, fitness, \
                             rmse, hypothesis, sample, s); break;
  switch (ransac_n) {
    GMF_RANSAC_CASE(3) GMF_RANSAC_CASE(4) GMF_RANSAC_CASE(5) GMF_RANSAC_CASE(6) GMF_RANSAC_CASE(7) GMF_RANSAC_CASE(8)
    default: return hipErrorInvalidValue;
  }
#undef GMF_RANSAC_CASE
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------
// ICP
// ---------------------------------------------------------------------------------------------------------------------------

// the source row transformed by the pair's fp64 [R | t], rounded once to fp32 (explicit fmas: k_icp_nn and k_icp_step agree)
GMF_DEVINL void transform_row(const double* T, const float* a, float* p) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
    p[r] = (float)fma(T[4 * r], (double)a[0], fma(T[4 * r + 1], (double)a[1], fma(T[4 * r + 2], (double)a[2], T[4 * r + 3])));
}

__global__ void __launch_bounds__(kThreads)
k_icp_init(const float* __restrict__ init, int B, double* __restrict__ T, double* __restrict__ prev, int* __restrict__ done) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
#pragma unroll
  for (int e = 0; e < 12; ++e) T[12 * (size_t)b + e] = (double)init[16 * (size_t)b + e];
  prev[2 * b] = 0.0;
  prev[2 * b + 1] = 0.0;
  done[b] = 0;
}

// grid (B * stiles, Y): workgroup x takes the source tiles x % stiles, + stiles, ... of pair x / stiles (every tile of any pair
// is covered whatever max_src said), and the y-th share of the pair's target tiles
__global__ void __launch_bounds__(kThreads)
k_icp_nn(const float* __restrict__ src, const int* __restrict__ soff, const float* __restrict__ tgt, const int* __restrict__ toff,
         int stiles, const double* __restrict__ Tst, const int* __restrict__ done, unsigned long long* __restrict__ key) {
  __shared__ float4 tile[kThreads];
  const int b = blockIdx.x / stiles, tid = threadIdx.x;
  if (done[b]) return;
  const int s0 = soff[b], ns = soff[b + 1] - s0, q0 = toff[b], nt = toff[b + 1] - q0;
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = Tst[12 * (size_t)b + e];
  const int ntile = (nt + kThreads - 1) / kThreads;
  const int t0 = (int)((long long)ntile * blockIdx.y / gridDim.y), t1 = (int)((long long)ntile * (blockIdx.y + 1) / gridDim.y);
  if (t1 <= t0) return;
  for (int st = blockIdx.x % stiles; st * kThreads < ns; st += stiles) {
    const int i = st * kThreads + tid;
    float p[3] = {0.f, 0.f, 0.f};
    if (i < ns) transform_row(T, src + 3 * (size_t)(s0 + i), p);
    float best = INFINITY;
    int bj = -1;
    for (int t = t0; t < t1; ++t) {
      const int jb = t * kThreads, nrow = min(kThreads, nt - jb);
      __syncthreads();
      if (tid < nrow) {
        const float* q = tgt + 3 * (size_t)(q0 + jb + tid);
        tile[tid] = make_float4(q[0], q[1], q[2], 0.f);
      }
      __syncthreads();
      for (int j = 0; j < nrow; ++j) {
        const float4 q = tile[j];
        const float dx = p[0] - q.x, dy = p[1] - q.y, dz = p[2] - q.z;
        const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
        if (d2 < best) { best = d2; bj = jb + j; }         // strict: the first (smallest) row among equal distances
      }
    }
    if (i < ns && bj >= 0)                               // d2 >= 0: its bits order as unsigned integers
      atomicMin(key + s0 + i, ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)bj);
  }
}

constexpr int kGridLanes = 32;                           // lanes per source row: one per cell of the 3 x 3 x 3 block (27 used)
constexpr int kGridRows = kThreads / kGridLanes;         // source rows per workgroup pass
constexpr int kGridBigSlot = 32;                         // a slot with more rows than this is walked by all 32 lanes

// The search of k_icp_nn restricted to the targets that can matter: a target with d^2 < tau^2 lies in one of the 27 cells (edge
// tau (1 + 2^-10)) around the transformed source row, and among those the minimum key is k_icp_nn's.  When no target is within
// tau the key stays ~0 or carries a d^2 >= tau^2; k_icp_step reads both as "no neighbour".  grid (B * qtiles): workgroup x takes
// the row groups x % qtiles, + qtiles, ... of pair x / qtiles.  A lane looks up one cell's slot and walks its rows; a hash
// collision only adds rows, which the pair test drops (a far cell of the same pair cannot win inside tau), and a slot reached
// twice changes no minimum.  One writer per key, and k_icp_step has reset it: a plain store.
__global__ void __launch_bounds__(kThreads)
k_icp_nn_grid(const float* __restrict__ src, const int* __restrict__ soff, const int* __restrict__ toff, int qtiles,
              const double* __restrict__ Tst, const int* __restrict__ done, unsigned long long tmask, double inv_h,
              const int* __restrict__ start, const float4* __restrict__ cell_pts, unsigned long long* __restrict__ key) {
  const int b = blockIdx.x / qtiles, tid = threadIdx.x;
  if (done[b]) return;
  const int g = tid & (kGridLanes - 1), half = (tid & 63) >> 5;
  const int s0 = soff[b], ns = soff[b + 1] - s0, q0 = toff[b], q1 = toff[b + 1];
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = Tst[12 * (size_t)b + e];
  // (every bound of this loop is uniform over the workgroup: the ballot and the shuffles below see whole waves)
  for (int qt = blockIdx.x % qtiles; (long long)qt * kGridRows < ns; qt += qtiles) {
    const int i = qt * kGridRows + tid / kGridLanes;
    float p[3] = {0.f, 0.f, 0.f};
    int a = 0, e = 0;                                    // this lane's slot holds cell_pts[a .. e)
    if (i < ns) {
      transform_row(T, src + 3 * (size_t)(s0 + i), p);
      if (g < 27) {
        const int s = (int)(cell_hash(b, grid_coord(p[0], inv_h) + g % 3 - 1, grid_coord(p[1], inv_h) + (g / 3) % 3 - 1,
                                      grid_coord(p[2], inv_h) + g / 9 - 1) & tmask);
        a = start[s];
        e = start[s + 1];
      }
    }
    unsigned long long best = ~0ull;
    auto visit = [&](int pos) {
      const float4 q = cell_pts[pos];
      const int j = __float_as_int(q.w);
      if (j >= q0 && j < q1) {
        const float dx = p[0] - q.x, dy = p[1] - q.y, dz = p[2] - q.z;
        const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));                      // k_icp_nn's expression, operand for operand
        const unsigned long long c = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)(j - q0);
        best = c < best ? c : best;
      }
    };
    const bool big = e - a > kGridBigSlot;
    if (!big)
      for (int pos = a; pos < e; ++pos) visit(pos);
    for (unsigned long long m = __ballot(big); m; m &= m - 1) {                    // (rare) a crowded slot: its row's 32 lanes share it
      const int l = __builtin_ctzll(m);
      const int a2 = __shfl(a, l), e2 = __shfl(e, l);
      if (half == l >> 5)
        for (int pos = a2 + g; pos < e2; pos += kGridLanes) visit(pos);
    }
#pragma unroll
    for (int o = kGridLanes / 2; o > 0; o >>= 1) {
      const unsigned long long c = __shfl_xor(best, o, kGridLanes);
      best = c < best ? c : best;
    }
    if (g == 0 && i < ns && best != ~0ull) key[s0 + i] = best;
  }
}

// pass k of the loop (k = 0: the evaluation at init): C, fitness, rmse; stop on convergence or at k == max_iter, else T <- dT T.
// Every key is read and reset to the atomicMin identity for the next k_icp_nn.
__global__ void __launch_bounds__(kThreads)
k_icp_step(const float* __restrict__ src, const int* __restrict__ soff, const float* __restrict__ tgt, const int* __restrict__ toff,
           int k, int max_iter, float tau2, double rel_f, double rel_r, double* __restrict__ Tst, double* __restrict__ prev,
           int* __restrict__ done, unsigned long long* __restrict__ key, float* __restrict__ T_out, float* __restrict__ fit_out,
           float* __restrict__ rmse_out, int* __restrict__ it_out, long long* __restrict__ nn) {
  __shared__ double sh[kThreads * 9];
  __shared__ int stop_sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (done[b]) return;
  const int s0 = soff[b], ns = soff[b + 1] - s0, q0 = toff[b];
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = Tst[12 * (size_t)b + e];
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};               // |C|, sum d^2, sum p, sum q
  for (int i = tid; i < ns; i += kThreads) {
    const unsigned long long kv = key[s0 + i];
    key[s0 + i] = ~0ull;
    const float d2 = __uint_as_float((unsigned)(kv >> 32));
    const int j = (int)(kv & 0xffffffffull);
    const bool in = kv != ~0ull && d2 < tau2;
    nn[s0 + i] = in ? j : -1;
    if (in) {
      float p[3];
      transform_row(T, src + 3 * (size_t)(s0 + i), p);
      const float* q = tgt + 3 * (size_t)(q0 + j);
      v[0] += 1.0; v[1] += (double)d2;
      v[2] += p[0]; v[3] += p[1]; v[4] += p[2];
      v[5] += q[0]; v[6] += q[1]; v[7] += q[2];
    }
  }
  tree_sum<8>(v, sh);
  const double nc = v[0];
  const double fit = nc / ns, rm = nc > 0 ? sqrt(v[1] / nc) : 0.0;
  if (tid == 0) {
    bool stop = k >= max_iter;
    if (k >= 1 && fabs(prev[2 * b] - fit) < rel_f && fabs(prev[2 * b + 1] - rm) < rel_r) stop = true;
    prev[2 * b] = fit;
    prev[2 * b + 1] = rm;
    if (stop) {
      float* To = T_out + 16 * (size_t)b;
#pragma unroll
      for (int e = 0; e < 12; ++e) To[e] = (float)T[e];
      To[12] = 0.f; To[13] = 0.f; To[14] = 0.f; To[15] = 1.f;
      fit_out[b] = (float)fit;
      rmse_out[b] = (float)rm;
      it_out[b] = k;
      done[b] = 1;
    }
    stop_sh = stop ? 1 : 0;
  }
  __syncthreads();
  if (stop_sh || nc == 0.0) return;                      // empty C: dT = identity, T stays
  const double ca[3] = {v[2] / nc, v[3] / nc, v[4] / nc}, cb[3] = {v[5] / nc, v[6] / nc, v[7] / nc};
  double Hm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < ns; i += kThreads) {
    const long long j = nn[s0 + i];                       // written by this thread above
    if (j < 0) continue;
    float p[3];
    transform_row(T, src + 3 * (size_t)(s0 + i), p);
    const float* q = tgt + 3 * (size_t)(q0 + j);
    const double am[3] = {p[0] - ca[0], p[1] - ca[1], p[2] - ca[2]};
    const double bm[3] = {q[0] - cb[0], q[1] - cb[1], q[2] - cb[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) Hm[3 * r + c] = fma(am[r], bm[c], Hm[3 * r + c]);
  }
  tree_sum<9>(Hm, sh);
  if (tid == 0) {
    double R[9];
    kabsch_rotation_from_H(Hm, R);
    double dt[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) dt[r] = cb[r] - (R[3 * r] * ca[0] + R[3 * r + 1] * ca[1] + R[3 * r + 2] * ca[2]);
    double Tn[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        Tn[4 * r + c] = R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c] + R[3 * r + 2] * T[8 + c] + (c == 3 ? dt[r] : 0.0);
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) Tst[12 * (size_t)b + e] = Tn[e];
  }
}

// Point-to-plane (open3d 0.9 TransformationEstimationPointToPlane): k_icp_step's work split in two launches.
//
// k_icp_plane_partials, grid (B * parts): workgroup x is part x % parts of pair x / parts and owns the pair's source rows
// [part R, (part + 1) R), R = kIcpPlaneRows (icp_plane_plan.hpp); a part behind the pair's rows returns.  It reads and resets
// the keys and writes nn as k_icp_step does, and leaves one partial of kIcpPlaneSums doubles: |C|, sum d^2, and over the rows of
// C with a finite normal the 21 upper entries of sum J J^T and the 6 of sum J r, J = [p x n ; n], r = (p - q) . n in fp64.
// Thread t takes the rows t, t + 256 of the part in that order; the 64 lanes of a wave fold with an xor butterfly (both
// operands of every add are the same two numbers in both lanes, so all lanes hold one sum), the four waves as (0 + 1) + (2 + 3).
// A fixed tree over rows counted from the pair's first row: the partial depends on the pair's rows alone.
__global__ void __launch_bounds__(kThreads)
k_icp_plane_partials(const float* __restrict__ src, const int* __restrict__ soff, const float* __restrict__ tgt,
                     const float* __restrict__ nrm, const int* __restrict__ toff, int parts, float tau2,
                     const double* __restrict__ Tst, const int* __restrict__ done, unsigned long long* __restrict__ key,
                     long long* __restrict__ nn, double* __restrict__ part) {
  constexpr int kWaves = kThreads / 64;
  static_assert(kWaves == 4 && kIcpPlaneRows % kThreads == 0, "the fold below is written for four waves and whole sweeps");
  __shared__ double wsum[kWaves][kIcpPlaneSums];
  const int b = blockIdx.x / parts, pt = blockIdx.x % parts, tid = threadIdx.x;
  if (done[b]) return;
  const int s0 = soff[b], ns = soff[b + 1] - s0, q0 = toff[b];
  if ((long long)pt * kIcpPlaneRows >= ns) return;
  const int r0 = pt * kIcpPlaneRows, left = ns - r0;     // rows of the pair from this part on (>= 1)
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = Tst[12 * (size_t)b + e];
  double v[kIcpPlaneSums];
#pragma unroll
  for (int e = 0; e < kIcpPlaneSums; ++e) v[e] = 0.0;
#pragma unroll
  for (int u = 0; u < kIcpPlaneRows / kThreads; ++u) {
    const int l = u * kThreads + tid;
    if (l >= left) continue;
    const size_t i = (size_t)s0 + r0 + l;
    const unsigned long long kv = key[i];
    key[i] = ~0ull;
    const float d2 = __uint_as_float((unsigned)(kv >> 32));
    const int j = (int)(kv & 0xffffffffull);
    const bool in = kv != ~0ull && d2 < tau2;
    nn[i] = in ? j : -1;
    if (!in) continue;
    v[0] += 1.0;
    v[1] += (double)d2;
    const float* n = nrm + 3 * (size_t)(q0 + j);
    const float n0 = n[0], n1 = n[1], n2 = n[2];
    if (!(isfinite(n0) && isfinite(n1) && isfinite(n2))) continue;
    float p[3];
    transform_row(T, src + 3 * i, p);
    const float* q = tgt + 3 * (size_t)(q0 + j);
    const double px = p[0], py = p[1], pz = p[2], nx = n0, ny = n1, nz = n2;
    // (the products of two fp32 are exact in fp64: each entry of p x n is rounded once)
    const double J[6] = {fma(py, nz, -(pz * ny)), fma(pz, nx, -(px * nz)), fma(px, ny, -(py * nx)), nx, ny, nz};
    const double r = fma(px - (double)q[0], nx, fma(py - (double)q[1], ny, (pz - (double)q[2]) * nz));
    int e = 2;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = a; c < 6; ++c) { v[e] = fma(J[a], J[c], v[e]); ++e; }
#pragma unroll
    for (int a = 0; a < 6; ++a) v[23 + a] = fma(J[a], r, v[23 + a]);
  }
#pragma unroll
  for (int e = 0; e < kIcpPlaneSums; ++e) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[e] += __shfl_xor(v[e], o, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int e = 0; e < kIcpPlaneSums; ++e) wsum[tid >> 6][e] = v[e];
  }
  __syncthreads();
  if (tid < kIcpPlaneSums)
    part[((size_t)b * parts + pt) * kIcpPlaneSums + tid] = (wsum[0][tid] + wsum[1][tid]) + (wsum[2][tid] + wsum[3][tid]);
}

// Coloured ICP (open3d 0.9 TransformationEstimationForColoredICP; Park, Zhou, Koltun, ICCV 2017): k_icp_plane_partials with a
// photometric term beside the geometric one.  The same grid, rows, keys, nn, |C|, sum d^2 and fold; the 27 sums of A and b hold
// the two terms of every row of C whose normal, gradient and two intensities are finite: with p, q, n as above, g the target's
// colour gradient and I_s, I_t the intensities of the source row and of its target,
//   r_G = (p - q) . n,  J_G = [p x n ; n]  (the plane form's expressions),
//   u = (p - q) - r_G n,  r_I = I_s - (g . u + I_t),  m = -(g - (g . n) n),  J_I = [p x m ; m],
// each term scaled by sg = sqrt(lambda) or si = sqrt(1 - lambda) (host doubles) before its products, so that
// A = sum lambda J_G J_G^T + (1 - lambda) J_I J_I^T and b = sum lambda J_G r_G + (1 - lambda) J_I r_I.  Every use of n is an
// even product, written so that negating n negates both operands of a multiplication or none: no output bit changes.
__global__ void __launch_bounds__(kThreads)
k_icp_color_partials(const float* __restrict__ src, const int* __restrict__ soff, const float* __restrict__ tgt,
                     const float* __restrict__ nrm, const int* __restrict__ toff, const float* __restrict__ sint,
                     const float* __restrict__ tint, const float* __restrict__ grd, double sg, double si, int parts, float tau2,
                     const double* __restrict__ Tst, const int* __restrict__ done, unsigned long long* __restrict__ key,
                     long long* __restrict__ nn, double* __restrict__ part) {
  constexpr int kWaves = kThreads / 64;
  static_assert(kWaves == 4 && kIcpPlaneRows % kThreads == 0, "the fold below is written for four waves and whole sweeps");
  __shared__ double wsum[kWaves][kIcpPlaneSums];
  const int b = blockIdx.x / parts, pt = blockIdx.x % parts, tid = threadIdx.x;
  if (done[b]) return;
  const int s0 = soff[b], ns = soff[b + 1] - s0, q0 = toff[b];
  if ((long long)pt * kIcpPlaneRows >= ns) return;
  const int r0 = pt * kIcpPlaneRows, left = ns - r0;     // rows of the pair from this part on (>= 1)
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = Tst[12 * (size_t)b + e];
  double v[kIcpPlaneSums];
#pragma unroll
  for (int e = 0; e < kIcpPlaneSums; ++e) v[e] = 0.0;
#pragma unroll
  for (int u = 0; u < kIcpPlaneRows / kThreads; ++u) {
    const int l = u * kThreads + tid;
    if (l >= left) continue;
    const size_t i = (size_t)s0 + r0 + l;
    const unsigned long long kv = key[i];
    key[i] = ~0ull;
    const float d2 = __uint_as_float((unsigned)(kv >> 32));
    const int j = (int)(kv & 0xffffffffull);
    const bool in = kv != ~0ull && d2 < tau2;
    nn[i] = in ? j : -1;
    if (!in) continue;
    v[0] += 1.0;
    v[1] += (double)d2;
    const size_t jt = (size_t)(q0 + j);
    const float* n = nrm + 3 * jt;
    const float* g = grd + 3 * jt;
    const float n0 = n[0], n1 = n[1], n2 = n[2], g0 = g[0], g1 = g[1], g2 = g[2], is = sint[i], it = tint[jt];
    if (!(isfinite(n0) && isfinite(n1) && isfinite(n2) && isfinite(g0) && isfinite(g1) && isfinite(g2) && isfinite(is) &&
          isfinite(it)))
      continue;
    float p[3];
    transform_row(T, src + 3 * i, p);
    const float* q = tgt + 3 * jt;
    const double px = p[0], py = p[1], pz = p[2], nx = n0, ny = n1, nz = n2, gx = g0, gy = g1, gz = g2;
    const double ex = px - (double)q[0], ey = py - (double)q[1], ez = pz - (double)q[2];
    // (the products of two fp32 are exact in fp64: each entry of p x n is rounded once)
    double JG[6] = {fma(py, nz, -(pz * ny)), fma(pz, nx, -(px * nz)), fma(px, ny, -(py * nx)), nx, ny, nz};
    const double rG = fma(ex, nx, fma(ey, ny, ez * nz));
    const double ux = fma(-rG, nx, ex), uy = fma(-rG, ny, ey), uz = fma(-rG, nz, ez);
    const double gn = fma(gx, nx, fma(gy, ny, gz * nz));
    const double mx = fma(gn, nx, -gx), my = fma(gn, ny, -gy), mz = fma(gn, nz, -gz);
    const double rI = ((double)is - (fma(gx, ux, fma(gy, uy, gz * uz)) + (double)it)) * si;
    double JI[6] = {fma(py, mz, -(pz * my)), fma(pz, mx, -(px * mz)), fma(px, my, -(py * mx)), mx, my, mz};
    const double rGs = rG * sg;
#pragma unroll
    for (int a = 0; a < 6; ++a) { JG[a] *= sg; JI[a] *= si; }
    int e = 2;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = a; c < 6; ++c) { v[e] = fma(JI[a], JI[c], fma(JG[a], JG[c], v[e])); ++e; }
#pragma unroll
    for (int a = 0; a < 6; ++a) v[23 + a] = fma(JI[a], rI, fma(JG[a], rGs, v[23 + a]));
  }
#pragma unroll
  for (int e = 0; e < kIcpPlaneSums; ++e) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[e] += __shfl_xor(v[e], o, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int e = 0; e < kIcpPlaneSums; ++e) wsum[tid >> 6][e] = v[e];
  }
  __syncthreads();
  if (tid < kIcpPlaneSums)
    part[((size_t)b * parts + pt) * kIcpPlaneSums + tid] = (wsum[0][tid] + wsum[1][tid]) + (wsum[2][tid] + wsum[3][tid]);
}

// One wave per pair.  Lane e < 29 adds entry e of the pair's partials in ascending part; lane 0 then does what k_icp_step does
// with its sums (fitness, rmse, the convergence test, the outputs and `done` on stop) and otherwise solves A x = -b by LDL^T
// without pivoting in a fixed order.  Pivot d_k is accepted when it is finite and d_k > 2^-40 A_kk (A_kk: the original diagonal
// entry); a rejected pivot or an empty C leaves T as it is for this pass.  dT = [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)], T <- dT T.
__global__ void __launch_bounds__(64)
k_icp_plane_solve(const int* __restrict__ soff, int parts, const double* __restrict__ part, int k, int max_iter, double rel_f,
                  double rel_r, double* __restrict__ Tst, double* __restrict__ prev, int* __restrict__ done,
                  float* __restrict__ T_out, float* __restrict__ fit_out, float* __restrict__ rmse_out, int* __restrict__ it_out) {
  __shared__ double acc[kIcpPlaneSums];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (done[b]) return;
  const int ns = soff[b + 1] - soff[b], np = icp_plane_pair_parts(ns);
  if (np > parts) {                                      // the caller's max_src was no bound for this pair: say so, loudly
    if (tid < 12) T_out[16 * (size_t)b + tid] = NAN;
    if (tid == 0) { fit_out[b] = 0.f; rmse_out[b] = 0.f; it_out[b] = -1; done[b] = 1; }
    return;
  }
  if (tid < kIcpPlaneSums) {
    // ascending p; sixteen loads are in flight before their adds, which keep that order (one load per add waits for each)
    const double* mine = part + (size_t)b * parts * kIcpPlaneSums + tid;
    double s = 0.0;
    int p = 0;
    for (; p + 16 <= np; p += 16) {
      double x[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) x[u] = mine[(size_t)(p + u) * kIcpPlaneSums];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += x[u];
    }
    for (; p < np; ++p) s += mine[(size_t)p * kIcpPlaneSums];
    acc[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = Tst[12 * (size_t)b + e];
  const double nc = acc[0];
  const double fit = nc / ns, rm = nc > 0 ? sqrt(acc[1] / nc) : 0.0;
  bool stop = k >= max_iter;
  if (k >= 1 && fabs(prev[2 * b] - fit) < rel_f && fabs(prev[2 * b + 1] - rm) < rel_r) stop = true;
  prev[2 * b] = fit;
  prev[2 * b + 1] = rm;
  if (stop) {
    float* To = T_out + 16 * (size_t)b;
#pragma unroll
    for (int e = 0; e < 12; ++e) To[e] = (float)T[e];
    To[12] = 0.f; To[13] = 0.f; To[14] = 0.f; To[15] = 1.f;
    fit_out[b] = (float)fit;
    rmse_out[b] = (float)rm;
    it_out[b] = k;
    done[b] = 1;
    return;
  }
  if (nc == 0.0) return;                                 // empty C: dT = identity, T stays
  double A[6][6], L[6][6], D[6], x[6];
  {
    int e = 2;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = a; c < 6; ++c) { A[a][c] = acc[e]; A[c][a] = acc[e]; ++e; }
  }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double d = A[c][c];
#pragma unroll
    for (int m = 0; m < c; ++m) d -= (L[c][m] * L[c][m]) * D[m];
    ok = ok && isfinite(d) && d > 0x1p-40 * A[c][c];
    D[c] = d;
#pragma unroll
    for (int i = c + 1; i < 6; ++i) {
      double l = A[i][c];
#pragma unroll
      for (int m = 0; m < c; ++m) l -= (L[i][m] * L[c][m]) * D[m];
      L[i][c] = l / d;
    }
  }
  if (!ok) return;                                       // a rejected pivot: dT = identity
#pragma unroll
  for (int i = 0; i < 6; ++i) {                          // L y = -b
    double y = -acc[23 + i];
#pragma unroll
    for (int m = 0; m < i; ++m) y -= L[i][m] * x[m];
    x[i] = y;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] /= D[i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {                         // L^T x = z
#pragma unroll
    for (int m = i + 1; m < 6; ++m) x[i] -= L[m][i] * x[m];
  }
  const double sx = sin(x[0]), cx = cos(x[0]), sy = sin(x[1]), cy = cos(x[1]), sz = sin(x[2]), cz = cos(x[2]);
  const double R[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                       sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx,
                       -sy,     cy * sx,                cy * cx};
  double Tn[12];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      Tn[4 * r + c] = R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c] + R[3 * r + 2] * T[8 + c] + (c == 3 ? x[3 + r] : 0.0);
  }
#pragma unroll
  for (int e = 0; e < 12; ++e) Tst[12 * (size_t)b + e] = Tn[e];
}

void icp_plane_scratch_list(IcpPlaneScratch& s, ArenaList& bufs) { bufs.add(s.part, s.plan.partial_doubles); }

void icp_scratch_list(long long total_src, int B, IcpScratch& s, ArenaList& bufs) {
  bufs.add(s.key, (size_t)total_src);
  bufs.add(s.T, (size_t)B * 12);
  bufs.add(s.prev, (size_t)B * 2);
  bufs.add(s.done, (size_t)B);
}

hipError_t launch_icp(const float* src, const int* src_off, const float* tgt, const int* tgt_off, int B, long long total_src,
                      int max_src, int max_tgt, const float* init, float tau, int max_iter, double rel_fitness, double rel_rmse,
                      const IcpScratch& ws, float* T_out, float* fitness, float* rmse, int* iterations, long long* nn,
                      hipStream_t s, const KnnScratch* grid, long long total_tgt, const IcpPlaneScratch* plane,
                      const IcpColorTerms* color) {
  hipError_t e = hipMemsetAsync(ws.key, 0xff, (size_t)total_src * 8, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_icp_init, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, s, init, B, ws.T, ws.prev, ws.done);
  // about 2048 workgroups per nearest-neighbour pass: source tiles x target shares
  const int stiles = std::max(1, (max_src + kThreads - 1) / kThreads);
  const long long wg = (long long)stiles * B;
  const int ttiles = std::max(1, (max_tgt + kThreads - 1) / kThreads);
  const int Y = (int)std::max(1LL, std::min<long long>({(2048 + wg - 1) / wg, (long long)ttiles, 256LL}));
  // grid search: the targets do not move, so one table serves every pass.  Cell edge tau (1 + 2^-10) in fp64: a target with
  // fp32 d^2 < tau^2 is nearer than that edge, with room for the rounding of p / h.
  const double h = (double)tau * (1.0 + 1.0 / 1024);
  const int qtiles = (int)std::max<long long>(1, std::min<long long>(((long long)max_src + kGridRows - 1) / kGridRows, (1LL << 30) / B));
  if (grid) {
    e = launch_grid_build(tgt, tgt_off, B, total_tgt, h, *grid, s);
    if (e != hipSuccess) return e;
  }
  const float tau2 = tau * tau;
  for (int k = 0; k <= max_iter; ++k) {
    if (grid)
      hipLaunchKernelGGL(k_icp_nn_grid, dim3((unsigned)((long long)qtiles * B)), dim3(kThreads), 0, s, src, src_off, tgt_off, qtiles,
                         ws.T, ws.done, (unsigned long long)grid->T - 1, 1.0 / h, grid->start, grid->cell_pts, ws.key);
    else
      hipLaunchKernelGGL(k_icp_nn, dim3((unsigned)wg, Y), dim3(kThreads), 0, s, src, src_off, tgt, tgt_off, stiles, ws.T, ws.done,
                         ws.key);
    if (plane && color) {
      hipLaunchKernelGGL(k_icp_color_partials, dim3((unsigned)plane->plan.blocks), dim3(kThreads), 0, s, src, src_off, tgt,
                         plane->normals, tgt_off, color->src_intensity, color->tgt_intensity, color->tgt_gradients,
                         color->sqrt_geometric, color->sqrt_photometric, plane->plan.parts, tau2, ws.T, ws.done, ws.key, nn,
                         plane->part);
      hipLaunchKernelGGL(k_icp_plane_solve, dim3(B), dim3(64), 0, s, src_off, plane->plan.parts, plane->part, k, max_iter,
                         rel_fitness, rel_rmse, ws.T, ws.prev, ws.done, T_out, fitness, rmse, iterations);
    } else if (plane) {
      hipLaunchKernelGGL(k_icp_plane_partials, dim3((unsigned)plane->plan.blocks), dim3(kThreads), 0, s, src, src_off, tgt,
                         plane->normals, tgt_off, plane->plan.parts, tau2, ws.T, ws.done, ws.key, nn, plane->part);
      hipLaunchKernelGGL(k_icp_plane_solve, dim3(B), dim3(64), 0, s, src_off, plane->plan.parts, plane->part, k, max_iter,
                         rel_fitness, rel_rmse, ws.T, ws.prev, ws.done, T_out, fitness, rmse, iterations);
    } else {
      hipLaunchKernelGGL(k_icp_step, dim3(B), dim3(kThreads), 0, s, src, src_off, tgt, tgt_off, k, max_iter, tau2, rel_fitness,
                         rel_rmse, ws.T, ws.prev, ws.done, ws.key, T_out, fitness, rmse, iterations, nn);
    }
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------
// Feature-matching RANSAC
// ---------------------------------------------------------------------------------------------------------------------------

// T s in fp32, and |p - q|^2: the two halves of "transform a row and take d^2".  The checker, both evaluation forms and the
// finish see a pose only through these, with k_icp_nn's d^2 expression, so a (pose, source row, target row) gives one bit pattern
// everywhere.
GMF_DEVINL void fm_point(const float* T, float sx, float sy, float sz, float* p) {
  p[0] = fmaf(T[0], sx, fmaf(T[1], sy, fmaf(T[2], sz, T[3])));
  p[1] = fmaf(T[4], sx, fmaf(T[5], sy, fmaf(T[6], sz, T[7])));
  p[2] = fmaf(T[8], sx, fmaf(T[9], sy, fmaf(T[10], sz, T[11])));
}

GMF_DEVINL float fm_d2(const float* p, float qx, float qy, float qz) {
  const float dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
  return fmaf(dx, dx, fmaf(dy, dy, dz * dz));
}

GMF_DEVINL unsigned long long fm_key(float d2, int row) {   // d2 >= 0: its bits order as unsigned integers
  return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)row;
}

// grid (hb * B): workgroup x proposes hypotheses [256 (x % hb), +256) of pair x / hb.  pass (zeroed by the launcher) gets a 1 and
// thyp the fp32 [R | t] where the sample survives: nn inside the pair's targets, the edge-length test, a fit, the distance test.
template <int NS>
__global__ void __launch_bounds__(kThreads)
k_fm_propose(const float* __restrict__ src, const int* __restrict__ soff, const float* __restrict__ tgt,
             const int* __restrict__ toff, const long long* __restrict__ nn, int H, long long Hs, int hb, unsigned long long seed,
             int first_pair, double edge_r2, float cd2, unsigned char* __restrict__ pass, float* __restrict__ thyp) {
  const int b = blockIdx.x / hb, h = (blockIdx.x % hb) * kThreads + threadIdx.x;
  const int s0 = soff[b], ns = soff[b + 1] - s0, q0 = toff[b], nt = toff[b + 1] - q0;
  if (ns < NS || nt <= 0 || h >= H) return;
  int rows[NS];
  ransac_draw<NS>(seed, (uint32_t)(first_pair + b), (uint32_t)h, (uint32_t)ns, rows);
  float4 a[NS], q[NS];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const long long j = nn[s0 + rows[k]];
    const bool inside = j >= 0 && j < nt;
    ok = ok && inside;
    const float* pa = src + 3 * (size_t)(s0 + rows[k]);
    const float* pq = tgt + 3 * (size_t)(q0 + (inside ? (int)j : 0));
    a[k] = make_float4(pa[0], pa[1], pa[2], 0.f);
    q[k] = make_float4(pq[0], pq[1], pq[2], 0.f);
  }
  if (ok && edge_r2 > 0.0) {                             // open3d's edge-length checker on squared lengths, in fp64
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
      for (int j = i + 1; j < NS; ++j) {
        const double ax = (double)a[i].x - a[j].x, ay = (double)a[i].y - a[j].y, az = (double)a[i].z - a[j].z;
        const double bx = (double)q[i].x - q[j].x, by = (double)q[i].y - q[j].y, bz = (double)q[i].z - q[j].z;
        const double ds = ax * ax + ay * ay + az * az, dt = bx * bx + by * by + bz * bz;
        ok = ok && ds >= edge_r2 * dt && dt >= edge_r2 * ds;
      }
  }
  if (!ok) return;
  int id[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) id[k] = k;
  double Td[12];
  if (!fit_sample<NS>(a, q, id, Td)) return;
  float T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = (float)Td[e];
  if (cd2 >= 0.f) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      float p[3];
      fm_point(T, a[k].x, a[k].y, a[k].z, p);
      ok = ok && fm_d2(p, q[k].x, q[k].y, q[k].z) <= cd2;
    }
    if (!ok) return;
  }
  pass[(size_t)b * Hs + h] = 1;
  float* To = thyp + ((size_t)b * H + h) * 12;
#pragma unroll
  for (int e = 0; e < 12; ++e) To[e] = T[e];
}

// One workgroup per pair: the first V passing h in increasing order (open3d's sequential rule without its dependence on the
// order of execution), by a prefix sum over four flags per thread.  hyp [B, V] (-1 padded), tval [B, V, 12].
__global__ void __launch_bounds__(kThreads)
k_fm_select(int H, long long Hs, int V, const unsigned char* __restrict__ pass, const float* __restrict__ thyp,
            int* __restrict__ hyp, float* __restrict__ tval, int* __restrict__ validated) {
  __shared__ int wsum[kThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned* pw = reinterpret_cast<const unsigned*>(pass + (size_t)b * Hs);      // Hs is a multiple of 4, the flags are 0 / 1
  const int words = (int)(Hs / 4);
  int* hb = hyp + (size_t)b * V;
  int base = 0;
  for (int w0 = 0; w0 < words && base < V; w0 += kThreads) {                           // (uniform bounds)
    const int w = w0 + tid;
    const unsigned word = w < words ? pw[w] : 0u;
    const int c = __popc(word);
    int inc = c;                                          // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o);
      inc += lane >= o ? up : 0;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) {
      before += k < wave ? wsum[k] : 0;
      total += wsum[k];
    }
    int pos = base + before + inc - c;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((word >> (8 * k)) & 1u) {
        if (pos < V) hb[pos] = 4 * w + k;
        ++pos;
      }
    base += total;
    __syncthreads();
  }
  const int nv = min(base, V);
  __syncthreads();                                        // the list above is read back below
  for (int v = tid; v < V; v += kThreads) {
    if (v >= nv) { hb[v] = -1; continue; }
    const float* Ti = thyp + ((size_t)b * H + hb[v]) * 12;
    float* To = tval + ((size_t)b * V + v) * 12;
#pragma unroll
    for (int e = 0; e < 12; ++e) To[e] = Ti[e];
  }
  if (tid == 0) validated[b] = nv;
}

struct FmGridView {
  unsigned long long tmask;
  double inv_h;
  const int* start;
  const float4* cell_pts;
};

// The evaluation: one lane per (validated hypothesis, source row); a workgroup holds 256 consecutive rows of one hypothesis, so
// the pose is uniform over the workgroup and the source loads coalesce.  The lane finds the minimum of (d^2 bits << 32 | target row) over the
// pair's targets: GRID walks the 27 cells around grid_coord(p) (nine slot bounds in flight at a time, then their rows), the other
// form streams every target through an LDS tile (a broadcast read).  KEYS = false: per hypothesis |C| and the fixed-point sum of
// d^2 over C, each wave adding its 64 rows' share by one 32-bit and one 64-bit integer atomic (integers: any split of the rows
// and any order give the same bits).  KEYS = true: the same search for the winner alone (win[b]), storing each row's key.
// A workgroup takes work items blockIdx.x, + gridDim.x, ...: item = ((pair, hypothesis), row tile rt0 < rtiles), and in it the
// tiles rt0, + rtiles, ... of 256 rows; everything that selects an item or a tile (validated, win, the offsets) is uniform over
// the workgroup, so the barriers of the LDS form are reached by all of it.
template <bool GRID, bool KEYS>
__global__ void __launch_bounds__(kThreads)
k_fm_eval(const float* __restrict__ src, const int* __restrict__ soff, const float* __restrict__ tgt, const int* __restrict__ toff,
          int B, int V, int rtiles, const int* __restrict__ validated, const int* __restrict__ win,
          const float* __restrict__ tval, FmGridView g, float tau2, float qscale, unsigned* __restrict__ cnt,
          unsigned long long* __restrict__ sq, unsigned long long* __restrict__ key) {
  __shared__ float4 tile[GRID ? 1 : kThreads];
  const int tid = threadIdx.x;
  const long long items = (long long)B * (KEYS ? 1 : V) * rtiles;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const int rt0 = (int)(w % rtiles);
    const long long bv = w / rtiles;
    const int b = (int)(KEYS ? bv : bv / V);
    const int v = KEYS ? win[b] : (int)(bv % V);
    if (KEYS ? v < 0 : v >= validated[b]) continue;
    const int s0 = soff[b], ns = soff[b + 1] - s0, q0 = toff[b], q1 = toff[b + 1];
    const size_t slot = (size_t)b * V + v;
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = tval[slot * 12 + e];
    // row tiles rt0, + rtiles, ...: every row of the pair is covered whatever max_src said
    for (int rt = rt0; (long long)rt * kThreads < ns; rt += rtiles) {
      const int i = rt * kThreads + tid;
      const bool active = i < ns;
      float p[3] = {0.f, 0.f, 0.f};
      if (active) {
        const float* a = src + 3 * (size_t)(s0 + i);
        fm_point(T, a[0], a[1], a[2], p);
      }
      unsigned long long best = ~0ull;
      if (GRID) {
        if (active) {
          const long long cx = grid_coord(p[0], g.inv_h), cy = grid_coord(p[1], g.inv_h), cz = grid_coord(p[2], g.inv_h);
#pragma unroll 1
          for (int ox = -1; ox <= 1; ++ox) {
            const unsigned long long kx = cell_hash_x(b, cx + ox);
            int lo[9], hi[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) {
              const int s = (int)(cell_hash_z(cell_hash_y(kx, cy + c / 3 - 1), cz + c % 3 - 1) & g.tmask);
              lo[c] = g.start[s];
              hi[c] = g.start[s + 1];
            }
#pragma unroll
            for (int c = 0; c < 9; ++c)
              for (int pos = lo[c]; pos < hi[c]; ++pos) {
                const float4 q = g.cell_pts[pos];
                const int j = __float_as_int(q.w);
                if (j >= q0 && j < q1) {                     // a colliding slot may list rows of another pair
                  const unsigned long long c2 = fm_key(fm_d2(p, q.x, q.y, q.z), j - q0);
                  best = c2 < best ? c2 : best;
                }
              }
          }
        }
      } else {
        const int nt = q1 - q0;
        for (int jb = 0; jb < nt; jb += kThreads) {
          const int nrow = min(kThreads, nt - jb);
          __syncthreads();
          if (tid < nrow) {
            const float* q = tgt + 3 * (size_t)(q0 + jb + tid);
            tile[tid] = make_float4(q[0], q[1], q[2], 0.f);
          }
          __syncthreads();
          for (int j = 0; j < nrow; ++j) {
            const float4 q = tile[j];
            const unsigned long long c2 = fm_key(fm_d2(p, q.x, q.y, q.z), jb + j);
            best = c2 < best ? c2 : best;
          }
        }
      }
      if (KEYS) {
        if (active) key[s0 + i] = best;
      } else {
        const float d2 = __uint_as_float((unsigned)(best >> 32));
        const bool in = active && best != ~0ull && d2 < tau2;
        const unsigned n_in = (unsigned)__popcll(__ballot(in));
        unsigned part = in ? min(__float2uint_rz(d2 * qscale), 0xFFFFFFu) : 0u;            // 64 rows of < 2^24 each: no overflow
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if ((tid & 63) == 0 && n_in) {
          atomicAdd(cnt + slot, n_in);
          atomicAdd(sq + slot, (unsigned long long)part);
        }
      }
    }
  }
}

// One workgroup per pair: the argmax over the validated hypotheses in the total order (count larger, then the fixed-point sum
// smaller, then h smaller; h increases with the list position).  A hypothesis with an empty C cannot win, as in open3d, whose
// running best starts at fitness 0.  win[b] = the list position, -1: the pair reports identity.
__global__ void __launch_bounds__(kThreads)
k_fm_winner(int V, const int* __restrict__ validated, const unsigned* __restrict__ cnt, const unsigned long long* __restrict__ sq,
            int* __restrict__ win) {
  __shared__ HypKey kk[kThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nv = validated[b];
  HypKey best = {0u, 0u, ~0ull, 0x7fffffff};
  for (int v = tid; v < nv; v += kThreads) {
    const size_t slot = (size_t)b * V + v;
    const HypKey c = {cnt[slot] > 0 ? 1u : 0u, cnt[slot], sq[slot], v};
    if (better(c, best)) best = c;
  }
  kk[tid] = best;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s && better(kk[tid + s], kk[tid])) kk[tid] = kk[tid + s];
    __syncthreads();
  }
  if (tid == 0) win[b] = kk[0].valid ? kk[0].h : -1;
}

// One workgroup per pair: the winner's C from the keys k_fm_eval<., true> left, fitness and rmse by fp64 sums in a fixed tree
// (a pair gives the same bits alone and in a batch), the pose, the hypothesis and its sample.
template <int NS>
__global__ void __launch_bounds__(kThreads)
k_fm_finish(const int* __restrict__ soff, int V, unsigned long long seed, int first_pair, float tau2, const int* __restrict__ win,
            const int* __restrict__ hyp, const float* __restrict__ tval, const unsigned long long* __restrict__ key,
            float* __restrict__ T_out, float* __restrict__ fitness, float* __restrict__ rmse, long long* __restrict__ hyp_out,
            long long* __restrict__ sample_out, long long* __restrict__ nn_out) {
  __shared__ double sh[kThreads * 2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int s0 = soff[b], ns = soff[b + 1] - s0;
  const int wv = win[b];
  const bool have = wv >= 0;
  double v[2] = {0.0, 0.0};                              // |C|, sum d^2
  for (int i = tid; i < ns; i += kThreads) {
    long long j = -1;
    if (have) {
      const unsigned long long kv = key[s0 + i];
      const float d2 = __uint_as_float((unsigned)(kv >> 32));
      if (kv != ~0ull && d2 < tau2) {
        j = (long long)(kv & 0xffffffffull);
        v[0] += 1.0;
        v[1] += (double)d2;
      }
    }
    nn_out[s0 + i] = j;
  }
  tree_sum<2>(v, sh);
  if (tid == 0) {
    const size_t slot = (size_t)b * V + (have ? wv : 0);
    float* To = T_out + 16 * (size_t)b;
#pragma unroll
    for (int e = 0; e < 12; ++e) To[e] = have ? tval[slot * 12 + e] : ((e % 5 == 0) ? 1.f : 0.f);
    To[12] = 0.f; To[13] = 0.f; To[14] = 0.f; To[15] = 1.f;
    fitness[b] = have ? (float)(v[0] / ns) : 0.f;
    rmse[b] = (have && v[0] > 0) ? (float)sqrt(v[1] / v[0]) : 0.f;
    const int h = have ? hyp[slot] : -1;
    hyp_out[b] = h;
    int rows[NS];
    if (have) ransac_draw<NS>(seed, (uint32_t)(first_pair + b), (uint32_t)h, (uint32_t)ns, rows);
#pragma unroll
    for (int k = 0; k < NS; ++k) sample_out[(size_t)b * NS + k] = have ? rows[k] : -1;
  }
}

void fm_scratch_list(long long total_src, int B, int H, int V, FmScratch& s, ArenaList& bufs) {
  const size_t Hs = ((size_t)H + 3) / 4 * 4, BV = (size_t)B * V;
  bufs.add(s.pass, (size_t)B * Hs);
  bufs.add(s.thyp, (size_t)B * H * 12);
  bufs.add(s.hyp, BV);
  bufs.add(s.cnt, BV);
  bufs.add(s.sq, BV);
  bufs.add(s.tval, BV * 12);
  bufs.add(s.win, (size_t)B);
  bufs.add(s.key, (size_t)total_src);
}

template <bool GRID>
static void launch_fm_eval(const float* src, const int* soff, const float* tgt, const int* toff, int B, int V, int rtiles,
                           const int* validated, const FmScratch& ws, const FmGridView& g, float tau2, float qscale, hipStream_t s) {
  // every validated (hypothesis, row tile) is a work item; past 2^20 workgroups a workgroup takes several
  const long long all = (long long)B * V * rtiles, one = (long long)B * rtiles;
  hipLaunchKernelGGL((k_fm_eval<GRID, false>), dim3((unsigned)std::min<long long>(all, 1LL << 20)), dim3(kThreads), 0, s, src, soff,
                     tgt, toff, B, V, rtiles, validated, ws.win, ws.tval, g, tau2, qscale, ws.cnt, ws.sq, ws.key);
  hipLaunchKernelGGL(k_fm_winner, dim3(B), dim3(kThreads), 0, s, V, validated, ws.cnt, ws.sq, ws.win);
  hipLaunchKernelGGL((k_fm_eval<GRID, true>), dim3((unsigned)std::min<long long>(one, 1LL << 20)), dim3(kThreads), 0, s, src, soff,
                     tgt, toff, B, V, rtiles, validated, ws.win, ws.tval, g, tau2, qscale, ws.cnt, ws.sq, ws.key);
}

template <int NS>
static void launch_fm_n(const float* src, const int* soff, const float* tgt, const int* toff, const long long* nn, int B,
                        int rtiles, int H, int V, float tau, float checker_distance, float edge_length, uint64_t seed,
                        int first_pair, const FmScratch& ws, const KnnScratch* grid, double h, float* T_out, float* fitness,
                        float* rmse, long long* hypothesis, long long* sample, long long* nn_out, int* validated, hipStream_t s) {
  const int hb = (H + kThreads - 1) / kThreads;
  const long long Hs = ((long long)H + 3) / 4 * 4;
  const float tau2 = tau * tau, qscale = 16777216.0f / tau2;
  const float cd2 = checker_distance >= 0.f ? checker_distance * checker_distance : -1.f;
  const double er2 = edge_length > 0.f ? (double)edge_length * (double)edge_length : 0.0;
  hipLaunchKernelGGL(k_fm_propose<NS>, dim3((unsigned)((long long)hb * B)), dim3(kThreads), 0, s, src, soff, tgt, toff, nn, H, Hs,
                     hb, (unsigned long long)seed, first_pair, er2, cd2, ws.pass, ws.thyp);
  hipLaunchKernelGGL(k_fm_select, dim3(B), dim3(kThreads), 0, s, H, Hs, V, ws.pass, ws.thyp, ws.hyp, ws.tval, validated);
  FmGridView g = {0ull, 0.0, nullptr, nullptr};
  if (grid) {
    g.tmask = (unsigned long long)grid->T - 1;
    g.inv_h = 1.0 / h;
    g.start = grid->start;
    g.cell_pts = grid->cell_pts;
    launch_fm_eval<true>(src, soff, tgt, toff, B, V, rtiles, validated, ws, g, tau2, qscale, s);
  } else {
    launch_fm_eval<false>(src, soff, tgt, toff, B, V, rtiles, validated, ws, g, tau2, qscale, s);
  }
  hipLaunchKernelGGL(k_fm_finish<NS>, dim3(B), dim3(kThreads), 0, s, soff, V, (unsigned long long)seed, first_pair, tau2, ws.win,
                     ws.hyp, ws.tval, ws.key, T_out, fitness, rmse, hypothesis, sample, nn_out);
}

hipError_t launch_ransac_feature_matching(const float* src, const int* src_off, const float* tgt, const int* tgt_off,
                                          const long long* nn, int B, long long total_src, long long total_tgt, int max_src,
                                          int ransac_n, int H, int V, float tau, float checker_distance, float edge_length,
                                          uint64_t seed, int first_pair, const FmScratch& ws, const KnnScratch* grid, float* T_out,
                                          float* fitness, float* rmse, long long* hypothesis, long long* sample, long long* nn_out,
                                          int* validated, hipStream_t s) {
  const size_t Hs = ((size_t)H + 3) / 4 * 4, BV = (size_t)B * V;
  hipError_t e = hipMemsetAsync(ws.pass, 0, (size_t)B * Hs, s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(ws.cnt, 0, BV * 4, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(ws.sq, 0, BV * 8, s)) != hipSuccess) return e;
  // cell edge tau (1 + 2^-10), as for ICP: a target with fp32 d^2 < tau^2 is in one of the 27 cells
  const double h = (double)tau * (1.0 + 1.0 / 1024);
  if (grid) {
    e = launch_grid_build(tgt, tgt_off, B, total_tgt, h, *grid, s);
    if (e != hipSuccess) return e;
  }
  const int rtiles = (int)std::max<long long>(1, ((long long)std::min<long long>(max_src, total_src) + kThreads - 1) / kThreads);
#define GMF_FM_CASE(n) \
  case n: launch_fm_n<n>(src, src_off, tgt, tgt_off, nn, B, rtiles, H, V, tau, checker_distance, edge_length, seed, first_pair, ws, \
                         grid, h, T_out, fitness, rmse, hypothesis, sample, nn_out, validated, s); break;
  switch (ransac_n) {
    GMF_FM_CASE(3) GMF_FM_CASE(4) GMF_FM_CASE(5) GMF_FM_CASE(6) GMF_FM_CASE(7) GMF_FM_CASE(8)
    default: return hipErrorInvalidValue;
  }
#undef GMF_FM_CASE
  return hipGetLastError();
}

}  // namespace gmf
