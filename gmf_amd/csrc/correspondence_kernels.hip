// PointDSC's correspondence set on the device.  Replaces the body of the reference's loaders,
//   GMF_PointDSC/datasets/ThreeDMatch.py:163-210, KITTI.py:94-129, demo_registration.py:101-107:
//       distance = sqrt(2 - 2 Fs Ft^T + 1e-6); source_idx = argmin(axis=1); target_idx = argmin(axis=0)
//       mutual = target_idx[source_idx] == arange; corr = (where(mutual), source_idx[mutual])
//       labels = |R x_src + t - x_tgt| < inlier_threshold; corr_pos = [x_src, x_tgt] - mean   (in_dim 6)
// for B ragged pairs in five launches: prep (match_kernels.hip), the two-sided sweep, flag, scan, emit.  Every score (i, j) is
// formed ONCE; its row minimum and its column minimum are two folds of the same bits, so "j is i's argmin" and "i is j's argmin"
// cannot disagree about a score.  No workgroup waits for another anywhere in the chain: the scan is a launch of its own.
#include "launchers_correspondence.hpp"
#include "match_common.hpp"
#include "mfma_core.hpp"

namespace gmf {

// order-preserving map of the finite floats and +-inf to unsigned words (-0 -> +0 first: the two compare equal as floats)
GMF_DEVINL unsigned score_word(float v) {
  const unsigned u = __float_as_uint(v + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the value of lane ^ M: inside a quad (M = 1, 2) a DPP move on the vector pipe, beyond it through the LDS crossbar
template <int M>
GMF_DEVINL int lane_xor(int v) {
  if constexpr (M == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);        // quad_perm [1, 0, 3, 2]
  else if constexpr (M == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);   // quad_perm [2, 3, 0, 1]
  else return __shfl_xor(v, M, 64);
}
template <int M>
GMF_DEVINL float lane_xor(float v) { return __int_as_float(lane_xor<M>(__float_as_int(v))); }

// One level of the butterfly reduce-scatter over the rows of a half-wave: a lane holds 2 H candidates (score, row) for 2 H keys,
// its partner lane ^ M the same keys for other rows.  The lane keeps the half of the keys its bit selects and receives the partner's
// candidates for them; the smaller score wins, among equal scores the smaller row.  H exchanges, not 2 H.
template <int H, int M>
GMF_DEVINL void fold_level(const float (&v)[2 * H], const int (&vi)[2 * H], float (&o)[H], int (&oi)[H], bool bit) {
#pragma unroll
  for (int q = 0; q < H; ++q) {
    const float keep = bit ? v[q + H] : v[q], send = bit ? v[q] : v[q + H];
    const int keepi = bit ? vi[q + H] : vi[q], sendi = bit ? vi[q] : vi[q + H];
    const float ov = lane_xor<M>(send);
    const int ovi = lane_xor<M>(sendi);
    const bool take = ov < keep || (ov == keep && ovi < keepi);
    o[q] = take ? ov : keep;
    oi[q] = take ? ovi : keepi;
  }
}

// k_nn_match_batched (match_kernels.hip) with a second fold of the same scores: per key j of the pair the minimum over the pair's
// source rows of (score word | source row), into colbest[key0 + j].  Mode 0 only (constant key norms: the score is symmetric in the
// two sides).  The row side is the existing kernel's, statement for statement.
// Column side, per 32 x 32 tile and wave: acc holds 16 keys in registers and 32 rows on the lanes of each half-wave; a butterfly
// reduce-scatter (lane ^ 1 keeps 8 keys, ^ 2 keeps 4, ^ 4 2, ^ 8 1, ^ 16 1: 16 exchanges) leaves one key's minimum on each lane.  The
// four waves' minima of a STAGE meet in the LDS (two buffers, so that the barrier every stage already has in acquire() is the only
// one) and threads 0 .. 32 TPS - 1 issue one 64-bit atomic minimum per key, workgroup and stage - after a plain read of colbest that
// drops what cannot win: a stale read only costs an atomic, never a result.
//   - rows at or beyond n0 of the pair's last tile are zero in the image and would score 0: they enter as +inf
//   - padding waves (tile_raw >= tiles0) re-run the last tile for the barriers' sake: they fold nothing and are left out of the combine
//   - keys at or beyond n1 (the last tile's tail, the tiles that pad a stage) are never written
//   - NaN and +inf scores never win a row (sc < best is false) and never win a column either
template <int KG>
__global__ void __launch_bounds__(256, 2)
k_nn_match_mutual_batched(const float* __restrict__ f0_img, const float* __restrict__ f1_img, const float* __restrict__ f1_norm2,
                          unsigned long long* __restrict__ best_out, unsigned long long* colbest, const MatchPair* __restrict__ tab,
                          int B) {
  constexpr int K = 8 * KG, KF = 4 * KG;
  constexpr int TPS = (4096 / (32 * K)) > 0 ? (4096 / (32 * K)) : 1;
  constexpr int kStage = TPS * 32 * K;
  constexpr int kKeys = TPS * 32;                                   // keys of a stage
  __shared__ __attribute__((aligned(16))) float lds[2 * kStage];
  __shared__ unsigned long long part[2][4][kKeys];
  const int lane = threadIdx.x & 63, h = lane >> 5, i = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int pb = match_pair_of(B, blockIdx.x, [&](int b) { return tab[b].wg0; });
  const MatchPair mp = tab[pb];
  const int local = (int)blockIdx.x - mp.wg0;
  const int bx = local % mp.wgx, by = local / mp.wgx;
  const int tiles0 = (mp.n0 + 31) / 32, tiles1 = (mp.n1 + 31) / 32;
  const int tile_raw = bx * 4 + wave;
  const bool active = tile_raw < tiles0;
  const int tile = active ? tile_raw : tiles0 - 1;

  float a[KF];
  load_frag_p32<KF>(a, f0_img + (size_t)(mp.tile0 + tile) * (32 * K), lane);

  const int s0 = (int)(((long)mp.stages * by) / mp.ks), s1 = (int)(((long)mp.stages * (by + 1)) / mp.ks);
  const int stages = s1 - s0;
  const float* norm_pair = f1_norm2 + (size_t)mp.stage0 * (TPS * 32);
  StageStream ss;
  ss.stage_floats = kStage;
  ss.init(lds, lds + kStage, wave, 4, lane, f1_img + (size_t)(mp.stage0 + s0) * kStage, stages);
  ss.prime();
  float best = INFINITY;
  int bidx = 0x7fffffff;
  const int row = tile * 32 + i;
  const bool row_ok = active && row < mp.n0;
  // the key of the tile this lane owns after the butterfly: register r = 8 b0 + 4 b1 + 2 b2 + b3 of half h (bits of i)
  const int r_own = ((i & 1) << 3) | ((i & 2) << 1) | ((i & 4) >> 1) | ((i & 8) >> 3);
  const int k_own = 4 * h + 8 * (r_own >> 2) + (r_own & 3);

  // the four waves' minima of stage `st` (already behind a barrier) -> colbest
  auto combine = [&](int st) {
    const int tid = threadIdx.x;
    if (tid < kKeys) {
      unsigned long long m = ~0ull;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (bx * 4 + w < tiles0) { const unsigned long long v = part[st & 1][w][tid]; m = v < m ? v : m; }
      const int key = (s0 + st) * kKeys + tid;
      if (key < mp.n1 && m != ~0ull) {
        unsigned long long* p = colbest + (size_t)mp.key0 + key;
        if (m < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, m);
      }
    }
  };

  for (int st = 0; st < stages; ++st) {
    const float4* lw = ss.acquire();
    if (st > 0) combine(st - 1);
#pragma unroll
    for (int tt = 0; tt < TPS; ++tt) {
      const int t = (s0 + st) * TPS + tt;
      if (t < tiles1) {
        const int jbase = t * 32 + 4 * h;
        const float4* np = reinterpret_cast<const float4*>(norm_pair + jbase);
        const float4 n0 = np[0], n1 = np[2], n2 = np[4], n3 = np[6];
        const float nn[16] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, n3.x, n3.y, n3.z, n3.w};
        f32x16 acc = zero16();
        mma_wx<KF>(acc, lw + tt * (32 * K / 4), a);
        float cv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = jbase + 8 * (r >> 2) + (r & 3);
          const float sc = fmaf(-2.0f, acc[r], nn[r]);
          if (sc < best) { best = sc; bidx = j; }
          cv[r] = (row_ok && sc < INFINITY) ? sc : INFINITY;
        }
        if (active) {                                               // (wave-uniform)
          // level 0 by hand: both rows are known (row, row ^ 1), only the scores travel
          float v8[8], v4[4], v2[2], v1[1];
          int i8[8], i4[4], i2[2], i1[1];
          const bool b0 = i & 1;
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const float keep = b0 ? cv[q + 8] : cv[q], send = b0 ? cv[q] : cv[q + 8];
            const float ov = lane_xor<1>(send);
            const bool take = ov < keep || (ov == keep && b0);      // the partner's row is the smaller one exactly when b0
            v8[q] = take ? ov : keep;
            i8[q] = take ? (row ^ 1) : row;
          }
          fold_level<4, 2>(v8, i8, v4, i4, i & 2);
          fold_level<2, 4>(v4, i4, v2, i2, i & 4);
          fold_level<1, 8>(v2, i2, v1, i1, i & 8);
          const float ov = __shfl_xor(v1[0], 16, 64);
          const int ovi = __shfl_xor(i1[0], 16, 64);
          const bool take = ov < v1[0] || (ov == v1[0] && ovi < i1[0]);
          const float fv = take ? ov : v1[0];
          const int fi = take ? ovi : i1[0];
          if (i < 16)
            part[st & 1][wave][tt * 32 + k_own] = fv < INFINITY ? ((unsigned long long)score_word(fv) << 32) | (unsigned)fi : ~0ull;
        }
      }
    }
  }
  __syncthreads();
  if (stages > 0) combine(stages - 1);
  {
    const float ov = __shfl_xor(best, 32, 64);
    const int oi = __shfl_xor(bidx, 32, 64);
    if (ov < best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
  }
  if (row_ok && h == 0 && bidx != 0x7fffffff)
    atomicMin(best_out + (size_t)mp.row0 + row, ((unsigned long long)score_word(best) << 32) | (unsigned)bidx);
}

// Per chunk of a pair's source rows (corr_plan.hpp): k_nn_finish_batched's work for every row - the winner, local to the pair, and
// its distance by the reference's formula - and the flag: with colbest, whether the winner's own best source row is this row (a row
// without a winner, all scores NaN, is never flagged); without, every row that has a winner.  With keypoints also the row's rank
// among the chunk's flagged rows, the chunk's count and the chunk's sums of the six coordinates over the flagged rows, reduced in a
// fixed tree: bits that depend on the chunk's rows alone.
__global__ void __launch_bounds__(kCorrChunk)
k_corr_flag(const unsigned long long* __restrict__ best, const unsigned long long* __restrict__ colbest, const float* __restrict__ F0,
            const float* __restrict__ F1, const float* __restrict__ kp0, const float* __restrict__ kp1,
            const MatchPair* __restrict__ tab, const CorrChunk* __restrict__ chunks, int d, int* __restrict__ idx_out,
            float* __restrict__ dist_out, unsigned char* __restrict__ mutual_out, int* __restrict__ rank_out,
            int* __restrict__ chunk_cnt, float* __restrict__ chunk_sum) {
  __shared__ int wcnt[4];
  __shared__ float wsum[4][6];
  const CorrChunk ck = chunks[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool in = tid < ck.n;
  bool flag = false;
  int bidx = 0;
  const int row = ck.row0 + tid;
  const int N1 = tab[ck.pair].n1, key0 = tab[ck.pair].key0;
  if (in) {
    const unsigned bi = (unsigned)(best[row] & 0xffffffffull);
    const bool won = bi < (unsigned)N1;
    bidx = won ? (int)bi : 0;
    const float* pa = F0 + (size_t)row * d;
    const float* pb1 = F1 + ((size_t)key0 + bidx) * d;
    float dot = 0.f;
    for (int k = 0; k < d; ++k) dot = fmaf(pa[k], pb1[k], dot);
    idx_out[row] = bidx;
    dist_out[row] = sqrtf(2.0f - 2.0f * dot + 1e-6f);
    flag = won && (!colbest || (unsigned)(colbest[(size_t)key0 + bidx] & 0xffffffffull) == (unsigned)(row - tab[ck.pair].row0));
    mutual_out[row] = flag ? 1 : 0;
  }
  if (!rank_out) return;                                            // (uniform: flags only)
  const unsigned long long bal = __ballot(flag);
  const int before = __popcll(bal & ((1ull << lane) - 1ull));
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (flag) {
    const float* p = kp0 + (size_t)row * 3;
    const float* q = kp1 + ((size_t)key0 + bidx) * 3;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = q[0]; v[4] = q[1]; v[5] = q[2];
  }
#pragma unroll
  for (int c = 0; c < 6; ++c)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v[c] += __shfl_down(v[c], m, 64);
  if (lane == 0) {
    wcnt[wave] = __popcll(bal);
#pragma unroll
    for (int c = 0; c < 6; ++c) wsum[wave][c] = v[c];
  }
  __syncthreads();
  int off = 0;
  for (int w = 0; w < wave; ++w) off += wcnt[w];
  if (in) rank_out[row] = off + before;
  if (tid == 0) chunk_cnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  if (tid < 6) chunk_sum[(size_t)blockIdx.x * 6 + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
}

// One workgroup per pair, a launch of its own behind k_corr_flag (nothing here waits for another workgroup): the pair's first output
// row = the flagged rows of all chunks before the pair's (integers: any order), then over the pair's chunks in chunk order their
// exclusive offsets, the pair's count M and the coordinate sums, and the means = sum / M.
__global__ void __launch_bounds__(64)
k_corr_scan(const int* __restrict__ chunk_cnt, const float* __restrict__ chunk_sum, const int* __restrict__ pair_chunk0, int B,
            int* __restrict__ chunk_excl, int* __restrict__ out_offsets, float* __restrict__ mean) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int c0 = pair_chunk0[b], c1 = pair_chunk0[b + 1];
  int before = 0;
  for (int c = lane; c < c0; c += 64) before += chunk_cnt[c];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) before += __shfl_xor(before, m, 64);
  if (lane != 0) return;
  int run = 0;
  float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c = c0; c < c1; ++c) {
    chunk_excl[c] = run;
    run += chunk_cnt[c];
    for (int k = 0; k < 6; ++k) s[k] += chunk_sum[(size_t)c * 6 + k];
  }
  out_offsets[b] = before;
  if (b == B - 1) out_offsets[B] = before + run;
  for (int k = 0; k < 6; ++k) mean[b * 6 + k] = run > 0 ? s[k] / (float)run : 0.f;
}

// Every flagged row writes its output row at out_offsets[pair] + the chunk's offset + its rank: source order, the reference's
// np.where order.
__global__ void __launch_bounds__(kCorrChunk)
k_corr_emit(const CorrChunk* __restrict__ chunks, const MatchPair* __restrict__ tab, const unsigned char* __restrict__ mutual,
            const int* __restrict__ idx, const int* __restrict__ rank, const int* __restrict__ chunk_excl,
            const int* __restrict__ out_offsets, const float* __restrict__ mean, const float* __restrict__ kp0,
            const float* __restrict__ kp1, const float* __restrict__ F0, const float* __restrict__ F1, int d, int in_dim,
            const float* __restrict__ gt_trans, float thr, long long* __restrict__ corr, float* __restrict__ src_out,
            float* __restrict__ tgt_out, float* __restrict__ corr_pos, float* __restrict__ src_desc_out,
            float* __restrict__ tgt_desc_out, float* __restrict__ labels) {
  const CorrChunk ck = chunks[blockIdx.x];
  const int tid = threadIdx.x;
  if (tid >= ck.n) return;
  const int row = ck.row0 + tid;
  if (!mutual[row]) return;
  const MatchPair& mp = tab[ck.pair];
  const int j = idx[row];
  const size_t o = (size_t)out_offsets[ck.pair] + chunk_excl[blockIdx.x] + rank[row];
  const float* p = kp0 + (size_t)row * 3;
  const float* q = kp1 + ((size_t)mp.key0 + j) * 3;
  const float x[6] = {p[0], p[1], p[2], q[0], q[1], q[2]};
  corr[2 * o] = row - mp.row0;
  corr[2 * o + 1] = j;
  for (int c = 0; c < 3; ++c) { src_out[3 * o + c] = x[c]; tgt_out[3 * o + c] = x[3 + c]; }
  if (in_dim == 6) {
    const float* mu = mean + ck.pair * 6;
    for (int c = 0; c < 6; ++c) corr_pos[6 * o + c] = x[c] - mu[c];
  } else {
    for (int c = 0; c < 3; ++c) corr_pos[3 * o + c] = x[c] - x[3 + c];
  }
  if (src_desc_out) {
    const float* fa = F0 + (size_t)row * d;
    const float* fb = F1 + ((size_t)mp.key0 + j) * d;
    for (int k = 0; k < d; ++k) { src_desc_out[o * d + k] = fa[k]; tgt_desc_out[o * d + k] = fb[k]; }
  }
  if (labels) {
    const float* T = gt_trans + (size_t)ck.pair * 16;
    float d2 = 0.f;
    for (int c = 0; c < 3; ++c) {
      const float w = fmaf(T[4 * c + 2], x[2], fmaf(T[4 * c + 1], x[1], fmaf(T[4 * c], x[0], T[4 * c + 3])));
      const float df = w - x[3 + c];
      d2 = fmaf(df, df, d2);
    }
    labels[o] = sqrtf(d2) < thr ? 1.f : 0.f;
  }
}

hipError_t launch_corr_match(const CorrArgs& a, const MatchTotals& tot, hipStream_t s) {
  const int K = padded_desc_width(a.d);
  if (K < 0) return hipErrorInvalidValue;
  unsigned long long* colbest = a.use_mutual ? a.colbest : nullptr;
  if (hipError_t e = launch_match_prep_batched(a.F0, a.F1, a.f0_img, a.f1_img, a.norm2, a.best, colbest, a.n_keys, a.tab, a.B, tot, a.d, 0, s))
    return e;
  if (!a.use_mutual) {                                               // no column side: the sweep is the existing kernel
    if (hipError_t e = launch_match_sweep_batched(a.f0_img, a.f1_img, a.norm2, a.best, a.tab, a.B, tot, a.d, s)) return e;
  } else {
    const dim3 grid((unsigned)tot.wgs);
    switch (K) {
      case 32: hipLaunchKernelGGL(k_nn_match_mutual_batched<4>, grid, dim3(256), 0, s, a.f0_img, a.f1_img, a.norm2, a.best, colbest, a.tab, a.B); break;
      case 40: hipLaunchKernelGGL(k_nn_match_mutual_batched<5>, grid, dim3(256), 0, s, a.f0_img, a.f1_img, a.norm2, a.best, colbest, a.tab, a.B); break;
      case 64: hipLaunchKernelGGL(k_nn_match_mutual_batched<8>, grid, dim3(256), 0, s, a.f0_img, a.f1_img, a.norm2, a.best, colbest, a.tab, a.B); break;
      default: hipLaunchKernelGGL(k_nn_match_mutual_batched<16>, grid, dim3(256), 0, s, a.f0_img, a.f1_img, a.norm2, a.best, colbest, a.tab, a.B); break;
    }
  }
  hipLaunchKernelGGL(k_corr_flag, dim3(a.n_chunks), dim3(kCorrChunk), 0, s, a.best, colbest, a.F0, a.F1, a.kp0, a.kp1, a.tab, a.chunks, a.d,
                     a.idx, a.dist, a.mutual, a.kp0 ? a.rank : nullptr, a.chunk_cnt, a.chunk_sum);
  return hipGetLastError();
}

hipError_t launch_corr_emit(const CorrArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_corr_scan, dim3(a.B), dim3(64), 0, s, a.chunk_cnt, a.chunk_sum, a.pair_chunk0, a.B, a.chunk_excl, a.out_offsets,
                     a.mean);
  hipLaunchKernelGGL(k_corr_emit, dim3(a.n_chunks), dim3(kCorrChunk), 0, s, a.chunks, a.tab, a.mutual, a.idx, a.rank, a.chunk_excl,
                     a.out_offsets, a.mean, a.kp0, a.kp1, a.F0, a.F1, a.d, a.in_dim, a.gt_trans, a.inlier_threshold, a.corr, a.src_out,
                     a.tgt_out, a.corr_pos, a.src_desc_out, a.tgt_desc_out, a.labels);
  return hipGetLastError();
}

}  // namespace gmf
