// Sparse coordinate engine and sparse convolution of MinkowskiEngine-style networks over up to 6-D coordinates (the inlier
// network of GMF_DeepGlobalRegistration/*/model/resunet_new.py:424-721).  Contract: gmf_amd/sparse.py.
//
// Levels (tensor stride 1, 2, 4, ...), all sized from the input row count M, row counts kept on the device:
//   level 0          the input rows in input order (k_load_level0).
//   level l + 1      the unique floor(c / 2t) * 2t of level l, batch index kept: k_coarse_keys writes each row's coarse key,
//                    a stable merge sort orders the rows by (valid, batch, c_1 .. c_D), k_heads flags the first row of each
//                    run of equal keys, a scan numbers them and k_emit writes them, so every coarse level is sorted and
//                    independent of the input row order.
//   hash table       per level, T = pow2 >= 2M slots of row indices; atomicCAS on the slot, equality on the full key
//                    (k_insert).  A second insertion of an equal key at level 0 is a duplicate input row: a status bit.
// Kernel maps: one wave per output row, one lane per offset, looks each neighbour up (k_map<false> counts, a scan, k_map<true>
//   fills): CSR of (offset, input row), ascending offset per output row.
// Offset-major lists: per map, a stable radix sort of the CSR pair indices by offset (k_pair_keys, then k_off_start): the pairs
//   of one offset in ascending output row, each output row at most once.
// Convolution (k_sparse_conv, k_split_reduce): the offsets are cut into nsplit fixed slices.  A workgroup owns (slice, 64 output
//   channels, output-row group) and walks its slice's offsets in ascending order, 64 real pairs per tile: W_d is read once per
//   tile, only real input rows are gathered, and the tile's product goes into the slice's partial row (written on the row's first
//   offset of the slice, added to after).  k_split_reduce adds a row's slices in slice order and applies the epilogue.  Every
//   output element has one fixed order: per offset, 16-channel FMA chains added in channel order; offsets ascending within a
//   slice; slices ascending.  No float atomics: results are bitwise repeatable and independent of the input row order and of the
//   row grouping.
// Narrow-input convolution (k_sparse_conv_narrow, FCGF's conv1: Cin <= 8, Cout <= 64): one group of lanes per output row reads
//   the row's CSR pairs directly, one fma chain per element over the pairs in ascending offset; W in LDS when it fits.
// FCGF head (k_sparse_head_l2): conv1_tr (1x1) on [x_a | x_b], ReLU, final (1x1) + bias and the optional L2 normalisation of
//   each row, one wave per row, both weight blocks in LDS.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <limits.h>

#include "launchers_sparse.hpp"

#define GMF_DEVINL __device__ __forceinline__

namespace gmf {

namespace {

constexpr int kThreads = kSparseWgThreads;
constexpr int kKI = kSparseKeyInts;

int blocks(long long n, int per) { return (int)((n + per - 1) / per); }
size_t a256(size_t b) { return (b + 255) / 256 * 256; }

// Floor semantics of a coarse coordinate: floor(c / s) * s for any sign of c (Python's c // s * s).  The one place that
// decides it (assumptions read from MinkowskiEngine).
GMF_DEVINL int coarse_coord(int c, int s) {
  const int m = ((c % s) + s) % s;
  return c - m;
}

GMF_DEVINL unsigned hash_key(const int* k, int nk) {
  unsigned long long h = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < nk; ++i) {
    h ^= (unsigned)k[i];
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
  }
  return (unsigned)h;
}

GMF_DEVINL bool key_eq(const int* a, const int* b, int nk) {
  for (int i = 0; i < nk; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

GMF_DEVINL int table_find(const int* __restrict__ coords, const int* __restrict__ table, unsigned tmask, const int* key, int nk) {
  unsigned s = hash_key(key, nk) & tmask;
  while (true) {
    const int r = table[s];
    if (r < 0) return -1;
    if (key_eq(coords + (size_t)r * kKI, key, nk)) return r;
    s = (s + 1) & tmask;
  }
}

__global__ __launch_bounds__(kThreads) void k_load_level0(const int* __restrict__ in, int M, int D, int* __restrict__ lvl,
                                                          int* __restrict__ counts) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) counts[0] = M;
  if (i >= M) return;
  for (int c = 0; c < kKI; ++c) lvl[(size_t)i * kKI + c] = c <= D ? in[(size_t)i * (D + 1) + c] : 0;
}

// the table has at least 2 n slots, so the probe always ends
__global__ __launch_bounds__(kThreads) void k_insert(const int* __restrict__ coords, const int* __restrict__ count, int nk,
                                                     int* __restrict__ table, unsigned tmask, int* status, int dup_bit) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= *count) return;
  const int* key = coords + (size_t)i * kKI;
  unsigned s = hash_key(key, nk) & tmask;
  while (true) {
    const int prev = atomicCAS(&table[s], -1, i);
    if (prev == -1) return;
    if (key_eq(coords + (size_t)prev * kKI, key, nk)) {
      if (dup_bit) atomicOr(status, dup_bit);
      return;
    }
    s = (s + 1) & tmask;
  }
}

// key of row i: (batch, coarse c_1 .. c_D, 0 ..., valid ? 0 : 1 in the last int)
__global__ __launch_bounds__(kThreads) void k_coarse_keys(const int* __restrict__ coords, const int* __restrict__ count, int M,
                                                          int D, int s2, int* __restrict__ keys, int* __restrict__ idx) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= M) return;
  idx[i] = i;
  int* k = keys + (size_t)i * kKI;
  const bool valid = i < *count;
  for (int c = 0; c < kKI; ++c) k[c] = 0;
  if (!valid) {
    k[kKI - 1] = 1;
    return;
  }
  const int* r = coords + (size_t)i * kKI;
  k[0] = r[0];
  for (int d = 1; d <= D; ++d) k[d] = coarse_coord(r[d], s2);
}

struct KeyLess {
  const int* keys;
  __host__ __device__ bool operator()(const int& a, const int& b) const {
    const int* ka = keys + (size_t)a * kKI;
    const int* kb = keys + (size_t)b * kKI;
    if (ka[kKI - 1] != kb[kKI - 1]) return ka[kKI - 1] < kb[kKI - 1];
    for (int c = 0; c < kKI - 1; ++c)
      if (ka[c] != kb[c]) return ka[c] < kb[c];
    return false;
  }
};

__global__ __launch_bounds__(kThreads) void k_heads(const int* __restrict__ keys, const int* __restrict__ idx, int M, int nk,
                                                    int* __restrict__ flags) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j == 0) flags[M] = 0;
  if (j >= M) return;
  const int* k = keys + (size_t)idx[j] * kKI;
  int h = 0;
  if (k[kKI - 1] == 0) h = (j == 0) || !key_eq(k, keys + (size_t)idx[j - 1] * kKI, nk);
  flags[j] = h;
}

__global__ __launch_bounds__(kThreads) void k_emit(const int* __restrict__ keys, const int* __restrict__ idx,
                                                   const int* __restrict__ flags, const int* __restrict__ pos, int M,
                                                   int* __restrict__ out, int* __restrict__ out_count) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j == 0) *out_count = pos[M];
  if (j >= M || !flags[j]) return;
  const int* k = keys + (size_t)idx[j] * kKI;
  int* o = out + (size_t)pos[j] * kKI;
  for (int c = 0; c < kKI - 1; ++c) o[c] = k[c];
  o[kKI - 1] = 0;
}

// neighbour of output row `base` through offset index d: base + sign * (offset of d) * t, the first spatial axis varying
// fastest in d (assumptions read from MinkowskiEngine)
GMF_DEVINL void neighbour_key(const int* base, int d, int k, int D, int sign_t, int* key) {
  key[0] = base[0];
  int rem = d;
  for (int a = 1; a <= D; ++a) {
    const int off = rem % k - k / 2;
    rem /= k;
    key[a] = base[a] + sign_t * off;
  }
}

// one wave per output row, one lane per offset: the hits of 64 consecutive offsets are ranked by a ballot, so the pairs land
// in ascending offset order
template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_map(const int* __restrict__ out_coords, const int* __restrict__ out_count, int M,
                                                  const int* __restrict__ in_coords, const int* __restrict__ in_table,
                                                  unsigned tmask, int D, int k, int K, int sign_t, int* __restrict__ cnt,
                                                  const int* __restrict__ row_ptr, int2* __restrict__ pairs) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (!kFill && o == 0 && lane == 0) cnt[M] = 0;
  if (o >= M) return;
  if (o >= *out_count) {
    if (!kFill && lane == 0) cnt[o] = 0;
    return;
  }
  int base[kKI], key[kKI];
  for (int c = 0; c < kKI; ++c) base[c] = out_coords[(size_t)o * kKI + c];
  const int nk = D + 1;
  int w = kFill ? row_ptr[o] : 0;
  for (int d0 = 0; d0 < K; d0 += 64) {
    const int d = d0 + lane;
    int r = -1;
    if (d < K) {
      neighbour_key(base, d, k, D, sign_t, key);
      r = table_find(in_coords, in_table, tmask, key, nk);
    }
    const unsigned long long hit = __ballot(r >= 0);
    if (kFill && r >= 0) pairs[w + __popcll(hit & ((1ull << lane) - 1))] = make_int2(d, r);
    w += __popcll(hit);
  }
  if (!kFill && lane == 0) cnt[o] = w;
}

constexpr int kTM = kSparseConvTile, kTN = kSparseConvTile, kTK = 16;

// The fused ReLU of every epilogue here keeps a NaN, as torch.relu and the training GEMM's relu_nan (mfma_core.hpp) do:
// fmaxf(NaN, 0) is 0 and would hand a non-finite row on as a clean zero row.  `<=`, not relu_nan's `<`, so that every other
// value keeps the bits fmaxf gave it: v_max_f32 returns +0 for (-0, +0).
GMF_DEVINL float relu_keep_nan(float v) { return v <= 0.f ? 0.f : v; }

GMF_DEVINL float epilogue(float v, int o, int oc, const SparseConvArgs& a) {
  if (a.scale || a.shift) v = fmaf(v, a.scale ? a.scale[oc] : 1.f, a.shift ? a.shift[oc] : 0.f);
  if (a.residual) v += a.residual[(size_t)o * a.cout + oc];
  if (a.relu) v = relu_keep_nan(v);
  return v;
}

// offset slices (slice_of, slice_begin) and output-row groups: sparse_conv_plan.hpp

// first index j in [lo, hi) with v[j] >= key (v ascending there)
GMF_DEVINL int lower_bound(const int* __restrict__ v, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One workgroup owns (offset slice blockIdx.x, 64 output channels blockIdx.y, output-row group blockIdx.z).  It walks the offsets
// of its slice in ascending order and, for each, the offset-major list of that offset's pairs whose output rows lie in its group
// (ascending row; an output row has at most one pair per offset).  Each 64-pair tile gathers only real input rows, reads W_d
// once for the tile and adds its product into the slice's partial row: written on the row's first offset of the slice, added
// to after that.  Rows are distinct within one offset, so no two threads update one element between two barriers; every
// element's partial is a fixed chain over the slice's offsets in ascending order.  Identity map (row_ptr == nullptr): one offset,
// pair j = row j, the epilogue applied here.
__global__ __launch_bounds__(kThreads) void k_sparse_conv(const SparseConvArgs a) {
  __shared__ __align__(16) float Xs[kTK][kTM];
  __shared__ __align__(16) float Ws[kTK][kTN];
  __shared__ int s_o[kTM], s_i[kTM], s_first[kTM];
  const int n_out = *a.n_out;
  const int split = blockIdx.x, col0 = blockIdx.y * kTN, grp = blockIdx.z;
  const int rlo = sparse_conv_group_begin(n_out, grp, gridDim.z), rhi = sparse_conv_group_begin(n_out, grp + 1, gridDim.z);
  if (rlo >= rhi) return;
  const bool ident = a.row_ptr == nullptr;
  const int d0 = ident ? 0 : slice_begin(split, a.nsplit, a.K), d1 = ident ? 1 : slice_begin(split + 1, a.nsplit, a.K);
  const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  const int cin = a.ca + a.cb;
  const int plo = ident ? 0 : a.row_ptr[rlo], phi = ident ? 0 : a.row_ptr[rhi];
  for (int d = d0; d < d1; ++d) {
    int lo = rlo, hi = rhi;
    if (!ident) {
      const int s0 = a.off_start[d], s1 = a.off_start[d + 1];
      if (s0 == s1) continue;
      lo = lower_bound(a.by_off, s0, s1, plo);
      hi = lower_bound(a.by_off, lo, s1, phi);
    }
    const float* Wd = a.W + (size_t)d * cin * a.cout;
    for (int t0 = lo; t0 < hi; t0 += kTM) {
      __syncthreads();                               // the previous tile is done with s_* and its partial rows are written
      if (tid < kTM) {
        const int j = t0 + tid;
        int o = -1, i = -1, first = 1;
        if (j < hi) {
          if (ident) {
            o = i = j;
          } else {
            const int p = a.by_off[j];
            int l = rlo, h = rhi - 1;                // the row of pair p: the last o with row_ptr[o] <= p
            while (l < h) {
              const int mid = (l + h + 1) >> 1;
              if (a.row_ptr[mid] <= p) l = mid; else h = mid - 1;
            }
            o = l;
            i = a.pairs[p].y;
            first = p == a.row_ptr[o] || slice_of(a.pairs[p - 1].x, a.nsplit, a.K) != split;
          }
        }
        s_o[tid] = o;
        s_i[tid] = i;
        s_first[tid] = first;
      }
      __syncthreads();
      float pd[4][4];                                // this offset's sum: 16-channel chains added in channel order
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) pd[r][c] = 0.f;
      for (int k0 = 0; k0 < cin; k0 += kTK) {
        for (int e = tid; e < kTM * kTK; e += kThreads) {
          const int r = e / kTK, kk = e % kTK, c = k0 + kk, ir = s_i[r];
          float v = 0.f;
          if (ir >= 0 && c < cin) v = c < a.ca ? a.xa[(size_t)ir * a.ca + c] : a.xb[(size_t)ir * a.cb + (c - a.ca)];
          Xs[kk][r] = v;
        }
        for (int e = tid; e < kTK * kTN; e += kThreads) {
          const int kk = e / kTN, cc = e % kTN, c = k0 + kk, oc = col0 + cc;
          Ws[kk][cc] = (c < cin && oc < a.cout) ? Wd[(size_t)c * a.cout + oc] : 0.f;
        }
        __syncthreads();
        float sk[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) sk[r][c] = 0.f;
#pragma unroll
        for (int kk = 0; kk < kTK; ++kk) {
          const float4 xv = *reinterpret_cast<const float4*>(&Xs[kk][tr * 4]);
          const float4 wv = *reinterpret_cast<const float4*>(&Ws[kk][tc * 4]);
          const float x4[4] = {xv.x, xv.y, xv.z, xv.w}, w4[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) sk[r][c] = fmaf(x4[r], w4[c], sk[r][c]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) pd[r][c] += sk[r][c];
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = s_o[tr * 4 + r];
        if (o < 0) continue;
        const bool first = s_first[tr * 4 + r];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int oc = col0 + tc * 4 + c;
          if (oc >= a.cout) continue;
          if (ident) {
            a.y[(size_t)o * a.cout + oc] = epilogue(pd[r][c], o, oc, a);
          } else {
            float* q = a.partial + ((size_t)split * a.cap_out + o) * a.cout + oc;
            *q = first ? pd[r][c] : *q + pd[r][c];
          }
        }
      }
    }
  }
}

// y[o] = epilogue(sum of the row's slice partials in slice order): the slices the row has pairs in, from its CSR list
__global__ __launch_bounds__(kThreads) void k_split_reduce(const SparseConvArgs a) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= a.cap_out * a.cout) return;
  const int o = (int)(e / a.cout), oc = (int)(e % a.cout);
  if (o >= *a.n_out) return;
  float v = 0.f;
  int prev = -1;
  for (int p = a.row_ptr[o], pe = a.row_ptr[o + 1]; p < pe; ++p) {
    const int s = slice_of(a.pairs[p].x, a.nsplit, a.K);
    if (s == prev) continue;
    v += a.partial[((size_t)s * a.cap_out + o) * a.cout + oc];
    prev = s;
  }
  a.y[(size_t)o * a.cout + oc] = epilogue(v, o, oc, a);
}

GMF_DEVINL float narrow_epilogue(float v, int o, int oc, const SparseNarrowArgs& a) {
  if (a.scale || a.shift) v = fmaf(v, a.scale ? a.scale[oc] : 1.f, a.shift ? a.shift[oc] : 0.f);
  if (a.residual) v += a.residual[(size_t)o * a.cout + oc];
  if (a.relu) v = relu_keep_nan(v);
  return v;
}

// Narrow-input convolution.  A group of L lanes (16, 32 or 64: the fewest that cover cout) owns one output row, lane c its
// output channel c; a wave holds 64 / L rows.  The group loads L pairs of its row at once, one per lane (the pair, then the
// input row's cin channels), so a row of ~100 pairs costs two dependent loads per L pairs, and then walks them in ascending
// order, taking each pair's offset and channels from the lane that loaded it (__shfl within the group).  Every element is one
// fma chain over the row's pairs, channels in order inside a pair.  A row belongs to one group whatever the grid, so results
// do not depend on how rows are grouped into workgroups.  kLdsW: W [K][cin][cout] is staged in LDS first.
template <bool kLdsW>
__global__ __launch_bounds__(kThreads) void k_sparse_conv_narrow(const SparseNarrowArgs a) {
  extern __shared__ __align__(16) float narrow_ws[];
  const float* W = a.W;
  if (kLdsW) {
    const int wlen = a.K * a.cin * a.cout;
    for (int e = threadIdx.x; e < wlen; e += kThreads) narrow_ws[e] = a.W[e];
    __syncthreads();
    W = narrow_ws;
  }
  const int L = sparse_narrow_lanes(a.cout);
  const int G = 64 / L;
  const int lane = threadIdx.x & 63, c = lane % L, gbase = lane - c;
  const int cc = c < a.cout ? c : a.cout - 1;        // lanes past cout compute a copy of the last channel and store nothing
  const long long n = *a.n_out < a.cap_out ? *a.n_out : a.cap_out;
  const int waves = gridDim.x * (kThreads / 64);
  for (long long w = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); w * G < n; w += waves) {
    const long long o = w * G + lane / L;
    int pb = 0, pe = 0;
    if (o < n) {
      pb = a.row_ptr[o];
      pe = a.row_ptr[o + 1];
    }
    float acc = 0.f;
    for (int p0 = pb; p0 < pe; p0 += L) {             // uniform within the group: every source lane below is active
      const int p = p0 + c;
      int d = 0;
      float xv[kSparseNarrowMaxCin];
#pragma unroll
      for (int k = 0; k < kSparseNarrowMaxCin; ++k) xv[k] = 0.f;
      if (p < pe) {
        const int2 pr = a.pairs[p];
        d = pr.x;
        const float* xr = a.x + (size_t)pr.y * a.cin;
#pragma unroll
        for (int k = 0; k < kSparseNarrowMaxCin; ++k)
          if (k < a.cin) xv[k] = xr[k];
      }
      const int jn = pe - p0 < L ? pe - p0 : L;
      for (int j = 0; j < jn; ++j) {
        const int dj = __shfl(d, gbase + j);
        const float* wd = W + (size_t)dj * a.cin * a.cout + cc;
#pragma unroll
        for (int k = 0; k < kSparseNarrowMaxCin; ++k)
          if (k < a.cin) acc = fmaf(__shfl(xv[k], gbase + j), wd[k * a.cout], acc);
      }
    }
    if (o < n && c < a.cout) a.y[o * a.cout + c] = narrow_epilogue(acc, (int)o, c, a);
  }
}

// Fused FCGF head, one wave per row.  Lane l holds input channel l of x_a and of x_b; lane c computes hidden channel c as an fma
// chain over the inputs in order (x_a, then x_b), then ReLU; lane j computes output j as an fma chain over the hidden channels in
// order, plus the bias.  The norm is one fma chain over the outputs in order, the same on every lane.  W1 [ca + cb][hid] and W2
// [hid][cout] sit in LDS.
__global__ __launch_bounds__(kThreads) void k_sparse_head_l2(const SparseHeadArgs a) {
  extern __shared__ __align__(16) float head_ws[];
  const int cin = a.ca + a.cb;
  float* W1s = head_ws;
  float* W2s = head_ws + cin * a.hid;
  for (int e = threadIdx.x; e < cin * a.hid; e += kThreads) W1s[e] = a.W1[e];
  for (int e = threadIdx.x; e < a.hid * a.cout; e += kThreads) W2s[e] = a.W2[e];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int ch = lane < a.hid ? lane : a.hid - 1, cy = lane < a.cout ? lane : a.cout - 1;
  const float b = a.bias ? a.bias[cy] : 0.f;
  const long long n = *a.n_out < a.cap_out ? *a.n_out : a.cap_out;
  for (long long o = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); o < n; o += gridDim.x * (kThreads / 64)) {
    const float xa = lane < a.ca ? a.xa[o * a.ca + lane] : 0.f;
    const float xb = lane < a.cb ? a.xb[o * a.cb + lane] : 0.f;
    float h = 0.f;
    for (int k = 0; k < a.ca; ++k) h = fmaf(__shfl(xa, k), W1s[k * a.hid + ch], h);
    for (int k = 0; k < a.cb; ++k) h = fmaf(__shfl(xb, k), W1s[(a.ca + k) * a.hid + ch], h);
    h = relu_keep_nan(h);
    float y = 0.f;
    for (int k = 0; k < a.hid; ++k) y = fmaf(__shfl(h, k), W2s[k * a.cout + cy], y);
    y += b;
    if (a.normalize) {                                // resunet.py: F / (||F||_2 + 1e-8)
      float s = 0.f;
      for (int j = 0; j < a.cout; ++j) {
        const float v = __shfl(y, j);
        s = fmaf(v, v, s);
      }
      y = y / (sqrtf(s) + 1e-8f);
    }
    if (lane < a.cout) a.y[o * a.cout + lane] = y;
  }
}

// offset-major lists: the key of CSR pair j is its offset (K past the last pair, so those sort last), the value j
__global__ __launch_bounds__(kThreads) void k_pair_keys(const int* __restrict__ row_ptr, const int* __restrict__ n_out,
                                                        const int2* __restrict__ pairs, long long total, int K,
                                                        int* __restrict__ keys, int* __restrict__ vals) {
  const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= total) return;
  keys[j] = j < row_ptr[*n_out] ? pairs[j].x : K;
  vals[j] = (int)j;
}

__global__ void k_off_start(const int* __restrict__ keys_sorted, int total, int K, int* __restrict__ off_start) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d <= K) off_start[d] = lower_bound(keys_sorted, 0, total, d);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------

bool sparse_plan_layout(long long M, int D, int levels, int nmaps, const SparseMapDesc* maps, SparsePlanLayout& lay) {
  if (M < 1 || M >= (1LL << 28) || D < 1 || D > kSparseMaxD || levels < 1 || levels > kSparseMaxLevels || nmaps < 0 ||
      nmaps > kSparseMaxMaps)
    return false;
  lay = SparsePlanLayout();
  lay.M = M;
  lay.D = D;
  lay.levels = levels;
  lay.nmaps = nmaps;
  long long T = 64;
  while (T < 2 * M) T *= 2;
  lay.T = T;
  size_t p = 0;
  auto take = [&](size_t bytes) { const size_t o = p; p += a256(bytes); return o; };
  lay.counts = take(16 * 4);
  for (int l = 0; l < levels; ++l) lay.coords[l] = take((size_t)M * kKI * 4);
  for (int l = 0; l < levels; ++l) lay.table[l] = take((size_t)T * 4);
  lay.keys = take((size_t)M * kKI * 4);
  lay.idx_a = take((size_t)M * 4);
  lay.idx_b = take((size_t)M * 4);
  lay.flags = take((size_t)(M + 1) * 4);
  lay.pos = take((size_t)(M + 1) * 4);
  size_t sort_b = 0, scan_b = 0;
  (void)hipcub::DeviceMergeSort::StableSortKeysCopy(nullptr, sort_b, (int*)nullptr, (int*)nullptr, (int)M, KeyLess{nullptr});
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, (int*)nullptr, (int*)nullptr, (int)(M + 1));
  lay.tmp_bytes = sort_b > scan_b ? sort_b : scan_b;
  long long maxK = 1;
  for (int m = 0; m < nmaps; ++m) {
    const SparseMapDesc& d = maps[m];
    if (d.k < 1 || d.k % 2 == 0 || d.out < 0 || d.out >= levels || d.in < 0 || d.in >= levels || d.out - d.in > 1 ||
        d.in - d.out > 1)
      return false;
    long long K = 1;
    for (int a = 0; a < D; ++a) {
      K *= d.k;
      if (K > kSparseMaxK) return false;
    }
    if (M * K >= (1LL << 31)) return false;          // CSR offsets are int32
    lay.maps[m] = d;
    lay.K[m] = (int)K;
    lay.row_ptr[m] = take((size_t)(M + 1) * 4);
    lay.pairs[m] = take((size_t)M * K * 8);
    lay.by_off[m] = take((size_t)M * K * 4);
    lay.off_start[m] = take((size_t)(K + 1) * 4);
    if (K > maxK) maxK = K;
  }
  // the offset sort: keys in / out and values in for M k^D pairs (shared by the maps), its temporary storage
  lay.skeys_a = take((size_t)M * maxK * 4);
  lay.skeys_b = take((size_t)M * maxK * 4);
  lay.svals = take((size_t)M * maxK * 4);
  size_t rsort_b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, rsort_b, (int*)nullptr, (int*)nullptr, (int*)nullptr, (int*)nullptr,
                                           (int)(M * maxK), 0, 11);
  if (rsort_b > lay.tmp_bytes) lay.tmp_bytes = rsort_b;
  lay.tmp = take(lay.tmp_bytes);
  lay.total = p;
  return true;
}

hipError_t launch_sparse_build_plan(const int* coords, const SparsePlanLayout& lay, char* base, int* status, int dup_bit,
                                    hipStream_t s) {
  const int M = (int)lay.M, D = lay.D, nk = D + 1;
  const unsigned tmask = (unsigned)(lay.T - 1);
  int* counts = reinterpret_cast<int*>(base + lay.counts);
  auto lvl = [&](int l) { return reinterpret_cast<int*>(base + lay.coords[l]); };
  auto tab = [&](int l) { return reinterpret_cast<int*>(base + lay.table[l]); };
  int* keys = reinterpret_cast<int*>(base + lay.keys);
  int* idx_a = reinterpret_cast<int*>(base + lay.idx_a);
  int* idx_b = reinterpret_cast<int*>(base + lay.idx_b);
  int* flags = reinterpret_cast<int*>(base + lay.flags);
  int* pos = reinterpret_cast<int*>(base + lay.pos);
  void* tmp = base + lay.tmp;
  hipError_t e = hipMemsetAsync(counts, 0, 16 * 4, s);
  if (e != hipSuccess) return e;
  k_load_level0<<<blocks(M, kThreads), kThreads, 0, s>>>(coords, M, D, lvl(0), counts);
  for (int l = 0; l < lay.levels; ++l) {
    if (l > 0) {
      k_coarse_keys<<<blocks(M, kThreads), kThreads, 0, s>>>(lvl(l - 1), counts + l - 1, M, D, 1 << l, keys, idx_a);
      size_t tb = lay.tmp_bytes;
      e = hipcub::DeviceMergeSort::StableSortKeysCopy(tmp, tb, idx_a, idx_b, M, KeyLess{keys}, s);
      if (e != hipSuccess) return e;
      k_heads<<<blocks(M, kThreads), kThreads, 0, s>>>(keys, idx_b, M, nk, flags);
      tb = lay.tmp_bytes;
      e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, flags, pos, M + 1, s);
      if (e != hipSuccess) return e;
      k_emit<<<blocks(M, kThreads), kThreads, 0, s>>>(keys, idx_b, flags, pos, M, lvl(l), counts + l);
    }
    e = hipMemsetAsync(tab(l), 0xFF, (size_t)lay.T * 4, s);
    if (e != hipSuccess) return e;
    k_insert<<<blocks(M, kThreads), kThreads, 0, s>>>(lvl(l), counts + l, nk, tab(l), tmask, status, l == 0 ? dup_bit : 0);
  }
  for (int m = 0; m < lay.nmaps; ++m) {
    const SparseMapDesc& d = lay.maps[m];
    const int t = 1 << (d.out < d.in ? d.out : d.in);
    const int sign_t = d.out < d.in ? -t : t;
    int* row_ptr = reinterpret_cast<int*>(base + lay.row_ptr[m]);
    int2* pairs = reinterpret_cast<int2*>(base + lay.pairs[m]);
    k_map<false><<<blocks(M, kThreads / 64), kThreads, 0, s>>>(lvl(d.out), counts + d.out, M, lvl(d.in), tab(d.in), tmask, D, d.k,
                                                          lay.K[m], sign_t, flags, nullptr, nullptr);
    size_t tb = lay.tmp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, flags, row_ptr, M + 1, s);
    if (e != hipSuccess) return e;
    k_map<true><<<blocks(M, kThreads / 64), kThreads, 0, s>>>(lvl(d.out), counts + d.out, M, lvl(d.in), tab(d.in), tmask, D, d.k,
                                                         lay.K[m], sign_t, nullptr, row_ptr, pairs);
    // offset-major list: the CSR pair indices stably sorted by offset (ascending output row within an offset)
    const long long total = (long long)M * lay.K[m];
    int* ka = reinterpret_cast<int*>(base + lay.skeys_a);
    int* kb = reinterpret_cast<int*>(base + lay.skeys_b);
    int* va = reinterpret_cast<int*>(base + lay.svals);
    int* by_off = reinterpret_cast<int*>(base + lay.by_off[m]);
    k_pair_keys<<<blocks(total, kThreads), kThreads, 0, s>>>(row_ptr, counts + d.out, pairs, total, lay.K[m], ka, va);
    tb = lay.tmp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(tmp, tb, ka, kb, va, by_off, (int)total, 0, 11, s);
    if (e != hipSuccess) return e;
    k_off_start<<<blocks(lay.K[m] + 1, kThreads), kThreads, 0, s>>>(kb, (int)total, lay.K[m],
                                                                      reinterpret_cast<int*>(base + lay.off_start[m]));
  }
  return hipGetLastError();
}

hipError_t launch_sparse_conv(const SparseConvArgs& a, hipStream_t s) {
  dim3 grid(a.nsplit, blocks(a.cout, kTN), sparse_conv_row_groups(a.K, a.ca + a.cb, a.cout, a.nsplit, a.cap_out));
  k_sparse_conv<<<grid, kThreads, 0, s>>>(a);
  if (a.row_ptr) k_split_reduce<<<blocks(a.cap_out * a.cout, kThreads), kThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_sparse_conv_narrow(const SparseNarrowArgs& a, hipStream_t s) {
  // the grid (sparse_narrow_grid) never changes a result: a row belongs to one lane group whatever the grid
  const int g = sparse_narrow_grid(a.cap_out, a.K, a.cin, a.cout);
  if (sparse_narrow_lds(a.K, a.cin, a.cout))
    k_sparse_conv_narrow<true><<<g, kThreads, (size_t)a.K * a.cin * a.cout * sizeof(float), s>>>(a);
  else
    k_sparse_conv_narrow<false><<<g, kThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_sparse_head_l2(const SparseHeadArgs& a, hipStream_t s) {
  const size_t lds = (size_t)((a.ca + a.cb) * a.hid + a.hid * a.cout) * sizeof(float);
  k_sparse_head_l2<<<sparse_head_grid(a.cap_out), kThreads, lds, s>>>(a);
  return hipGetLastError();
}

}  // namespace gmf
