// RGB-D odometry: open3d 0.9's compute_rgbd_odometry with RGBDOdometryJacobianFromHybridTerm as the reference's
// make_fragments.py drives it, for E frame pairs over F frames whose pyramids are built once.  The contract is DESIGN.md section
// 4p and its numpy restatement tests/rgbd_reference.py; this file is built with -ffp-contract=off: the planes and the
// correspondence maps equal that restatement exactly, the sums differ from it by their order alone.
//
//   preparation  stencil launches over all frames: convert, Gaussian, four Sobel planes per level in one launch, 2 x 2 mean
//   iteration    three launches for all pairs (the pair in blockIdx.y):
//     scatter    one thread per source pixel, one 64-bit atomicMin on (float bits of d_s) << 32 | source pixel per candidate
//     walk       one workgroup per 2048 target pixels: reads the map (and resets it for the next scatter), forms the two
//                Jacobian rows, sums 28 numbers per thread, then a fixed tree (xor shuffles, four waves in order) to one partial
//     finish     one wave per pair: the partials in index order, the 6 x 6 solve, T <- M(x) T
//   the normalisation scales and the information matrix are the same three launches with other sums.
#include <hip/hip_runtime.h>
#include <math.h>

#include "launchers_rgbd.hpp"

#define RGBD_DEVINL __device__ __forceinline__

namespace gmf {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = kRgbdChunk / kThreads;
constexpr unsigned long long kNone = ~0ull;
constexpr int kCountSlot = kRgbdSlots - 1;

enum WalkMode { kWalkNorm = 0, kWalkJacobian = 1, kWalkInformation = 2 };

int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

struct Taps { double x0, x1, x2, y0, y1, y2; };
constexpr Taps kGauss{0.25, 0.5, 0.25, 0.25, 0.5, 0.25};
constexpr Taps kSobelX{-1.0, 0.0, 1.0, 1.0, 2.0, 1.0};
constexpr Taps kSobelY{1.0, 2.0, 1.0, -1.0, 0.0, 1.0};

// the part of a level every odometry kernel needs
struct LevelView {
  const float* base;          // [F,6,h,w]
  int h, w, F;
  double fx, fy, cx, cy;      // the level's intrinsics
};

// ---- preparation --------------------------------------------------------------------------------------------------------------

// steps 1 and the intensity: raw_i, raw_d [F,H,W]
__global__ __launch_bounds__(kThreads) void k_rgbd_convert(const void* __restrict__ color, int kind, const void* __restrict__ depth,
                                                           bool u16, long long n, float scale, float trunc, float dmin, float dmax,
                                                           float* __restrict__ raw_i, float* __restrict__ raw_d) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float v;
  if (kind == kRgbdGray8) {
    v = (float)static_cast<const unsigned char*>(color)[i] / 255.f;
  } else if (kind == kRgbdRgb8) {
    const unsigned char* c = static_cast<const unsigned char*>(color) + 3 * i;
    v = ((0.2990f * (float)c[0] + 0.5870f * (float)c[1]) + 0.1140f * (float)c[2]) / 255.f;
  } else {
    v = static_cast<const float*>(color)[i];
  }
  raw_i[i] = v;
  float d;
  if (u16) {
    d = (float)static_cast<const unsigned short*>(depth)[i] / scale;
  } else {
    d = static_cast<const float*>(depth)[i];
    if (!(d >= 0.f) || isinf(d)) d = 0.f;
  }
  if (d >= trunc) d = 0.f;
  if (d < dmin || d > dmax || d <= 0.f) d = __builtin_nanf("");
  raw_d[i] = d;
}

// Filter(kx, ky) at one pixel: the horizontal pass of the three rows (each rounded to float32), then the vertical one
RGBD_DEVINL float filter_at(const float* __restrict__ in, int h, int w, int r, int c, const Taps& k) {
  const int c0 = c > 0 ? c - 1 : 0, c2 = c < w - 1 ? c + 1 : w - 1;
  const int r0 = r > 0 ? r - 1 : 0, r2 = r < h - 1 ? r + 1 : h - 1;
  const int rows[3] = {r0, r, r2};
  const double ky[3] = {k.y0, k.y1, k.y2};
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float* row = in + (size_t)rows[j] * w;
    double hacc = 0.0;
    hacc = hacc + k.x0 * (double)row[c0];
    hacc = hacc + k.x1 * (double)row[c];
    hacc = hacc + k.x2 * (double)row[c2];
    const float hv = (float)hacc;
    acc = acc + ky[j] * (double)hv;
  }
  return (float)acc;
}

// `planes` images of h x w, image p at in + p * in_stride -> out + p * out_stride
__global__ __launch_bounds__(kThreads) void k_rgbd_filter(const float* __restrict__ in, size_t in_stride, float* __restrict__ out,
                                                          size_t out_stride, int planes, int h, int w, Taps k) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long hw = (long long)h * w;
  if (i >= planes * hw) return;
  const int p = (int)(i / hw), q = (int)(i % hw);
  out[p * out_stride + q] = filter_at(in + p * in_stride, h, w, q / w, q % w, k);
}

// the four gradient planes of one level [F,6,h,w]: blockIdx.y = 0..3 -> Idx, Idy, Ddx, Ddy
__global__ __launch_bounds__(kThreads) void k_rgbd_sobel(float* __restrict__ level, int F, int h, int w) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long hw = (long long)h * w;
  if (i >= F * hw) return;
  const int which = blockIdx.y;
  const int f = (int)(i / hw), q = (int)(i % hw);
  float* frame = level + (size_t)f * kRgbdPlanes * hw;
  frame[(size_t)(2 + which) * hw + q] = filter_at(frame + (size_t)(which >> 1) * hw, h, w, q / w, q % w, (which & 1) ? kSobelY : kSobelX);
}

// Down: h x w -> floor(h/2) x floor(w/2)
__global__ __launch_bounds__(kThreads) void k_rgbd_down(const float* __restrict__ in, size_t in_stride, int w_in, float* __restrict__ out,
                                                        size_t out_stride, int planes, int h, int w) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long hw = (long long)h * w;
  if (i >= planes * hw) return;
  const int p = (int)(i / hw), q = (int)(i % hw);
  const int r = q / w, c = q % w;
  const float* a = in + p * in_stride + (size_t)(2 * r) * w_in + 2 * c;
  out[p * out_stride + q] = (((a[0] + a[1]) + a[w_in]) + a[w_in + 1]) / 4.f;
}

// ---- the pairs ----------------------------------------------------------------------------------------------------------------

// T = the first three rows of odo_init over (0, 0, 0, 1), or I; a pair that names no frame fails at once
__global__ void k_rgbd_begin(const int* __restrict__ pair_src, const int* __restrict__ pair_tgt, int E, int F,
                             const double* __restrict__ init, double* __restrict__ pose, int* __restrict__ failed) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int s = pair_src[e], t = pair_tgt[e];
  bool bad = s < 0 || s >= F || t < 0 || t >= F;
  for (int j = 0; j < 16; ++j) {
    const double v = init && j < 12 ? init[(size_t)e * 16 + j] : ((j % 5) == 0 ? 1.0 : 0.0);
    if (!isfinite(v)) bad = true;
    pose[(size_t)e * 16 + j] = v;
  }
  failed[e] = bad ? 1 : 0;
}

// step 4: candidates into the map
__global__ __launch_bounds__(kThreads) void k_rgbd_scatter(LevelView L, const int* __restrict__ pair_src, const int* __restrict__ pair_tgt,
                                                           const double* __restrict__ pose, const int* __restrict__ failed,
                                                           double max_depth_diff, unsigned long long* __restrict__ map) {
  const int e = blockIdx.y;
  if (failed[e]) return;
  __shared__ double g[12];                    // M = K R K^-1 (rows), k = K t
  if (threadIdx.x == 0) {
    const double* T = pose + (size_t)e * 16;
    double KR[3][3];
    for (int j = 0; j < 3; ++j) {
      KR[0][j] = L.fx * T[j] + L.cx * T[8 + j];
      KR[1][j] = L.fy * T[4 + j] + L.cy * T[8 + j];
      KR[2][j] = T[8 + j];
    }
    for (int i = 0; i < 3; ++i) {
      const double m0 = KR[i][0] / L.fx, m1 = KR[i][1] / L.fy;
      g[3 * i] = m0;
      g[3 * i + 1] = m1;
      g[3 * i + 2] = KR[i][2] - (m0 * L.cx + m1 * L.cy);
    }
    g[9] = L.fx * T[3] + L.cx * T[11];
    g[10] = L.fy * T[7] + L.cy * T[11];
    g[11] = T[11];
  }
  __syncthreads();
  const int hw = L.h * L.w;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= hw) return;
  const size_t frame = (size_t)kRgbdPlanes * hw;
  const float ds = L.base[pair_src[e] * frame + hw + i];
  if (isnan(ds)) return;
  const double us = (double)(i % L.w), vs = (double)(i / L.w), d = (double)ds;
  const double p0 = d * ((g[0] * us + g[1] * vs) + g[2]) + g[9];
  const double p1 = d * ((g[3] * us + g[4] * vs) + g[5]) + g[10];
  const double z = d * ((g[6] * us + g[7] * vs) + g[8]) + g[11];
  const double fu = p0 / z + 0.5, fv = p1 / z + 0.5;
  if (!(fabs(fu) < 1073741824.0 && fabs(fv) < 1073741824.0)) return;      // also the non-finite ones
  const int ut = (int)fu, vt = (int)fv;                                     // toward zero: (-1, 0) lands on 0
  if (ut < 0 || ut >= L.w || vt < 0 || vt >= L.h) return;
  const int t = vt * L.w + ut;
  const float dt = L.base[pair_tgt[e] * frame + hw + t];
  if (isnan(dt)) return;
  if (!(fabs(z - (double)dt) <= max_depth_diff)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(ds) << 32) | (unsigned int)i;
  atomicMin(&map[(size_t)e * hw + t], key);
}

// map -> [E,h,w] int32 (and the map is reset)
__global__ __launch_bounds__(kThreads) void k_rgbd_map_out(unsigned long long* __restrict__ map, long long n, int* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = map[i];
  out[i] = key == kNone ? -1 : (int)(unsigned int)key;
  if (key != kNone) map[i] = kNone;
}

// the 21 + 6 + 1 sums of one row: A's upper triangle row by row, b, r2
RGBD_DEVINL void add_row(double (&acc)[28], const double (&J)[6], double r) {
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = a; b < 6; ++b) acc[k++] += J[a] * J[b];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
  acc[27] += r * r;
}

// steps 5, 6 and 7: the sums over the correspondences of one chunk of target pixels
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_rgbd_walk(LevelView L, const int* __restrict__ pair_src, const int* __restrict__ pair_tgt,
                                                        const double* __restrict__ pose, const double* __restrict__ scale,
                                                        const int* __restrict__ failed, unsigned long long* __restrict__ map,
                                                        double* __restrict__ partial) {
  constexpr int NS = MODE == kWalkNorm ? 2 : MODE == kWalkJacobian ? 28 : 21;
  const int e = blockIdx.y;
  if (failed[e]) return;
  const int hw = L.h * L.w;
  const size_t frame = (size_t)kRgbdPlanes * hw;
  const float* S = L.base + pair_src[e] * frame;
  const float* Tg = L.base + pair_tgt[e] * frame;
  double T[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) T[j] = pose[(size_t)e * 16 + j];
  double s_src = 1.0, s_tgt = 1.0;
  if (MODE == kWalkJacobian) {
    s_src = scale[2 * e];
    s_tgt = scale[2 * e + 1];
  }
  const double sl_img = sqrt(1.0 - 0.968), sl_dep = sqrt(0.968);
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  int n = 0;
  unsigned long long* m = map + (size_t)e * hw;
  for (int j = 0; j < kPerThread; ++j) {
    const int i = blockIdx.x * kRgbdChunk + j * kThreads + threadIdx.x;
    if (i >= hw) break;
    const unsigned long long key = m[i];
    if (key == kNone) continue;
    m[i] = kNone;
    const int src = (int)(unsigned int)key;
    ++n;
    if (MODE == kWalkNorm) {
      acc[0] += (double)S[src];
      acc[1] += (double)Tg[i];
      continue;
    }
    const double z = (double)S[hw + src];
    const double x = (double)(float)((((double)(src % L.w) - L.cx) * z) / L.fx);
    const double y = (double)(float)((((double)(src / L.w) - L.cy) * z) / L.fy);
    if (MODE == kWalkInformation) {
      const double r0[6] = {0.0, z, -y, 1.0, 0.0, 0.0}, r1[6] = {-z, 0.0, x, 0.0, 1.0, 0.0}, r2[6] = {y, -x, 0.0, 0.0, 0.0, 1.0};
      add_row(acc, r0, 0.0);
      add_row(acc, r1, 0.0);
      add_row(acc, r2, 0.0);
      continue;
    }
    const double p0 = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    const double p1 = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    const double p2 = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    const double diff_photo = s_tgt * (double)Tg[i] - s_src * (double)S[src];
    const double dIdx = 0.125 * (s_tgt * (double)Tg[2 * (size_t)hw + i]), dIdy = 0.125 * (s_tgt * (double)Tg[3 * (size_t)hw + i]);
    double dDdx = 0.125 * (double)Tg[4 * (size_t)hw + i], dDdy = 0.125 * (double)Tg[5 * (size_t)hw + i];
    if (isnan(dDdx)) dDdx = 0.0;
    if (isnan(dDdy)) dDdy = 0.0;
    const double diff_geo = (double)Tg[hw + i] - p2;
    const double invz = 1.0 / p2;
    const double c0 = (dIdx * L.fx) * invz, c1 = (dIdy * L.fy) * invz;
    const double c2 = -(c0 * p0 + c1 * p1) * invz;
    const double d0 = (dDdx * L.fx) * invz, d1 = (dDdy * L.fy) * invz;
    const double d2 = -(d0 * p0 + d1 * p1) * invz;
    const double Ji[6] = {sl_img * (-p2 * c1 + p1 * c2), sl_img * (p2 * c0 - p0 * c2), sl_img * (-p1 * c0 + p0 * c1),
                          sl_img * c0, sl_img * c1, sl_img * c2};
    const double Jd[6] = {sl_dep * ((-p2 * d1 + p1 * d2) - p1), sl_dep * ((p2 * d0 - p0 * d2) + p0), sl_dep * (-p1 * d0 + p0 * d1),
                          sl_dep * d0, sl_dep * d1, sl_dep * (d2 - 1.0)};
    add_row(acc, Ji, sl_img * diff_photo);
    add_row(acc, Jd, sl_dep * diff_geo);
  }
  // a fixed tree: xor shuffles inside the wave, then the four waves in order
  __shared__ double red[kWaves][kRgbdSlots];
  if (threadIdx.x < kWaves * kRgbdSlots) (&red[0][0])[threadIdx.x] = 0.0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][k] = v;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off, 64);
  if (lane == 0) red[wave][kCountSlot] = (double)n;
  __syncthreads();
  if (threadIdx.x < kRgbdSlots) {
    double v = red[0][threadIdx.x];
    for (int wv = 1; wv < kWaves; ++wv) v += red[wv][threadIdx.x];
    partial[((size_t)e * gridDim.x + blockIdx.x) * kRgbdSlots + threadIdx.x] = v;
  }
}

// A x = rhs by Gaussian elimination with partial pivoting, every index static (the rows stay in registers).  Returns det A; x is
// only meaningful when that is not 0.
RGBD_DEVINL double solve6(double (&a)[6][7], double (&x)[6]) {
  double det = 1.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
      if (fabs(a[r][k]) > fabs(a[k][k])) {
#pragma unroll
        for (int c = 0; c < 7; ++c) {
          const double t = a[k][c];
          a[k][c] = a[r][c];
          a[r][c] = t;
        }
        det = -det;
      }
    }
    const double piv = a[k][k];
    det *= piv;
    const double inv = piv != 0.0 ? 1.0 / piv : 0.0;
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
      const double f = a[r][k] * inv;
#pragma unroll
      for (int c = k; c < 7; ++c) a[r][c] -= f * a[k][c];
    }
  }
#pragma unroll
  for (int k = 5; k >= 0; --k) {
    double v = a[k][6];
#pragma unroll
    for (int c = k + 1; c < 6; ++c) v -= a[k][c] * x[c];
    x[k] = a[k][k] != 0.0 ? v / a[k][k] : 0.0;
  }
  return det;
}

// the partials of a pair in index order, then what the mode does with the sums
template <int MODE>
__global__ __launch_bounds__(64) void k_rgbd_finish(int nblk, const double* __restrict__ partial, double* __restrict__ pose,
                                                    double* __restrict__ scale, int* __restrict__ failed, int iteration, int total,
                                                    int e0, unsigned char* __restrict__ success, double* __restrict__ T_out,
                                                    double* __restrict__ info_out, double* __restrict__ scales_out,
                                                    int* __restrict__ trace_n, double* __restrict__ trace) {
  const int e = blockIdx.x;             // within the chunk; e0 + e in the call's outputs
  const size_t eo = (size_t)e0 + e;
  __shared__ double sum[kRgbdSlots];
  const bool dead = failed[e] != 0;
  if (!dead && threadIdx.x < kRgbdSlots) {
    double v = 0.0;
    for (int b = 0; b < nblk; ++b) v += partial[((size_t)e * nblk + b) * kRgbdSlots + threadIdx.x];
    sum[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* T = pose + (size_t)e * 16;
  if (MODE == kWalkNorm) {
    if (dead) return;
    const double n = sum[kCountSlot];
    const double ss = 0.5 / (sum[0] / n), st = 0.5 / (sum[1] / n);
    if (!(n > 0.0) || !isfinite(ss) || !isfinite(st)) {
      failed[e] = 1;
      return;
    }
    scale[2 * e] = ss;
    scale[2 * e + 1] = st;
    if (scales_out) {
      scales_out[2 * eo] = ss;
      scales_out[2 * eo + 1] = st;
    }
    return;
  }
  if (MODE == kWalkInformation) {
    success[eo] = dead ? 0 : 1;
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b, ++k) {
        const double v = dead ? (a == b ? 1.0 : 0.0) : sum[k];
        info_out[eo * 36 + a * 6 + b] = v;
        info_out[eo * 36 + b * 6 + a] = v;
      }
    for (int j = 0; j < 16; ++j) T_out[eo * 16 + j] = dead ? ((j % 5) == 0 ? 1.0 : 0.0) : T[j];
    return;
  }
  if (dead) return;
  double a[6][7], x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool finite = isfinite(sum[27]);
  {
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
      for (int c = r; c < 6; ++c, ++k) {
        a[r][c] = sum[k];
        a[c][r] = sum[k];
        finite = finite && isfinite(sum[k]);
      }
      a[r][6] = -sum[21 + r];
      finite = finite && isfinite(sum[21 + r]);
    }
  }
  double* tr = trace ? trace + (eo * total + iteration) * kRgbdTrace : nullptr;
  if (tr) {
    trace_n[eo * total + iteration] = (int)sum[kCountSlot];
    for (int r = 0; r < 6; ++r) {
      for (int c = 0; c < 6; ++c) tr[r * 6 + c] = a[r][c];
      tr[36 + r] = sum[21 + r];
    }
    tr[42] = sum[27];
  }
  const double det = finite ? solve6(a, x) : 0.0;
  bool ok = finite && fabs(det) >= 1e-6;
#pragma unroll
  for (int r = 0; r < 6; ++r) ok = ok && isfinite(x[r]);
  if (!ok) {
    failed[e] = 1;
    return;
  }
  const double cx = cos(x[0]), sx = sin(x[0]), cy = cos(x[1]), sy = sin(x[1]), cz = cos(x[2]), sz = sin(x[2]);
  const double M[3][3] = {{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx},
                          {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx},
                          {-sy, cy * sx, cy * cx}};
  double Tn[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double v = (M[i][0] * T[j] + M[i][1] * T[4 + j]) + M[i][2] * T[8 + j];
      if (j == 3) v += x[3 + i];
      Tn[4 * i + j] = v;
    }
  for (int j = 0; j < 12; ++j) T[j] = Tn[j];
  if (tr) {
    for (int r = 0; r < 6; ++r) tr[43 + r] = x[r];
    for (int j = 0; j < 16; ++j) tr[49 + j] = T[j];
  }
}

LevelView view(const float* planes, const RgbdShape& s, int l, const RgbdCamera& K) {
  const double f = ldexp(1.0, -l);
  return LevelView{planes + s.offset(l), s.h(l), s.w(l), s.F, K.fx * f, K.fy * f, K.cx * f, K.cy * f};
}

}  // namespace

hipError_t launch_rgbd_pyramids(const void* color, int color_kind, const void* depth, bool depth_u16, const RgbdShape& s,
                                float depth_scale, float depth_trunc, float min_depth, float max_depth,
                                const RgbdPyramidScratch& ws, float* planes, hipStream_t st) {
  const long long n = (long long)s.F * s.H * s.W;
  k_rgbd_convert<<<blocks(n, kThreads), kThreads, 0, st>>>(color, color_kind, depth, depth_u16, n, depth_scale, depth_trunc, min_depth,
                                                           max_depth, ws.raw_i, ws.raw_d);
  const size_t hw0 = s.pixels(0);
  k_rgbd_filter<<<blocks(n, kThreads), kThreads, 0, st>>>(ws.raw_i, hw0, planes, kRgbdPlanes * hw0, s.F, s.H, s.W, kGauss);
  k_rgbd_filter<<<blocks(n, kThreads), kThreads, 0, st>>>(ws.raw_d, hw0, planes + hw0, kRgbdPlanes * hw0, s.F, s.H, s.W, kGauss);
  for (int l = 0; l < s.levels; ++l) {
    float* level = planes + s.offset(l);
    const size_t hw = s.pixels(l);
    const long long nl = (long long)s.F * hw;
    k_rgbd_sobel<<<dim3(blocks(nl, kThreads), 4), kThreads, 0, st>>>(level, s.F, s.h(l), s.w(l));
    if (l + 1 == s.levels) break;
    float* next = planes + s.offset(l + 1);
    const size_t hw1 = s.pixels(l + 1);
    const long long n1 = (long long)s.F * hw1;
    k_rgbd_filter<<<blocks(nl, kThreads), kThreads, 0, st>>>(level, kRgbdPlanes * hw, ws.raw_i, hw, s.F, s.h(l), s.w(l), kGauss);
    k_rgbd_down<<<blocks(n1, kThreads), kThreads, 0, st>>>(ws.raw_i, hw, s.w(l), next, kRgbdPlanes * hw1, s.F, s.h(l + 1), s.w(l + 1));
    k_rgbd_down<<<blocks(n1, kThreads), kThreads, 0, st>>>(level + hw, kRgbdPlanes * hw, s.w(l), next + hw1, kRgbdPlanes * hw1, s.F,
                                                           s.h(l + 1), s.w(l + 1));
  }
  return hipGetLastError();
}

hipError_t launch_rgbd_correspondences(const float* planes, const RgbdShape& s, int level, const int* pair_src, const int* pair_tgt, int E,
                                       const double* transformation, const RgbdCamera& K, double max_depth_diff,
                                       const RgbdOdometryScratch& ws, int* map_out, hipStream_t st) {
  const int chunk = rgbd_pair_chunk(s, E);
  const LevelView L = view(planes, s, level, K);
  const size_t hw = s.pixels(level);
  for (int e0 = 0; e0 < E; e0 += chunk) {
    const int Ec = E - e0 < chunk ? E - e0 : chunk;
    hipError_t err = hipMemsetAsync(ws.map, 0xff, (size_t)Ec * hw * 8, st);
    if (err != hipSuccess) return err;
    k_rgbd_begin<<<blocks(Ec, 64), 64, 0, st>>>(pair_src + e0, pair_tgt + e0, Ec, s.F, transformation + (size_t)e0 * 16, ws.pose, ws.failed);
    k_rgbd_scatter<<<dim3(blocks((long long)hw, kThreads), Ec), kThreads, 0, st>>>(L, pair_src + e0, pair_tgt + e0, ws.pose, ws.failed,
                                                                                   max_depth_diff, ws.map);
    k_rgbd_map_out<<<blocks((long long)Ec * hw, kThreads), kThreads, 0, st>>>(ws.map, (long long)Ec * hw, map_out + (size_t)e0 * hw);
  }
  return hipGetLastError();
}

hipError_t launch_rgbd_odometry(const float* planes, const RgbdShape& s, const int* pair_src, const int* pair_tgt, int E,
                                const double* odo_init, const RgbdCamera& K, double max_depth_diff, const int* iterations,
                                const RgbdOdometryScratch& ws, unsigned char* success, double* transformation, double* information,
                                double* scales, int* trace_n, double* trace, hipStream_t st) {
  const int chunk = rgbd_pair_chunk(s, E);
  int total = 0;
  for (int l = 0; l < s.levels; ++l) total += iterations[l];
  for (int e0 = 0; e0 < E; e0 += chunk) {
    const int Ec = E - e0 < chunk ? E - e0 : chunk;
    const int* ps = pair_src + e0;
    const int* pt = pair_tgt + e0;
    // every consumed entry is reset by its consumer, so one fill serves the whole run of the chunk
    hipError_t err = hipMemsetAsync(ws.map, 0xff, (size_t)Ec * s.pixels(0) * 8, st);
    if (err != hipSuccess) return err;
    k_rgbd_begin<<<blocks(Ec, 64), 64, 0, st>>>(ps, pt, Ec, s.F, odo_init ? odo_init + (size_t)e0 * 16 : nullptr, ws.pose, ws.failed);
    auto scatter = [&](const LevelView& L) {
      k_rgbd_scatter<<<dim3(blocks((long long)L.h * L.w, kThreads), Ec), kThreads, 0, st>>>(L, ps, pt, ws.pose, ws.failed, max_depth_diff,
                                                                                            ws.map);
    };
    const LevelView L0 = view(planes, s, 0, K);
    const int nblk0 = rgbd_walk_blocks(s.pixels(0));
    scatter(L0);
    k_rgbd_walk<kWalkNorm><<<dim3(nblk0, Ec), kThreads, 0, st>>>(L0, ps, pt, ws.pose, ws.scale, ws.failed, ws.map, ws.partial);
    k_rgbd_finish<kWalkNorm><<<Ec, 64, 0, st>>>(nblk0, ws.partial, ws.pose, ws.scale, ws.failed, 0, total, e0, success, transformation,
                                                information, scales, trace_n, trace);
    int it = 0;
    for (int l = s.levels - 1; l >= 0; --l) {
      const LevelView L = view(planes, s, l, K);
      const int nblk = rgbd_walk_blocks(s.pixels(l));
      for (int i = 0; i < iterations[s.levels - 1 - l]; ++i, ++it) {
        scatter(L);
        k_rgbd_walk<kWalkJacobian><<<dim3(nblk, Ec), kThreads, 0, st>>>(L, ps, pt, ws.pose, ws.scale, ws.failed, ws.map, ws.partial);
        k_rgbd_finish<kWalkJacobian><<<Ec, 64, 0, st>>>(nblk, ws.partial, ws.pose, ws.scale, ws.failed, it, total, e0, success,
                                                        transformation, information, scales, trace_n, trace);
      }
    }
    scatter(L0);
    k_rgbd_walk<kWalkInformation><<<dim3(nblk0, Ec), kThreads, 0, st>>>(L0, ps, pt, ws.pose, ws.scale, ws.failed, ws.map, ws.partial);
    k_rgbd_finish<kWalkInformation><<<Ec, 64, 0, st>>>(nblk0, ws.partial, ws.pose, ws.scale, ws.failed, 0, total, e0, success,
                                                       transformation, information, scales, trace_n, trace);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipGetLastError();
}

}  // namespace gmf
