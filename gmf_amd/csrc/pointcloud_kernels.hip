// Point-cloud descriptors, batched over ragged clouds: the radius-bounded kNN search, normals, FPFH and the two voxel grids that
// the reference runs through open3d / MinkowskiEngine on the CPU before matching (GMF_DeepGlobalRegistration/*/core/
// deep_global_registration.py:143-193; GMF_PointDSC/misc/cal_fpfh.py:202-215).  Contract: gmf_amd/features.py.
//
// Radius search, four launches after one memset, no host synchronisation (graph-capturable for a fixed N):
//   k_grid_count     each row's cell (edge r (1 + 2^-10), so a neighbour within r lies in one of the 27 cells around the
//                    query's) hashed with its cloud into a table of T = pow2 >= 2N slots; rows per slot by integer atomics.
//   (hipcub scan)    slot starts.
//   k_grid_scatter   the rows in slot order (the order inside a slot is arrival order: nothing downstream depends on it).
//   k_knn_search     one wave per query: the 27 cells' distinct slots; a hash collision only adds candidates, which the cloud
//                    and distance tests drop.  d^2 is fp64 from the fp32 coordinates, (dx dx + dy dy) + dz dz, no contraction;
//                    in radius: d^2 < r^2.  Candidates in radius <= max_nn: all are kept.  More: a radix select over the
//                    96-bit key (d^2 bits, row) - 8-bit digits, an LDS histogram per pass, stopping as soon as the chosen bin
//                    holds exactly the keys still needed - finds the max_nn-th key, and the keys <= it are kept.  No
//                    candidate buffer, so no count of candidates drops a row.  The survivors are bitonic-sorted by key in LDS.
// Normals, one thread per row: fp64 cumulants over the neighbour list in key order, open3d's covariance, Eberly's 3x3 solver.
// FPFH, two launches: k_spfh (one wave per row, one lane per neighbour, pair features in fp64, integer bin counts in LDS) and
//   k_fpfh (one wave per row, one lane per bin, the neighbours in key order).  Every sum has a fixed order: bitwise repeatable.
// Voxel grids: the voxel of each row goes into an open-addressing table (atomicCAS on a row, equality by recomputing the
//   occupant's voxel), atomicMin gives each voxel its smallest row, a scan of the "smallest row" flags numbers the voxels in
//   first-occurrence order; for the mean, a radix sort of the unique keys (voxel id << 32 | row) lists each voxel's rows in
//   ascending order.  The caller reads back one voxel count and a range flag.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <limits.h>

#include "grid_hash.hpp"
#include "launchers_pointcloud.hpp"

#pragma clang fp contract(off)

#define GMF_DEVINL __device__ __forceinline__

namespace gmf {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

long long table_slots(long long N) {
  long long T = 64;
  while (T < 2 * N) T <<= 1;
  return T;
}

GMF_DEVINL void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the cloud of row i: the largest b with off[b] <= i
GMF_DEVINL int cloud_of(const int* __restrict__ off, int B, int i) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

GMF_DEVINL double dist2(float4 c, float qx, float qy, float qz) {
  const double dx = (double)c.x - (double)qx, dy = (double)c.y - (double)qy, dz = (double)c.z - (double)qz;
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// ---------------------------------------------------------------------------------------------------------------------------
// radius search
// ---------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_grid_count(const float* __restrict__ pts, const int* __restrict__ off, int B, int N,
                                                         unsigned long long tmask, double inv_h, int* __restrict__ slot,
                                                         int* __restrict__ cnt) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int b = cloud_of(off, B, i);
  const int s = (int)(cell_hash(b, grid_coord(pts[3 * i], inv_h), grid_coord(pts[3 * i + 1], inv_h),
                                grid_coord(pts[3 * i + 2], inv_h)) & tmask);
  slot[i] = s;
  atomicAdd(&cnt[s], 1);
}

__global__ __launch_bounds__(kThreads) void k_grid_scatter(const float* __restrict__ pts, int N, const int* __restrict__ slot,
                                                           const int* __restrict__ start, int* __restrict__ cnt,
                                                           float4* __restrict__ cell_pts) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int s = slot[i];
  const int pos = start[s] + atomicSub(&cnt[s], 1) - 1;
  cell_pts[pos] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], __int_as_float(i));
}

// calls f(in, row, d2) once per candidate of the query's distinct cells, on every lane of the wave (uniform trip count)
template <typename F>
GMF_DEVINL void scan_cells(const int* s_slot, unsigned long long keep, const int* __restrict__ start,
                           const float4* __restrict__ cell_pts, int lo, int hi, float qx, float qy, float qz, double r2, F&& f) {
  const int lane = threadIdx.x & 63;
  for (unsigned long long m = keep; m; m &= m - 1) {
    const int s = s_slot[__builtin_ctzll(m)];
    const int a = start[s], e = start[s + 1];
    for (int base = a; base < e; base += 64) {
      const int p = base + lane;
      bool in = false;
      int j = 0;
      double d = 0.0;
      if (p < e) {
        const float4 c = cell_pts[p];
        j = __float_as_int(c.w);
        if (j >= lo && j < hi) {
          d = dist2(c, qx, qy, qz);
          in = d < r2;
        }
      }
      f(in, j, d);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_knn_search(const float* __restrict__ pts, const int* __restrict__ off, int B, int N,
                                                         unsigned long long tmask, double inv_h, double r2, int max_nn,
                                                         const int* __restrict__ start, const float4* __restrict__ cell_pts,
                                                         int* __restrict__ idx, double* __restrict__ d2o, int* __restrict__ cnt_out) {
  __shared__ int s_slot[kWaves][32];
  __shared__ int s_hist[kWaves][256];
  __shared__ double s_d[kWaves][kKnnMaxNN];
  __shared__ int s_i[kWaves][kKnnMaxNN];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = blockIdx.x * kWaves + w;
  if (q >= N) return;                                   // (a whole wave: no workgroup barrier follows)
  const int b = cloud_of(off, B, q);
  const int lo = off[b], hi = off[b + 1];
  const float qx = pts[3 * q], qy = pts[3 * q + 1], qz = pts[3 * q + 2];
  const long long cx = grid_coord(qx, inv_h), cy = grid_coord(qy, inv_h), cz = grid_coord(qz, inv_h);
  if (lane < 27)
    s_slot[w][lane] = (int)(cell_hash(b, cx + lane % 3 - 1, cy + (lane / 3) % 3 - 1, cz + lane / 9 - 1) & tmask);
  wave_sync();
  bool keep = lane < 27;
  if (keep)
    for (int k = 0; k < lane; ++k) keep = keep && s_slot[w][k] != s_slot[w][lane];
  const unsigned long long kmask = __ballot(keep);       // each distinct slot once (colliding cells would repeat rows)
  const unsigned long long lt = (1ull << lane) - 1;
  const int* sl = s_slot[w];
  int* si = s_i[w];
  double* sd = s_d[w];

  int total = 0;
  scan_cells(sl, kmask, start, cell_pts, lo, hi, qx, qy, qz, r2, [&](bool in, int, double) { total += __popcll(__ballot(in)); });
  const int k = total < max_nn ? total : max_nn;
  if (total <= max_nn) {
    int n = 0;
    scan_cells(sl, kmask, start, cell_pts, lo, hi, qx, qy, qz, r2, [&](bool in, int j, double d) {
      const unsigned long long m = __ballot(in);
      if (in) {
        const int pos = n + __popcll(m & lt);
        si[pos] = j;
        sd[pos] = d;
      }
      n += __popcll(m);
    });
  } else {
    // radix select of the max_nn-th smallest key; ph / pl hold the chosen digits so far under the masks mh / ml
    unsigned long long mh = 0, ph = 0;
    unsigned ml = 0, pl = 0;
    int need = max_nn;
    for (int pass = 0; pass < 12; ++pass) {
      for (int t = lane; t < 256; t += 64) s_hist[w][t] = 0;
      wave_sync();
      const int shh = 56 - 8 * pass, shl = 24 - 8 * (pass - 8);
      scan_cells(sl, kmask, start, cell_pts, lo, hi, qx, qy, qz, r2, [&](bool in, int j, double d) {
        if (in) {
          const unsigned long long kh = (unsigned long long)__double_as_longlong(d);
          const unsigned kl = (unsigned)j;
          if ((kh & mh) == ph && (kl & ml) == pl)
            atomicAdd(&s_hist[w][pass < 8 ? (int)((kh >> shh) & 255) : (int)((kl >> shl) & 255)], 1);
        }
      });
      wave_sync();
      int h4[4], s4 = 0;
      for (int u = 0; u < 4; ++u) {
        h4[u] = s_hist[w][lane * 4 + u];
        s4 += h4[u];
      }
      int incl = s4;
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
      }
      const int excl = incl - s4;
      const bool own = excl < need && need <= incl;
      const int owner = __builtin_ctzll(__ballot(own));
      int dig = 0, left = 0, binc = 0;
      if (own) {
        int c = excl;
        for (int u = 0; u < 4; ++u) {
          if (c + h4[u] >= need) {
            dig = lane * 4 + u;
            left = need - c;
            binc = h4[u];
            break;
          }
          c += h4[u];
        }
      }
      dig = __shfl(dig, owner);
      left = __shfl(left, owner);
      binc = __shfl(binc, owner);
      if (pass < 8) {
        ph |= (unsigned long long)dig << shh;
        mh |= 255ull << shh;
      } else {
        pl |= (unsigned)dig << shl;
        ml |= 255u << shl;
      }
      need = left;
      wave_sync();
      if (binc == need) break;                         // every key of the chosen bin is taken: the prefix decides
    }
    int n = 0;
    scan_cells(sl, kmask, start, cell_pts, lo, hi, qx, qy, qz, r2, [&](bool in, int j, double d) {
      bool sv = false;
      if (in) {
        const unsigned long long a = (unsigned long long)__double_as_longlong(d) & mh;
        sv = a < ph || (a == ph && ((unsigned)j & ml) <= pl);
      }
      const unsigned long long m = __ballot(sv);
      if (sv) {
        const int pos = n + __popcll(m & lt);
        si[pos] = j;
        sd[pos] = d;
      }
      n += __popcll(m);
    });
  }
  // bitonic sort of the k survivors by (d2, row), padded to a power of two
  int P = 1;
  while (P < k) P <<= 1;
  for (int t = k + lane; t < P; t += 64) {
    si[t] = INT_MAX;
    sd[t] = INFINITY;
  }
  wave_sync();
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int t = lane; t < P / 2; t += 64) {
        const int i0 = 2 * jj * (t / jj) + (t % jj), i1 = i0 + jj;
        const double a = sd[i0], c = sd[i1];
        const int ia = si[i0], ic = si[i1];
        const bool gt = a > c || (a == c && ia > ic);
        if (gt == ((i0 & kk) == 0)) {
          sd[i0] = c;
          sd[i1] = a;
          si[i0] = ic;
          si[i1] = ia;
        }
      }
      wave_sync();
    }
  }
  const size_t row = (size_t)q * max_nn;
  for (int t = lane; t < max_nn; t += 64) {
    const bool v = t < k;
    idx[row + t] = v ? si[t] - lo : -1;
    if (d2o) d2o[row + t] = v ? sd[t] : 0.0;
  }
  if (lane == 0) cnt_out[q] = k;
}

// ---------------------------------------------------------------------------------------------------------------------------
// normals: open3d's ComputeNormal (cumulant form) and FastEigen3x3 (Eberly, "A Robust Eigensolver for 3 x 3 Symmetric
// Matrices"), step for step in fp64
// ---------------------------------------------------------------------------------------------------------------------------

struct V3 {
  double x, y, z;
};
GMF_DEVINL V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
GMF_DEVINL double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// A: a00 a01 a02 a11 a12 a22
GMF_DEVINL V3 eigenvector0(const double* A, double e) {
  const V3 r0 = {A[0] - e, A[1], A[2]}, r1 = {A[1], A[3] - e, A[4]}, r2 = {A[2], A[4], A[5] - e};
  const V3 c01 = cross(r0, r1), c02 = cross(r0, r2), c12 = cross(r1, r2);
  const double d0 = dot(c01, c01), d1 = dot(c02, c02), d2 = dot(c12, c12);
  double dmax = d0;
  int imax = 0;
  if (d1 > dmax) {
    dmax = d1;
    imax = 1;
  }
  if (d2 > dmax) imax = 2;
  if (imax == 0) {
    const double s = sqrt(d0);
    return {c01.x / s, c01.y / s, c01.z / s};
  }
  if (imax == 1) {
    const double s = sqrt(d1);
    return {c02.x / s, c02.y / s, c02.z / s};
  }
  const double s = sqrt(d2);
  return {c12.x / s, c12.y / s, c12.z / s};
}

GMF_DEVINL V3 eigenvector1(const double* A, V3 e0, double e) {
  V3 U;
  if (fabs(e0.x) > fabs(e0.y)) {
    const double il = 1 / sqrt(e0.x * e0.x + e0.z * e0.z);
    U = {-e0.z * il, 0, e0.x * il};
  } else {
    const double il = 1 / sqrt(e0.y * e0.y + e0.z * e0.z);
    U = {0, e0.z * il, -e0.y * il};
  }
  const V3 V = cross(e0, U);
  const V3 AU = {A[0] * U.x + A[1] * U.y + A[2] * U.z, A[1] * U.x + A[3] * U.y + A[4] * U.z, A[2] * U.x + A[4] * U.y + A[5] * U.z};
  const V3 AV = {A[0] * V.x + A[1] * V.y + A[2] * V.z, A[1] * V.x + A[3] * V.y + A[4] * V.z, A[2] * V.x + A[4] * V.y + A[5] * V.z};
  double m00 = U.x * AU.x + U.y * AU.y + U.z * AU.z - e;
  double m01 = U.x * AV.x + U.y * AV.y + U.z * AV.z;
  double m11 = V.x * AV.x + V.y * AV.y + V.z * AV.z - e;
  const double a00 = fabs(m00), a01 = fabs(m01), a11 = fabs(m11);
  if (a00 >= a11) {
    if (fmax(a00, a01) > 0) {
      if (a00 >= a01) {
        m01 /= m00;
        m00 = 1 / sqrt(1 + m01 * m01);
        m01 *= m00;
      } else {
        m00 /= m01;
        m01 = 1 / sqrt(1 + m00 * m00);
        m00 *= m01;
      }
      return {m01 * U.x - m00 * V.x, m01 * U.y - m00 * V.y, m01 * U.z - m00 * V.z};
    }
    return U;
  }
  if (fmax(a11, a01) > 0) {
    if (a11 >= a01) {
      m01 /= m11;
      m11 = 1 / sqrt(1 + m01 * m01);
      m01 *= m11;
    } else {
      m11 /= m01;
      m01 = 1 / sqrt(1 + m11 * m11);
      m11 *= m01;
    }
    return {m11 * U.x - m01 * V.x, m11 * U.y - m01 * V.y, m11 * U.z - m01 * V.z};
  }
  return U;
}

// the eigenvector of the smallest eigenvalue (zero vector for a zero matrix)
GMF_DEVINL V3 fast_eigen3x3(double* A) {
  double mc = A[0];
  const double all[9] = {A[0], A[1], A[2], A[1], A[3], A[4], A[2], A[4], A[5]};
  for (int k = 1; k < 9; ++k) mc = all[k] > mc ? all[k] : mc;        // Eigen maxCoeff: the first maximum
  if (mc == 0) return {0, 0, 0};
  for (int k = 0; k < 6; ++k) A[k] /= mc;
  const double norm = A[1] * A[1] + A[2] * A[2] + A[4] * A[4];
  if (norm > 0) {
    const double q = (A[0] + A[3] + A[5]) / 3;
    const double b00 = A[0] - q, b11 = A[3] - q, b22 = A[5] - q;
    const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * 2) / 6);
    const double c00 = b11 * b22 - A[4] * A[4];
    const double c01 = A[1] * b22 - A[4] * A[2];
    const double c02 = A[1] * A[4] - b11 * A[2];
    const double det = (b00 * c00 - A[1] * c01 + A[2] * c02) / (p * p * p);
    double half_det = det * 0.5;
    half_det = fmin(fmax(half_det, -1.0), 1.0);
    const double angle = acos(half_det) / (double)3;
    const double two_thirds_pi = 2.09439510239319549;
    const double beta2 = cos(angle) * 2;
    const double beta0 = cos(angle + two_thirds_pi) * 2;
    const double beta1 = -(beta0 + beta2);
    const double e0 = q + p * beta0, e1 = q + p * beta1, e2 = q + p * beta2;
    if (half_det >= 0) {
      const V3 v2 = eigenvector0(A, e2);
      if (e2 < e0 && e2 < e1) return v2;
      const V3 v1 = eigenvector1(A, v2, e1);
      if (e1 < e0 && e1 < e2) return v1;
      return cross(v1, v2);
    }
    const V3 v0 = eigenvector0(A, e0);
    if (e0 < e1 && e0 < e2) return v0;
    const V3 v1 = eigenvector1(A, v0, e1);
    if (e1 < e0 && e1 < e2) return v1;
    return cross(v0, v1);
  }
  for (int k = 0; k < 6; ++k) A[k] *= mc;
  if (A[0] < A[3] && A[0] < A[5]) return {1, 0, 0};
  if (A[3] < A[0] && A[3] < A[5]) return {0, 1, 0};
  return {0, 0, 1};
}

__global__ __launch_bounds__(kThreads) void k_normals(const float* __restrict__ pts, const int* __restrict__ off, int B, int N,
                                                      const int* __restrict__ idx, const int* __restrict__ count, int max_nn,
                                                      float* __restrict__ normals) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int c = count[i];
  V3 n = {0, 0, 1};
  if (c >= 3) {
    const int lo = off[cloud_of(off, B, i)];
    double cu[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int* row = idx + (size_t)i * max_nn;
    for (int t = 0; t < c; ++t) {
      const int j = lo + row[t];
      const double x = pts[3 * j], y = pts[3 * j + 1], z = pts[3 * j + 2];
      cu[0] += x;
      cu[1] += y;
      cu[2] += z;
      cu[3] += x * x;
      cu[4] += x * y;
      cu[5] += x * z;
      cu[6] += y * y;
      cu[7] += y * z;
      cu[8] += z * z;
    }
    for (int k = 0; k < 9; ++k) cu[k] /= (double)c;
    double A[6] = {cu[3] - cu[0] * cu[0], cu[4] - cu[0] * cu[1], cu[5] - cu[0] * cu[2],
                   cu[6] - cu[1] * cu[1], cu[7] - cu[1] * cu[2], cu[8] - cu[2] * cu[2]};
    n = fast_eigen3x3(A);
    if (n.x * n.x + n.y * n.y + n.z * n.z == 0.0) n = {0, 0, 1};
  }
  normals[3 * i] = (float)n.x;
  normals[3 * i + 1] = (float)n.y;
  normals[3 * i + 2] = (float)n.z;
}

// ---------------------------------------------------------------------------------------------------------------------------
// colour gradients: open3d's InitializePointCloudForColoredICP
// ---------------------------------------------------------------------------------------------------------------------------

// One lane per row, over the row's neighbour list (key (d^2, row), self included).  count < 4: g = 0.  Otherwise the first list
// entry is skipped as open3d skips it (the query row, unless an earlier row coincides with it), and over the others in list
// order, in fp64 from the fp32 inputs: e = v_a - v, d = e - (e . n) n, A = sum d d^T + (count - 1)^2 n n^T,
// b = sum d (I_a - I).  A g = b by 3 x 3 LDL^T without pivoting; pivot d_k is accepted when it is finite and d_k > 2^-40 A_kk.
// A rejected pivot or a non-finite component gives g = 0 (open3d applies whatever ldlt() returns).  Every use of n is an even
// product: negating a normal changes no bit.
__global__ __launch_bounds__(kThreads) void k_color_gradient(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                             const float* __restrict__ inten, const int* __restrict__ off, int B,
                                                             int N, const int* __restrict__ idx, const int* __restrict__ count,
                                                             int max_nn, float* __restrict__ grad) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int c = count[i];
  double g[3] = {0, 0, 0};
  if (c >= 4) {
    const int lo = off[cloud_of(off, B, i)];
    const double vx = pts[3 * i], vy = pts[3 * i + 1], vz = pts[3 * i + 2];
    const double nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2], I = inten[i];
    double A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};          // A: xx xy xz yy yz zz
    const int* row = idx + (size_t)i * max_nn;
    for (int t = 1; t < c; ++t) {
      const int j = lo + row[t];
      const double ex = (double)pts[3 * j] - vx, ey = (double)pts[3 * j + 1] - vy, ez = (double)pts[3 * j + 2] - vz;
      const double en = fma(ex, nx, fma(ey, ny, ez * nz));
      const double dx = fma(-en, nx, ex), dy = fma(-en, ny, ey), dz = fma(-en, nz, ez);
      const double di = (double)inten[j] - I;
      A[0] = fma(dx, dx, A[0]);
      A[1] = fma(dx, dy, A[1]);
      A[2] = fma(dx, dz, A[2]);
      A[3] = fma(dy, dy, A[3]);
      A[4] = fma(dy, dz, A[4]);
      A[5] = fma(dz, dz, A[5]);
      b[0] = fma(dx, di, b[0]);
      b[1] = fma(dy, di, b[1]);
      b[2] = fma(dz, di, b[2]);
    }
    const double w = (double)(c - 1) * (double)(c - 1);           // (the products of two fp32 normals are exact in fp64)
    A[0] = fma(w, nx * nx, A[0]);
    A[1] = fma(w, nx * ny, A[1]);
    A[2] = fma(w, nx * nz, A[2]);
    A[3] = fma(w, ny * ny, A[3]);
    A[4] = fma(w, ny * nz, A[4]);
    A[5] = fma(w, nz * nz, A[5]);
    const double d0 = A[0];
    bool ok = isfinite(d0) && d0 > 0x1p-40 * A[0];
    const double l10 = A[1] / d0, l20 = A[2] / d0;
    const double d1 = A[3] - (l10 * l10) * d0;
    ok = ok && isfinite(d1) && d1 > 0x1p-40 * A[3];
    const double l21 = (A[4] - (l20 * l10) * d0) / d1;
    const double d2 = (A[5] - (l20 * l20) * d0) - (l21 * l21) * d1;
    ok = ok && isfinite(d2) && d2 > 0x1p-40 * A[5];
    if (ok) {
      const double y0 = b[0], y1 = b[1] - l10 * y0, y2 = (b[2] - l20 * y0) - l21 * y1;      // L y = b
      const double x2 = y2 / d2, x1 = y1 / d1 - l21 * x2, x0 = (y0 / d0 - l10 * x1) - l20 * x2;   // D z = y, L^T g = z
      if (isfinite(x0) && isfinite(x1) && isfinite(x2)) { g[0] = x0; g[1] = x1; g[2] = x2; }
    }
  }
  grad[3 * i] = (float)g[0];
  grad[3 * i + 1] = (float)g[1];
  grad[3 * i + 2] = (float)g[2];
}

// ---------------------------------------------------------------------------------------------------------------------------
// FPFH: open3d's ComputePairFeatures, SPFH and FPFH
// ---------------------------------------------------------------------------------------------------------------------------

// bin of (11 (x + 1) * 0.5) style values; NaN -> 0
GMF_DEVINL int bin11(double v) {
  if (!(v == v)) return 0;
  const double f = floor(v);
  return f < 0 ? 0 : (f >= 11 ? 10 : (int)f);
}

__global__ __launch_bounds__(kThreads) void k_spfh(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                   const int* __restrict__ off, int B, int N, const int* __restrict__ idx,
                                                   const int* __restrict__ count, int max_nn, double* __restrict__ spfh) {
  __shared__ int s_h[kWaves][33];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * kWaves + w;
  if (i >= N) return;
  if (lane < 33) s_h[w][lane] = 0;
  wave_sync();
  const int c = count[i];
  if (c > 1) {
    const int lo = off[cloud_of(off, B, i)];
    const V3 p1 = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const V3 n1 = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
    const double kPi = 3.14159265358979323846;
    for (int t = lane; t < c; t += 64) {
      const int j = lo + idx[(size_t)i * max_nn + t];
      if (j == i) continue;                            // the query, by index
      const V3 p2 = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
      const V3 n2 = {nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2]};
      double f0 = 0, f1 = 0, f2 = 0;
      V3 dp = {p2.x - p1.x, p2.y - p1.y, p2.z - p1.z};
      const double d = sqrt(dp.x * dp.x + dp.y * dp.y + dp.z * dp.z);
      if (d != 0.0) {
        V3 ns = n1, nt = n2;
        const double a1 = dot(n1, dp) / d, a2 = dot(n2, dp) / d;
        if (acos(fabs(a1)) > acos(fabs(a2))) {
          ns = n2;
          nt = n1;
          dp = {-dp.x, -dp.y, -dp.z};
          f2 = -a2;
        } else {
          f2 = a1;
        }
        V3 v = cross(dp, ns);
        const double vn = sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
        if (vn == 0.0) {
          f2 = 0;
        } else {
          v = {v.x / vn, v.y / vn, v.z / vn};
          const V3 ww = cross(ns, v);
          f1 = dot(v, nt);
          f0 = atan2(dot(ww, nt), dot(ns, nt));
        }
      }
      atomicAdd(&s_h[w][bin11(11 * (f0 + kPi) / (2.0 * kPi))], 1);
      atomicAdd(&s_h[w][11 + bin11(11 * (f1 + 1.0) * 0.5)], 1);
      atomicAdd(&s_h[w][22 + bin11(11 * (f2 + 1.0) * 0.5)], 1);
    }
  }
  wave_sync();
  if (lane < 33) spfh[(size_t)i * 33 + lane] = c > 1 ? (double)s_h[w][lane] * (100.0 / (double)(c - 1)) : 0.0;
}

__global__ __launch_bounds__(kThreads) void k_fpfh(const int* __restrict__ off, int B, int N, const int* __restrict__ idx,
                                                   const double* __restrict__ d2, const int* __restrict__ count, int max_nn,
                                                   const double* __restrict__ spfh, float* __restrict__ out) {
  __shared__ double s_a[kWaves][33];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * kWaves + w;
  if (i >= N) return;
  const int c = count[i];
  double acc = 0.0;
  if (c > 1 && lane < 33) {
    const int lo = off[cloud_of(off, B, i)];
    const size_t row = (size_t)i * max_nn;
    for (int t = 0; t < c; ++t) {
      const int j = lo + idx[row + t];
      const double dist = d2[row + t];
      if (j == i || dist == 0.0) continue;
      acc += spfh[(size_t)j * 33 + lane] / dist;
    }
  }
  if (lane < 33) s_a[w][lane] = acc;
  wave_sync();
  if (lane < 33) {
    const int b0 = lane / 11 * 11;
    double sum = 0.0;
    for (int u = 0; u < 11; ++u) sum += s_a[w][b0 + u];
    const double sc = sum != 0.0 ? 100.0 / sum : 0.0;
    out[(size_t)i * 33 + lane] = c > 1 ? (float)(acc * sc + spfh[(size_t)i * 33 + lane]) : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// voxel grids
// ---------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_cloud_min(const float* __restrict__ pts, const int* __restrict__ off, double half,
                                                        double* __restrict__ origin) {
  __shared__ float sm[3][kThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  float m[3] = {INFINITY, INFINITY, INFINITY};
  for (int i = off[b] + tid; i < off[b + 1]; i += kThreads)
    for (int k = 0; k < 3; ++k) m[k] = fminf(m[k], pts[3 * i + k]);
  for (int k = 0; k < 3; ++k) sm[k][tid] = m[k];
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < 3; ++k) sm[k][tid] = fminf(sm[k][tid], sm[k][tid + s]);
    __syncthreads();
  }
  if (tid < 3) origin[3 * b + tid] = (double)sm[tid][0] - half;
}

GMF_DEVINL bool voxel_of(const float* __restrict__ pts, int i, const double* o, double v, int (&c)[3]) {
  for (int k = 0; k < 3; ++k) {
    const double r = floor(((double)pts[3 * i + k] - (o ? o[k] : 0.0)) / v);
    if (!(r >= -2147483648.0 && r <= 2147483647.0)) return false;
    c[k] = (int)r;
  }
  return true;
}

__global__ __launch_bounds__(kThreads) void k_voxel_insert(const float* __restrict__ pts, const int* __restrict__ off, int B, int N,
                                                           const double* __restrict__ origin, double v, unsigned long long tmask,
                                                           int* table, int* rep, int* __restrict__ slot, int* flag) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int b = cloud_of(off, B, i);
  const double* o = origin ? origin + 3 * b : nullptr;
  int c[3];
  if (!voxel_of(pts, i, o, v, c)) {
    slot[i] = -1;
    atomicOr(flag, 1);
    return;
  }
  unsigned long long h = cell_hash(b, c[0], c[1], c[2]) & tmask;
  for (unsigned long long probe = 0; probe <= tmask; ++probe) {
    int cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur < 0) {
      cur = atomicCAS(&table[h], -1, i);
      if (cur < 0) break;                              // this row opened the slot
    }
    int cc[3];
    if (cloud_of(off, B, cur) == b && voxel_of(pts, cur, o, v, cc) && cc[0] == c[0] && cc[1] == c[1] && cc[2] == c[2]) break;
    h = (h + 1) & tmask;
  }
  atomicMin(&rep[h], i);
  slot[i] = (int)h;
}

__global__ __launch_bounds__(kThreads) void k_voxel_heads(int N, const int* __restrict__ rep, const int* __restrict__ slot,
                                                          int* __restrict__ head) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i > N) return;
  head[i] = i < N && slot[i] >= 0 && rep[slot[i]] == i;
}

__global__ __launch_bounds__(kThreads) void k_voxel_keys(int N, const int* __restrict__ rep, const int* __restrict__ slot,
                                                         const int* __restrict__ vid, unsigned long long* __restrict__ key) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int s = slot[i];
  key[i] = s < 0 ? ~0ull : ((unsigned long long)vid[rep[s]] << 32) | (unsigned)i;
}

__global__ __launch_bounds__(kThreads) void k_voxel_starts(int N, const unsigned long long* __restrict__ key, int* __restrict__ vstart) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= N) return;
  const unsigned long long k = key[p];
  if (k == ~0ull) return;
  const unsigned v = (unsigned)(k >> 32);
  if (p == 0 || (unsigned)(key[p - 1] >> 32) != v) vstart[v] = p;
  if (p == N - 1 || (unsigned)(key[p + 1] >> 32) != v) vstart[v + 1] = p + 1;
}

__global__ __launch_bounds__(kThreads) void k_voxel_mean(const float* __restrict__ pts, int N, const unsigned long long* __restrict__ key,
                                                         const int* __restrict__ vstart, const int* __restrict__ nv,
                                                         float* __restrict__ out) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= N || v >= *nv) return;
  const int a = vstart[v], e = vstart[v + 1];
  double s[3] = {0, 0, 0};
  for (int p = a; p < e; ++p) {
    const int i = (int)(key[p] & 0xffffffffull);
    for (int k = 0; k < 3; ++k) s[k] += (double)pts[3 * i + k];
  }
  for (int k = 0; k < 3; ++k) out[3 * v + k] = (float)(s[k] / (double)(e - a));
}

__global__ __launch_bounds__(kThreads) void k_voxel_select(const int* __restrict__ off, int B, int N, const int* __restrict__ head,
                                                           const int* __restrict__ vid, int* __restrict__ out_idx) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N || !head[i]) return;
  out_idx[vid[i]] = i - off[cloud_of(off, B, i)];
}

__global__ void k_voxel_offsets(const int* __restrict__ off, int B, const int* __restrict__ vid, int* __restrict__ out_off) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b <= B) out_off[b] = vid[off[b]];
}

int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------

void knn_scratch_list(long long N, KnnScratch& s, ArenaList& bufs) {
  s.T = table_slots(N);
  s.scan_bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s.scan_bytes, (int*)nullptr, (int*)nullptr, (int)(s.T + 1));
  bufs.add(s.slot, (size_t)N);
  bufs.add(s.cnt, (size_t)s.T + 1);
  bufs.add(s.start, (size_t)s.T + 1);
  bufs.add(s.cell_pts, (size_t)N);
  bufs.add(s.scan_tmp, s.scan_bytes);
}

hipError_t launch_grid_build(const float* pts, const int* offsets, int B, long long N, double h, const KnnScratch& ws,
                             hipStream_t s) {
  const double inv_h = 1.0 / h;
  const unsigned long long tmask = (unsigned long long)ws.T - 1;
  hipError_t e = hipMemsetAsync(ws.cnt, 0, (ws.T + 1) * 4, s);
  if (e != hipSuccess) return e;
  k_grid_count<<<blocks(N, kThreads), kThreads, 0, s>>>(pts, offsets, B, (int)N, tmask, inv_h, ws.slot, ws.cnt);
  size_t sb = ws.scan_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(ws.scan_tmp, sb, ws.cnt, ws.start, (int)(ws.T + 1), s);
  if (e != hipSuccess) return e;
  k_grid_scatter<<<blocks(N, kThreads), kThreads, 0, s>>>(pts, (int)N, ws.slot, ws.start, ws.cnt, ws.cell_pts);
  return hipGetLastError();
}

hipError_t launch_radius_knn(const float* pts, const int* offsets, int B, long long N, double radius, int max_nn,
                             const KnnScratch& ws, int* idx, double* d2, int* count, hipStream_t s) {
  const double h = radius * (1.0 + 1.0 / 1024);
  hipError_t e = launch_grid_build(pts, offsets, B, N, h, ws, s);
  if (e != hipSuccess) return e;
  k_knn_search<<<blocks(N, kWaves), kThreads, 0, s>>>(pts, offsets, B, (int)N, (unsigned long long)ws.T - 1, 1.0 / h,
                                                     radius * radius, max_nn, ws.start, ws.cell_pts, idx, d2, count);
  return hipGetLastError();
}

hipError_t launch_normals(const float* pts, const int* offsets, int B, long long N, const int* idx, const int* count,
                          int max_nn, float* normals, hipStream_t s) {
  k_normals<<<blocks(N, kThreads), kThreads, 0, s>>>(pts, offsets, B, (int)N, idx, count, max_nn, normals);
  return hipGetLastError();
}

hipError_t launch_color_gradient(const float* pts, const float* normals, const float* intensity, const int* offsets, int B,
                                 long long N, const int* idx, const int* count, int max_nn, float* gradients, hipStream_t s) {
  k_color_gradient<<<blocks(N, kThreads), kThreads, 0, s>>>(pts, normals, intensity, offsets, B, (int)N, idx, count, max_nn,
                                                            gradients);
  return hipGetLastError();
}

hipError_t launch_fpfh(const float* pts, const float* normals, const int* offsets, int B, long long N, const int* idx,
                       const double* d2, const int* count, int max_nn, double* spfh, float* features, hipStream_t s) {
  k_spfh<<<blocks(N, kWaves), kThreads, 0, s>>>(pts, normals, offsets, B, (int)N, idx, count, max_nn, spfh);
  k_fpfh<<<blocks(N, kWaves), kThreads, 0, s>>>(offsets, B, (int)N, idx, d2, count, max_nn, spfh, features);
  return hipGetLastError();
}

void voxel_scratch_list(long long N, int B, VoxelScratch& s, ArenaList& bufs) {
  size_t scan = 0, sort = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (int*)nullptr, (int*)nullptr, (int)(N + 1));
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, sort, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)N);
  s.T = table_slots(N);
  s.tmp_bytes = scan > sort ? scan : sort;
  bufs.add(s.table, (size_t)s.T);
  bufs.add(s.rep, (size_t)s.T);
  bufs.add(s.slot, (size_t)N);
  bufs.add(s.head, (size_t)N + 1);
  bufs.add(s.vid, (size_t)N + 1);
  bufs.add(s.key, (size_t)N);
  bufs.add(s.key_sorted, (size_t)N);
  bufs.add(s.vstart, (size_t)N + 1);
  bufs.add(s.lo, (size_t)B * 3);
  bufs.add(s.flag, 1);
  bufs.add(s.tmp, s.tmp_bytes);
}

hipError_t launch_voxel(const float* pts, const int* offsets, int B, long long N, double voxel, bool mean,
                        const VoxelScratch& ws, float* out_pts, int* out_idx, int* out_offsets, int* host2, hipStream_t s,
                        const float* colors, float* out_colors) {
  const unsigned long long tmask = (unsigned long long)ws.T - 1;
  const int n = (int)N;
  hipError_t e = hipMemsetAsync(ws.table, 0xFF, ws.T * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws.rep, 0x7F, ws.T * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws.flag, 0, 4, s);
  if (e != hipSuccess) return e;
  if (mean) k_cloud_min<<<B, kThreads, 0, s>>>(pts, offsets, voxel * 0.5, ws.lo);
  k_voxel_insert<<<blocks(N, kThreads), kThreads, 0, s>>>(pts, offsets, B, n, mean ? ws.lo : nullptr, voxel, tmask, ws.table,
                                                          ws.rep, ws.slot, ws.flag);
  k_voxel_heads<<<blocks(N + 1, kThreads), kThreads, 0, s>>>(n, ws.rep, ws.slot, ws.head);
  size_t tb = ws.tmp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(ws.tmp, tb, ws.head, ws.vid, n + 1, s);
  if (e != hipSuccess) return e;
  if (mean) {
    k_voxel_keys<<<blocks(N, kThreads), kThreads, 0, s>>>(n, ws.rep, ws.slot, ws.vid, ws.key);
    int vbits = 1;
    while (vbits < 32 && (1LL << vbits) <= N) ++vbits;
    tb = ws.tmp_bytes;
    e = hipcub::DeviceRadixSort::SortKeys(ws.tmp, tb, ws.key, ws.key_sorted, n, 0, 32 + vbits, s);
    if (e != hipSuccess) return e;
    k_voxel_starts<<<blocks(N, kThreads), kThreads, 0, s>>>(n, ws.key_sorted, ws.vstart);
    k_voxel_mean<<<blocks(N, kThreads), kThreads, 0, s>>>(pts, n, ws.key_sorted, ws.vstart, ws.vid + N, out_pts);
    if (colors)                                        // the same mean over the same rows in the same order, of the colours
      k_voxel_mean<<<blocks(N, kThreads), kThreads, 0, s>>>(colors, n, ws.key_sorted, ws.vstart, ws.vid + N, out_colors);
  } else {
    k_voxel_select<<<blocks(N, kThreads), kThreads, 0, s>>>(offsets, B, n, ws.head, ws.vid, out_idx);
  }
  k_voxel_offsets<<<blocks(B + 1, 64), 64, 0, s>>>(offsets, B, ws.vid, out_offsets);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host2, ws.vid + N, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(host2 + 1, ws.flag, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e;
}

}  // namespace gmf
