// Multiway registration: the two pieces the reference takes from open3d 0.9 in
// GMF_PointDSC/multiway/test_multi_ate.py - get_information_matrix_from_point_clouds and global_optimization.
//
//   k_info_chunk       one workgroup per (edge, chunk of kInfoChunk source rows): k_icp_nn_grid's search, 32 lanes per source
//                      row over the 27 cells of the TARGET cloud's id, the same (d^2 bits | row) minimum; the row's leader lane
//                      gathers the winner's target row and adds its G^T G terms in fp64; nine sums and the count per chunk.
//   k_info_finish      one wave per edge: the chunk partials in chunk order per lane, then a fixed butterfly; the 36 entries.
//   k_posegraph        one persistent workgroup per graph: Levenberg-Marquardt with a line process per uncertain edge, two
//                      passes with the pruning in between.  H and its factor live in the workspace; the LDL^T is right-looking
//                      in panels of kPanel columns held in LDS.
//
// No floating-point atomics anywhere: every sum has one owner and a fixed order.  This file is compiled with -ffp-contract=off:
// the fp64 terms are those of tests/posegraph_reference.py operation for operation (the explicit fma of the row transform, which
// is ICP's, stays).
#include <math.h>

#include "grid_hash.hpp"
#include "launchers_posegraph.hpp"

namespace gmf {

constexpr int kThreads = 256;
constexpr int kGridLanes = 32;                           // as in solver_kernels.hip: lanes per source row, one per cell (27 used)
constexpr int kGridRows = kThreads / kGridLanes;
constexpr int kGridBigSlot = 32;

// ICP's transformed row (solver_kernels.hip transform_row), operand for operand
GMF_DEVINL void transform_row(const double* T, const float* a, float* p) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
    p[r] = (float)fma(T[4 * r], (double)a[0], fma(T[4 * r + 1], (double)a[1], fma(T[4 * r + 2], (double)a[2], T[4 * r + 3])));
}

// ---------------------------------------------------------------------------------------------------------------------------
// information matrices
// ---------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads)
k_info_chunk(const float* __restrict__ pts, const int* __restrict__ coff, const int* __restrict__ esrc, const int* __restrict__ etgt,
             const InfoChunk* __restrict__ chunks, const double* __restrict__ Tin, float tau2, unsigned long long tmask, double inv_h,
             const int* __restrict__ start, const float4* __restrict__ cell_pts, double* __restrict__ part, long long* __restrict__ nn) {
  __shared__ double sh[kGridRows][kInfoPart];
  const InfoChunk ck = chunks[blockIdx.x];
  const int tid = threadIdx.x, g = tid & (kGridLanes - 1), half = (tid & 63) >> 5, grp = tid / kGridLanes;
  const int cs = esrc[ck.edge], ct = etgt[ck.edge];
  const int s0 = coff[cs] + ck.row0, q0 = coff[ct], q1 = coff[ct + 1];
  double T[12];
  bool fin = true;
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    T[e] = Tin[16 * (size_t)ck.edge + e];
    fin = fin && isfinite(T[e]);
  }
  double v[kInfoPart];
#pragma unroll
  for (int d = 0; d < kInfoPart; ++d) v[d] = 0.0;
  // (every bound of this loop is uniform over the workgroup: the ballot and the shuffles below see whole waves)
  for (int r0 = 0; r0 < ck.n; r0 += kGridRows) {
    const int i = r0 + grp;
    float p[3] = {0.f, 0.f, 0.f};
    int a = 0, e = 0;
    if (i < ck.n && fin) {
      transform_row(T, pts + 3 * (size_t)(s0 + i), p);
      if (g < 27) {
        const int s = (int)(cell_hash(ct, grid_coord(p[0], inv_h) + g % 3 - 1, grid_coord(p[1], inv_h) + (g / 3) % 3 - 1,
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
    for (unsigned long long m = __ballot(big); m; m &= m - 1) {                    // a crowded slot: its row's 32 lanes share it
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
    if (g == 0 && i < ck.n) {
      const float d2 = __uint_as_float((unsigned)(best >> 32));
      const int j = (int)(best & 0xffffffffull);
      const bool in = best != ~0ull && d2 < tau2;                                  // k_icp_step's test
      if (nn) nn[(size_t)ck.out0 + i] = in ? j : -1;
      if (in) {
        const float* q = pts + 3 * (size_t)(q0 + j);
        const double x = q[0], y = q[1], z = q[2];
        v[0] += y * y + z * z; v[1] += x * x + z * z; v[2] += x * x + y * y;
        v[3] += x * y; v[4] += x * z; v[5] += y * z;
        v[6] += x; v[7] += y; v[8] += z;
        v[9] += 1.0;
      }
    }
  }
  if (g == 0) {
#pragma unroll
    for (int d = 0; d < kInfoPart; ++d) sh[grp][d] = v[d];
  }
  __syncthreads();
  if (tid < kInfoPart)
    part[(size_t)blockIdx.x * kInfoPart + tid] =
        ((sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid])) + ((sh[4][tid] + sh[5][tid]) + (sh[6][tid] + sh[7][tid]));
}

// block = one wave per edge
__global__ void __launch_bounds__(64)
k_info_finish(const double* __restrict__ part, const int* __restrict__ edge_chunk0, double* __restrict__ info, int* __restrict__ count) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const int c0 = edge_chunk0[e], c1 = edge_chunk0[e + 1];
  double v[kInfoPart];
#pragma unroll
  for (int d = 0; d < kInfoPart; ++d) v[d] = 0.0;
  for (int c = c0 + lane; c < c1; c += 64) {
#pragma unroll
    for (int d = 0; d < kInfoPart; ++d) v[d] += part[(size_t)c * kInfoPart + d];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int d = 0; d < kInfoPart; ++d) v[d] += __shfl_xor(v[d], o, 64);
  }
  if (lane == 0) {
    double* I = info + 36 * (size_t)e;
    const double n = v[9];
    const double M[36] = {v[0],  -v[3], -v[4], 0.0,   -v[8], v[7],
                          -v[3], v[1],  -v[5], v[8],  0.0,   -v[6],
                          -v[4], -v[5], v[2],  -v[7], v[6],  0.0,
                          0.0,   v[8],  -v[7], n,     0.0,   0.0,
                          -v[8], 0.0,   v[6],  0.0,   n,     0.0,
                          v[7],  -v[6], 0.0,   0.0,   0.0,   n};
#pragma unroll
    for (int k = 0; k < 36; ++k) I[k] = M[k] + 0.0;      // (-0 -> +0)
    count[e] = (int)n;
  }
}

void info_scratch_list(long long N, long n_chunks, InfoScratch& s, ArenaList& bufs) {
  knn_scratch_list(N, s.grid, bufs);
  bufs.add(s.part, (size_t)n_chunks * kInfoPart);
}

hipError_t launch_information_matrix(const float* pts, const int* cloud_off, int F, long long N, const int* esrc, const int* etgt,
                                     int E, const InfoChunk* chunks, long n_chunks, const int* edge_chunk0, const double* T, float tau,
                                     const InfoScratch& ws, double* info, int* count, long long* nn, hipStream_t s) {
  const double h = (double)tau * (1.0 + 1.0 / 1024);     // ICP's cell edge
  hipError_t e = launch_grid_build(pts, cloud_off, F, N, h, ws.grid, s);
  if (e != hipSuccess) return e;
  if (n_chunks > 0)
    hipLaunchKernelGGL(k_info_chunk, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, pts, cloud_off, esrc, etgt, chunks, T, tau * tau,
                       (unsigned long long)ws.grid.T - 1, 1.0 / h, ws.grid.start, ws.grid.cell_pts, ws.part, nn);
  hipLaunchKernelGGL(k_info_finish, dim3((unsigned)E), dim3(64), 0, s, ws.part, edge_chunk0, info, count);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------
// pose-graph optimisation
// ---------------------------------------------------------------------------------------------------------------------------

constexpr int kPanel = 4;                                // panel columns of the LDL^T held in LDS: 6 * 256 rows * 4 * 8 B = 48 KiB
constexpr int kMaxDim = 6 * kPoseGraphMaxNodes;

// stop codes (tests/posegraph_reference.py names them the same)
enum { kStopMaxIter = 0, kStopRightTerm = 1, kStopIncrement = 2, kStopResidualIncrement = 3, kStopResidual = 4, kStopLmMax = 5,
       kStopPivot = 6 };

// rigid [R | t] as 12 doubles, row-major 3 x 4
GMF_DEVINL void rigid_mul(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) C[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j];
    C[4 * i + 3] = A[4 * i] * B[3] + A[4 * i + 1] * B[7] + A[4 * i + 2] * B[11] + A[4 * i + 3];
  }
}
GMF_DEVINL void rigid_inv(const double* A, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) C[4 * i + j] = A[4 * j + i];
    C[4 * i + 3] = -(A[i] * A[3] + A[4 + i] * A[7] + A[8 + i] * A[11]);
  }
}
GMF_DEVINL void load12(const double* P16, double* A) {
#pragma unroll
  for (int e = 0; e < 12; ++e) A[e] = P16[e];
}
// lin of a 3 x 4 block
GMF_DEVINL void lin12(const double* M, double* z) {
  z[0] = (M[9] - M[6]) / 2;
  z[1] = (M[2] - M[8]) / 2;
  z[2] = (M[4] - M[1]) / 2;
  z[3] = M[3]; z[4] = M[7]; z[5] = M[11];
}
GMF_DEVINL void mat6(const double* v, double* M) {
  const double cx = cos(v[0]), sx = sin(v[0]), cy = cos(v[1]), sy = sin(v[1]), cz = cos(v[2]), sz = sin(v[2]);
  M[0] = cz * cy; M[1] = cz * sy * sx - sz * cx; M[2] = cz * sy * cx + sz * sx; M[3] = v[3];
  M[4] = sz * cy; M[5] = sz * sy * sx + cz * cx; M[6] = sz * sy * cx - cz * sx; M[7] = v[4];
  M[8] = -sy;     M[9] = cy * sx;                M[10] = cy * cx;               M[11] = v[5];
}
GMF_DEVINL void vec6(const double* M, double* v) {
  v[0] = atan2(M[9], M[10]);
  v[1] = atan2(-M[8], sqrt(M[9] * M[9] + M[10] * M[10]));
  v[2] = atan2(M[4], M[0]);
  v[3] = M[3]; v[4] = M[7]; v[5] = M[11];
}

// the workgroup's sum of x(c), c in [0, n): thread t adds c = t, t + 256, ... in order, then a fixed halving tree
template <typename F>
GMF_DEVINL double wg_sum(int n, double* sh, F&& x) {
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int c = tid; c < n; c += kThreads) a += x(c);
  __syncthreads();
  sh[tid] = a;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
template <typename F>
GMF_DEVINL double wg_max(int n, double* sh, F&& x) {
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int c = tid; c < n; c += kThreads) {
    const double y = x(c);
    a = (y > a || y != y) ? y : a;                       // a NaN sticks
  }
  __syncthreads();
  sh[tid] = a;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const double y = sh[tid + s];
      if (y > sh[tid] || y != y) sh[tid] = y;
    }
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

struct PgGraph {
  int n, m, ma, node0, edge0, ref;                       // ma: edges alive in this pass (elist[0 .. ma))
  const int *esrc, *etgt;                                // the call's arrays, indexed by edge0 + k
  const double *X, *Lam;
  const unsigned char* unc;
  const int* elist;
  double p;
};

// zeta and q = zeta^T Lambda zeta of edge k (numbered within the call) at poses P [16 per node, numbered within the graph]
GMF_DEVINL double edge_residual(const PgGraph& g, int k, const double* P, double* zeta, double* A) {
  double Xk[12], Xi[12], Pt[12], Pti[12], Ps[12], Z[12];
  load12(g.X + 16 * (size_t)k, Xk);
  load12(P + 16 * (size_t)g.etgt[k], Pt);
  load12(P + 16 * (size_t)g.esrc[k], Ps);
  rigid_inv(Xk, Xi);
  rigid_inv(Pt, Pti);
  rigid_mul(Xi, Pti, A);
  rigid_mul(A, Ps, Z);
  lin12(Z, zeta);
  const double* Lm = g.Lam + 36 * (size_t)k;
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) a += Lm[6 * i + j] * zeta[j];
    q += zeta[i] * a;
  }
  return q;
}

// The linearisation at poses P: per alive edge l, its share e of the residual, J_s, l J^T Lambda J and l J^T Lambda zeta;
// then H and b per node in edge order.  Returns r.
GMF_DEVINL double linearise(const PgGraph& g, const double* P, double* lp, double* ev, double* JM, double* H,
                            double* b, const int* nl0, const NodeEdge* list, const unsigned char* alive, double* sh) {
  const int tid = threadIdx.x, N6 = 6 * g.n;
  for (int c = tid; c < g.ma; c += kThreads) {
    const int k = g.elist[c];
    double zeta[6], A[12], Ps[12];
    const double q = edge_residual(g, k, P, zeta, A);
    load12(P + 16 * (size_t)g.esrc[k], Ps);
    double l = 1.0, e;
    if (g.unc[k]) {
      const double w = g.p / (g.p + q);
      l = w * w;
      const double d = sqrt(l) - 1.0;
      e = l * q + g.p * (d * d);
    } else {
      e = l * q;
    }
    lp[k] = l;
    ev[c] = e;
    double* out = JM + 78 * (size_t)k;
    double J[36];                                        // row-major 6 x 6: J[a][i] = component a of column i
    // columns 0..2: lin(Ra S_i [Rs | ts]); S_i the generator of the rotation about axis i
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int u = (i + 1) % 3, w = (i + 2) % 3;        // S_i: row u <- -row w ... (S_i P)[u] = -P[w], (S_i P)[w] = P[u]
      double GP[12], M[12];
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        GP[4 * i + c4] = 0.0;
        GP[4 * u + c4] = -Ps[4 * w + c4];
        GP[4 * w + c4] = Ps[4 * u + c4];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) M[4 * r + c4] = A[4 * r] * GP[c4] + A[4 * r + 1] * GP[4 + c4] + A[4 * r + 2] * GP[8 + c4];
      double z[6];
      lin12(M, z);
#pragma unroll
      for (int a = 0; a < 6; ++a) J[6 * a + i] = z[a];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        J[6 * a + 3 + i] = 0.0;
        J[6 * (a + 3) + 3 + i] = A[4 * a + i];
      }
    }
    const double* Lm = g.Lam + 36 * (size_t)k;
    double LJ[36], Lz[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double s = 0.0;
#pragma unroll
      for (int bb = 0; bb < 6; ++bb) s += Lm[6 * a + bb] * zeta[bb];
      Lz[a] = s;
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) {
        double t = 0.0;
#pragma unroll
        for (int bb = 0; bb < 6; ++bb) t += Lm[6 * a + bb] * J[6 * bb + cc];
        LJ[6 * a + cc] = t;
      }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) {
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) t += J[6 * a + r] * LJ[6 * a + cc];
        out[36 + 6 * r + cc] = l * t;
      }
      double t = 0.0;
#pragma unroll
      for (int a = 0; a < 6; ++a) t += J[6 * a + r] * Lz[a];
      out[72 + r] = l * t;
    }
#pragma unroll
    for (int e2 = 0; e2 < 36; ++e2) out[e2] = J[e2];
  }
  const double r = wg_sum(g.ma, sh, [&](int c) { return ev[c]; });   // (its barriers also publish JM)
  for (int x = tid; x < N6 * N6; x += kThreads) H[x] = 0.0;
  __syncthreads();
  // entry (rr, cc) of every block of block row v has one owner, which walks v's incident edges in edge order
  for (int it = tid; it < g.n * 36; it += kThreads) {
    const int v = it / 36, rr = (it % 36) / 6, cc = it % 6;
    double* row = H + (size_t)(6 * v + rr) * N6;
    for (int x = nl0[g.node0 + v]; x < nl0[g.node0 + v + 1]; ++x) {
      const NodeEdge ne = list[x];
      if (!alive[ne.edge]) continue;
      const double mk = JM[78 * (size_t)ne.edge + 36 + 6 * rr + cc];
      row[6 * v + cc] += mk;
      row[6 * ne.other + cc] -= mk;
    }
  }
  for (int it = tid; it < N6; it += kThreads) {
    const int v = it / 6, rr = it % 6;
    double a = 0.0;
    for (int x = nl0[g.node0 + v]; x < nl0[g.node0 + v + 1]; ++x) {
      const NodeEdge ne = list[x];
      if (!alive[ne.edge]) continue;
      const double gk = JM[78 * (size_t)ne.edge + 72 + rr];
      a = ne.sign > 0 ? a - gk : a + gk;
    }
    b[it] = a;
  }
  __syncthreads();
  if (g.ref >= 0) {
    for (int x = tid; x < 6 * N6; x += kThreads) {
      const int rr = x / N6, cc = x % N6;                // row 6 ref + rr, column cc; and the mirrored entry
      const double val = (cc == 6 * g.ref + rr) ? 1.0 : 0.0;
      H[(size_t)(6 * g.ref + rr) * N6 + cc] = val;
      H[(size_t)cc * N6 + 6 * g.ref + rr] = val;
    }
    if (tid < 6) b[6 * g.ref + tid] = 0.0;
    __syncthreads();
  }
  return r;
}

// L <- H + lambda I, factored in place as L D L^T (unit L below the diagonal, D on it), right-looking, kPanel columns at a time:
// element (i, j) takes its subtractions L[i][p] * (d[p] * L[j][p]) one by one in increasing p, as the unblocked form does.
// Then delta <- the solution of (L D L^T) delta = b.  false: a pivot was not finite or not positive.
GMF_DEVINL bool factor_solve(int N6, const double* H, double lambda, double* L, const double* b, double* delta, double* pan) {
  const int tid = threadIdx.x;
  for (int x = tid; x < N6 * N6; x += kThreads) {
    const int i = x / N6, j = x % N6;
    L[x] = H[x] + (i == j ? lambda : 0.0);
  }
  __syncthreads();
  __shared__ double dpan[kPanel];
  for (int k0 = 0; k0 < N6; k0 += kPanel) {
    const int nb = min(kPanel, N6 - k0);
    // the panel's columns, one after the other: column k's rows below the diagonal have one owner each
    for (int p = 0; p < nb; ++p) {
      const int k = k0 + p;
      const double d = L[(size_t)k * N6 + k];
      if (!(d > 0.0) || !isfinite(d)) return false;      // (uniform: every thread reads the same word)
      for (int i = k + 1 + tid; i < N6; i += kThreads) {
        const double c = L[(size_t)i * N6 + k];
        const double lik = c / d;
        L[(size_t)i * N6 + k] = lik;
        pan[(size_t)(i - k0) * kPanel + p] = lik;
      }
      if (tid == 0) dpan[p] = d;
      __syncthreads();
      // the rest of the panel's columns take column k now (their rows i > k)
      for (int x = tid; x < (N6 - k - 1) * (nb - p - 1); x += kThreads) {
        const int i = k + 1 + x / (nb - p - 1), j = k + 1 + x % (nb - p - 1);
        if (j <= i) L[(size_t)i * N6 + j] -= pan[(size_t)(i - k0) * kPanel + p] * (d * pan[(size_t)(j - k0) * kPanel + p]);
      }
      __syncthreads();
    }
    // trailing update: rows i >= k0 + nb, columns k0 + nb <= j <= i; one wave per row, lanes along j
    const int t0 = k0 + nb;
    for (int i = t0 + (tid >> 6); i < N6; i += kThreads / 64) {
      double li[kPanel];
#pragma unroll
      for (int p = 0; p < kPanel; ++p) li[p] = p < nb ? pan[(size_t)(i - k0) * kPanel + p] : 0.0;
      for (int j = t0 + (tid & 63); j <= i; j += 64) {
        double a = L[(size_t)i * N6 + j];
        for (int p = 0; p < nb; ++p) a -= li[p] * (dpan[p] * pan[(size_t)(j - k0) * kPanel + p]);
        L[(size_t)i * N6 + j] = a;
      }
    }
    __syncthreads();
  }
  // forward, diagonal, backward: column-oriented, every element has one owner and takes its subtractions in order
  for (int i = tid; i < N6; i += kThreads) delta[i] = b[i];
  __syncthreads();
  for (int j = 0; j < N6; ++j) {
    const double yj = delta[j];
    for (int i = j + 1 + tid; i < N6; i += kThreads) delta[i] -= L[(size_t)i * N6 + j] * yj;
    __syncthreads();
  }
  for (int i = tid; i < N6; i += kThreads) delta[i] = delta[i] / L[(size_t)i * N6 + i];
  __syncthreads();
  for (int j = N6 - 1; j > 0; --j) {
    const double xj = delta[j];
    for (int i = tid; i < j; i += kThreads) delta[i] -= L[(size_t)j * N6 + i] * xj;
    __syncthreads();
  }
  return true;
}

__global__ void __launch_bounds__(kThreads)
k_posegraph(double* __restrict__ poses, const int* __restrict__ node_off, const int* __restrict__ edge_off,
            const long long* __restrict__ hoff, const int* __restrict__ esrc, const int* __restrict__ etgt, const double* __restrict__ X,
            const double* __restrict__ Lam, const unsigned char* __restrict__ unc, const unsigned char* __restrict__ mask,
            const int* __restrict__ nl0, const NodeEdge* __restrict__ list, PoseGraphOptions opt, PoseGraphScratch ws, int* elist_all,
            double* ev_all, double* __restrict__ lp, unsigned char* __restrict__ kept, int* __restrict__ stats,
            double* __restrict__ resid, double* __restrict__ trace, int* status, int status_bit) {
  __shared__ double pan[(size_t)kMaxDim * kPanel];
  __shared__ double sh[kThreads];
  __shared__ int ctl_sh[1];
  const int gi = blockIdx.x, tid = threadIdx.x;
  PgGraph g;
  g.node0 = node_off[gi];
  g.n = node_off[gi + 1] - g.node0;
  g.edge0 = edge_off[gi];
  g.m = edge_off[gi + 1] - g.edge0;
  g.esrc = esrc; g.etgt = etgt; g.X = X; g.Lam = Lam; g.unc = unc;
  g.p = opt.preference_loop_closure;
  g.ref = (opt.reference_node >= 0 && opt.reference_node < g.n) ? opt.reference_node : -1;
  int* elist = elist_all + g.edge0;
  double* ev = ev_all + g.edge0;
  g.elist = elist;
  const int N6 = 6 * g.n;
  double* P = poses + 16 * (size_t)g.node0;
  double* Pt = ws.trial + 16 * (size_t)g.node0;
  double* H = ws.H + hoff[gi];
  double* L = ws.L + hoff[gi];
  double* b = ws.b + 6 * (size_t)g.node0;
  double* delta = ws.delta + 6 * (size_t)g.node0;
  unsigned char* alive = ws.alive;

  for (int k = g.edge0 + tid; k < g.edge0 + g.m; k += kThreads) {
    alive[k] = mask ? (mask[k] ? 1 : 0) : 1;
    lp[k] = 0.0;
  }
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      for (int k = g.edge0 + tid; k < g.edge0 + g.m; k += kThreads) {
        if (alive[k] && unc[k] && lp[k] < opt.edge_prune_threshold) alive[k] = 0;
        if (!alive[k]) lp[k] = 0.0;
      }
      __syncthreads();
    }
    if (tid == 0) {                                      // the alive edges in edge order
      int c = 0;
      for (int k = g.edge0; k < g.edge0 + g.m; ++k)
        if (alive[k]) elist[c++] = k;
      ctl_sh[0] = c;
    }
    __syncthreads();
    g.ma = ctl_sh[0];
    __syncthreads();
    int iters = 0, rejected = 0, stop = -1;
    double r = linearise(g, P, lp, ev, ws.JM, H, b, nl0, list, alive, sh);
    double lambda = 1e-5 * wg_max(N6, sh, [&](int i) { return H[(size_t)i * N6 + i]; });
    double nu = 2.0;
    double* tr = trace ? trace + ((size_t)gi * 2 + pass) * (opt.max_iteration + 1) * 2 : nullptr;
    if (tr) {
      for (int x = tid; x < (opt.max_iteration + 1) * 2; x += kThreads) tr[x] = NAN;
      __syncthreads();
      if (tid == 0) { tr[0] = r; tr[1] = lambda; }
    }
    if (wg_max(N6, sh, [&](int i) { return fabs(b[i]); }) < opt.min_right_term) stop = kStopRightTerm;
    for (int it = 0; it < opt.max_iteration && stop < 0; ++it) {
      if (r < opt.min_residual) { stop = kStopResidual; break; }
      ++iters;
      for (int lm = 0;; ++lm) {                          // (at most max_iteration_lm rejections)
        if (!factor_solve(N6, H, lambda, L, b, delta, pan)) {
          stop = kStopPivot;
          if (tid == 0) atomicOr(status, status_bit);
          break;
        }
        __syncthreads();
        const double dn2 = wg_sum(N6, sh, [&](int i) { return delta[i] * delta[i]; });
        const double xn2 = wg_sum(g.n, sh, [&](int v) {
          double A[12], x6[6];
          load12(P + 16 * (size_t)v, A);
          vec6(A, x6);
          double s = 0.0;
#pragma unroll
          for (int a = 0; a < 6; ++a) s += x6[a] * x6[a];
          return s;
        });
        if (sqrt(dn2) < opt.min_relative_increment * (sqrt(xn2) + opt.min_relative_increment)) { stop = kStopIncrement; break; }
        for (int v = tid; v < g.n; v += kThreads) {
          double A[12], D[12], C[12];
          load12(P + 16 * (size_t)v, A);
          if (v == g.ref) {
#pragma unroll
            for (int e = 0; e < 12; ++e) C[e] = A[e];
          } else {
            mat6(delta + 6 * v, D);
            rigid_mul(D, A, C);
          }
#pragma unroll
          for (int e = 0; e < 12; ++e) Pt[16 * (size_t)v + e] = C[e];
          Pt[16 * (size_t)v + 12] = 0.0; Pt[16 * (size_t)v + 13] = 0.0; Pt[16 * (size_t)v + 14] = 0.0; Pt[16 * (size_t)v + 15] = 1.0;
        }
        __syncthreads();
        const double r2 = wg_sum(g.ma, sh, [&](int c) {
          const int k = elist[c];
          double zeta[6], A[12];
          const double q = edge_residual(g, k, Pt, zeta, A);
          const double l = lp[k];
          if (!unc[k]) return l * q;
          const double d = sqrt(l) - 1.0;
          return l * q + g.p * (d * d);
        });
        const double den = wg_sum(N6, sh, [&](int i) { return delta[i] * (lambda * delta[i] + b[i]); }) + 1e-3;
        const double rho = (r - r2) / den;
        if (rho > 0.0) {
          if (r - r2 < opt.min_relative_residual_increment * r) stop = kStopResidualIncrement;
          const double c3 = 2.0 * rho - 1.0;
          lambda = lambda * fmax(1.0 / 3.0, fmin(1.0 - c3 * c3 * c3, 2.0 / 3.0));
          nu = 2.0;
          for (int x = tid; x < 16 * g.n; x += kThreads)
            if (x / 16 != g.ref) P[x] = Pt[x];
          __syncthreads();
          r = linearise(g, P, lp, ev, ws.JM, H, b, nl0, list, alive, sh);
          if (wg_max(N6, sh, [&](int i) { return fabs(b[i]); }) < opt.min_right_term) stop = kStopRightTerm;
          break;
        }
        lambda = lambda * nu;
        nu = 2.0 * nu;
        ++rejected;
        if (lm + 1 >= opt.max_iteration_lm) { stop = kStopLmMax; break; }
      }
      if (tr && tid == 0) { tr[2 * (it + 1)] = r; tr[2 * (it + 1) + 1] = lambda; }
    }
    if (stop < 0) stop = (r < opt.min_residual) ? kStopResidual : kStopMaxIter;
    if (tid == 0) {
      int* st = stats + ((size_t)gi * 2 + pass) * kPoseGraphStats;
      st[0] = iters; st[1] = rejected; st[2] = stop; st[3] = g.ma;
      resid[gi * 2 + pass] = r;
    }
    __syncthreads();
  }
  for (int k = g.edge0 + tid; k < g.edge0 + g.m; k += kThreads) kept[k] = alive[k];
}

void posegraph_scratch_list(long long N, long long M, long long D, PoseGraphScratch& s, ArenaList& bufs) {
  bufs.add(s.H, (size_t)D);
  bufs.add(s.L, (size_t)D);
  bufs.add(s.b, (size_t)6 * N);
  bufs.add(s.delta, (size_t)6 * N);
  bufs.add(s.trial, (size_t)16 * N);
  bufs.add(s.JM, (size_t)78 * M);
  bufs.add(s.alive, (size_t)M);
  bufs.add(s.elist, (size_t)M);
  bufs.add(s.ev, (size_t)M);
}

hipError_t launch_posegraph(double* poses, const int* node_off, const int* edge_off, const long long* hoff, int G, const int* esrc,
                            const int* etgt, const double* X, const double* Lambda, const unsigned char* uncertain,
                            const unsigned char* mask, const int* node_list0, const NodeEdge* list, const PoseGraphOptions& opt,
                            const PoseGraphScratch& ws, double* line_process, unsigned char* kept, int* stats, double* resid,
                            double* trace, int* status, int status_bit, hipStream_t s) {
  hipLaunchKernelGGL(k_posegraph, dim3((unsigned)G), dim3(kThreads), 0, s, poses, node_off, edge_off, hoff, esrc, etgt, X, Lambda,
                     uncertain, mask, node_list0, list, opt, ws, ws.elist, ws.ev, line_process, kept, stats, resid, trace, status,
                     status_bit);
  return hipGetLastError();
}

}  // namespace gmf
