// The batched input of DGR's inlier network, built on the device.  Replaces, per training and validation
// iteration of GMF_DeepGlobalRegistration_fcgf,
//   util/pointcloud.py:83-96   get_matching_indices: the ground-truth pairs within a radius of the transformed source points
//   core/correspondence.py:14-53   find_correct_correspondence: hashed pair keys and a membership test
//   core/trainer.py:616-678   generate_inlier_input / generate_inlier_features: the [M, 7] rows and the features of the predicted pairs
// Compiled with -ffp-contract=off (Makefile): the fp64 transform and squared distance are held bitwise to a numpy restatement.
#include <hipcub/hipcub.hpp>

#include "launchers_dgr_input.hpp"

#define GMF_DEVINL __device__ __forceinline__

namespace gmf {

namespace {

constexpr int kMiThreads = 128;      // source rows of a workgroup
constexpr int kMiTile = 512;         // target points of an LDS tile (12 KiB as three fp64 planes)

// the pair whose rows hold r: the largest b < B with off[b] <= r (empty pairs share their offset with the next)
GMF_DEVINL int pair_of_row(const int* __restrict__ off, int B, long long r) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// One pass over all pairs of the batch: a thread owns one source row, a workgroup 128 consecutive rows of the packed source tensor.
// The workgroup walks the pairs its rows belong to; the target points of a pair go through LDS in tiles of 512 (as fp64) and every
// thread of that pair tests the tile in order, so a row meets its targets in ascending j.
//   p  = ((T00 x + T01 y) + T02 z) + T03 (likewise y, z), x, y, z the fp32 coordinates as fp64, T the pair's row-major fp64 4 x 4
//   d2 = ((px - qx)^2 + (py - qy)^2) + (pz - qz)^2, every operation rounded on its own;  in: d2 < r2
// FILL = false: cnt[row] = the row's count.  FILL = true: the row's pairs (i, j), local to the pair, from pairs[row_start[row]] on.
template <bool FILL>
__global__ __launch_bounds__(kMiThreads) void k_matching_indices(const float* __restrict__ xyz0, const int* __restrict__ off0,
                                                                 const float* __restrict__ xyz1, const int* __restrict__ off1, int B,
                                                                 long long N0, const double* __restrict__ T, double r2,
                                                                 int* __restrict__ cnt, const long long* __restrict__ row_start,
                                                                 long long* __restrict__ pairs) {
  __shared__ double sx[kMiTile], sy[kMiTile], sz[kMiTile];
  const long long first = (long long)blockIdx.x * kMiThreads;
  const long long r = first + threadIdx.x;
  const bool live = r < N0;
  const long long last = (first + kMiThreads < N0 ? first + kMiThreads : N0) - 1;
  const int p_first = pair_of_row(off0, B, first), p_last = pair_of_row(off0, B, last);
  const int mine = live ? pair_of_row(off0, B, r) : -1;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (live) {
    const double x = (double)xyz0[r * 3 + 0], y = (double)xyz0[r * 3 + 1], z = (double)xyz0[r * 3 + 2];
    const double* t = T + (size_t)mine * 16;
    px = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
    py = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
    pz = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
  }
  int count = 0;
  long long w = (FILL && live) ? row_start[r] : 0;
  for (int p = p_first; p <= p_last; ++p) {
    if (off0[p + 1] == off0[p]) continue;            // (uniform: an empty pair owns none of the rows)
    const int k0 = off1[p], k1 = off1[p + 1];
    const long long i_local = r - off0[p];
    for (int base = k0; base < k1; base += kMiTile) {
      const int n = k1 - base < kMiTile ? k1 - base : kMiTile;
      __syncthreads();                               // the previous tile has been read by everyone
      for (int e = threadIdx.x; e < n; e += kMiThreads) {
        const float* q = xyz1 + (size_t)(base + e) * 3;
        sx[e] = (double)q[0];
        sy[e] = (double)q[1];
        sz[e] = (double)q[2];
      }
      __syncthreads();
      if (mine == p) {
        for (int e = 0; e < n; ++e) {
          const double dx = px - sx[e], dy = py - sy[e], dz = pz - sz[e];
          const double d2 = (dx * dx + dy * dy) + dz * dz;
          if (d2 < r2) {
            if (FILL) {
              pairs[2 * w] = i_local;
              pairs[2 * w + 1] = (long long)(base - k0 + e);
              ++w;
            } else {
              ++count;
            }
          }
        }
      }
    }
  }
  if (!FILL) {
    if (live) cnt[r] = count;
    if (r == 0) cnt[N0] = 0;                         // the scan's last entry is then the number of pairs
  }
}

__global__ void k_matching_offsets(const int* __restrict__ off0, int B, const long long* __restrict__ row_start,
                                   long long* __restrict__ pair_offsets) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b <= B) pair_offsets[b] = row_start[off0[b]];
}

struct IntToLong {
  __host__ __device__ long long operator()(const int& v) const { return (long long)v; }
};
using CountIter = hipcub::TransformInputIterator<long long, IntToLong, const int*>;

// Rows [0, rb) of the grid: one thread per predicted pair m - the pair (i, j), the row cat(c0[i], c1[j, 1:]), the 'ones' / 'coords'
// features and the label (a binary search of i + j seed among the pair's sorted positive keys).  Rows [rb, ..): the 'feats'
// features, one thread per output element (coalesced rows of 2 c floats).
__global__ __launch_bounds__(256) void k_inlier_input(const InlierInput in, int rb) {
  const int blk = blockIdx.x;
  if (blk < rb) {
    const long long m = (long long)blk * 256 + threadIdx.x;
    if (m >= in.M) return;
    const int b = pair_of_row(in.off0, in.B, m);
    long long i, j;
    if (in.nn) {
      i = m - in.off0[b];
      j = in.nn[m];
      in.pred_out[2 * m] = i;
      in.pred_out[2 * m + 1] = j;
    } else {
      i = in.pred[2 * m];
      j = in.pred[2 * m + 1];
    }
    if (in.coords_out) {
      // rows of the packed source / target tensors (coords_out comes with `nn`; a match outside its pair's keys is clamped, never read)
      const long long n1 = in.off1[b + 1] - in.off1[b];
      const long long g0 = m, g1 = in.off1[b] + (j < 0 ? 0 : j >= n1 ? n1 - 1 : j);
      const int* a = in.c0 + g0 * 4;
      const int* c = in.c1 + g1 * 4;
      int* o = in.coords_out + m * 7;
      o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3];
      o[4] = c[1]; o[5] = c[2]; o[6] = c[3];
      if (in.feat_type == 0) {
        in.feats_out[m] = 1.0f;
      } else if (in.feat_type == 2) {
        // cos in fp64 of the fp32 coordinate, rounded once to fp32
        const float* p = in.a0 + g0 * 3;
        const float* q = in.a1 + g1 * 3;
        float* f = in.feats_out + m * 6;
        for (int e = 0; e < 3; ++e) {
          f[e] = (float)cos((double)p[e]);
          f[3 + e] = (float)cos((double)q[e]);
        }
      }
    }
    if (in.labels_out) {
      const unsigned long long key = (unsigned long long)i + (unsigned long long)j * (unsigned long long)in.seeds[b];   // int64, wrapping
      const long long k = (long long)key;
      long long lo = in.pos_off[b], hi = in.pos_off[b + 1];
      while (lo < hi) {                                // lower bound
        const long long mid = lo + ((hi - lo) >> 1);
        if (in.pos_keys[mid] < k) lo = mid + 1; else hi = mid;
      }
      in.labels_out[m] = (lo < in.pos_off[b + 1] && in.pos_keys[lo] == k) ? 1 : 0;
    }
    return;
  }
  const int w = 2 * in.c;
  const long long e = (long long)(blk - rb) * 256 + threadIdx.x;
  if (e >= in.M * w) return;
  const long long m = e / w;
  const int col = (int)(e - m * w);
  const int b = pair_of_row(in.off0, in.B, m);
  float v;
  if (col < in.c) {
    v = in.a0[m * in.c + col];
  } else {
    const long long n1 = in.off1[b + 1] - in.off1[b], j = in.nn[m];
    v = in.a1[(in.off1[b] + (j < 0 ? 0 : j >= n1 ? n1 - 1 : j)) * in.c + (col - in.c)];
  }
  in.feats_out[e] = v;
}

}  // namespace

size_t matching_indices_scan_bytes(long long n0) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, CountIter(nullptr, IntToLong()), (long long*)nullptr, (int)(n0 + 1));
  return bytes;
}

hipError_t launch_matching_indices_count(const float* xyz0, const int* off0, const float* xyz1, const int* off1, int B, long long n0,
                                         const double* T, double r2, int* cnt, void* scan_tmp, size_t scan_bytes, long long* row_start,
                                         long long* pair_offsets, hipStream_t s) {
  const unsigned blocks = (unsigned)((n0 + kMiThreads - 1) / kMiThreads);
  hipLaunchKernelGGL(k_matching_indices<false>, dim3(blocks), dim3(kMiThreads), 0, s, xyz0, off0, xyz1, off1, B, n0, T, r2, cnt,
                     (const long long*)nullptr, (long long*)nullptr);
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, CountIter(cnt, IntToLong()), row_start, (int)(n0 + 1), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_matching_offsets, dim3((B + 1 + 255) / 256), dim3(256), 0, s, off0, B, row_start, pair_offsets);
  return hipGetLastError();
}

hipError_t launch_matching_indices_fill(const float* xyz0, const int* off0, const float* xyz1, const int* off1, int B, long long n0,
                                        const double* T, double r2, const long long* row_start, long long* pairs, hipStream_t s) {
  const unsigned blocks = (unsigned)((n0 + kMiThreads - 1) / kMiThreads);
  hipLaunchKernelGGL(k_matching_indices<true>, dim3(blocks), dim3(kMiThreads), 0, s, xyz0, off0, xyz1, off1, B, n0, T, r2,
                     (int*)nullptr, row_start, pairs);
  return hipGetLastError();
}

hipError_t launch_inlier_input(const InlierInput& in, hipStream_t s) {
  const int rb = (int)((in.M + 255) / 256);
  const long long fe = (in.coords_out && in.feat_type == 1) ? in.M * 2 * in.c : 0;
  const int fb = (int)((fe + 255) / 256);
  hipLaunchKernelGGL(k_inlier_input, dim3(rb + fb), dim3(256), 0, s, in, rb);
  return hipGetLastError();
}

}  // namespace gmf
