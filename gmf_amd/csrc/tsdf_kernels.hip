// Fragments from posed depth frames: open3d 0.9's ScalableTSDFVolume(volume_unit_resolution = 16) as the reference's
// make_fragments.py and integration.py drive it - allocate the 16^3 units the frames touch, integrate every frame into every
// unit born by then, and extract the vertices of the marching-cubes mesh.  The contract is DESIGN.md section 4o and its numpy
// restatement tests/tsdf_reference.py; this file is built with -ffp-contract=off and equals that restatement bit for bit.
//
//   allocation   one launch over the sampled pixels of all frames: the (fragment, x, y, z) keys go into an open-addressing table
//                (64-bit compare-and-swap, grid_hash.hpp's hash), the birth frame by atomicMin; then compact, sort, count, scan
//   integration  one workgroup per unit, one thread per (x, y) column: the column's 16 tsdf and weight values stay in registers
//                over the unit's whole frame loop and are written once
//   extraction   one workgroup per unit: the unit's values and a one-voxel halo of its 26 neighbours in LDS (18^3), a count
//                pass, a scan, an emit pass
//   colour       (open3d's RGB8 volume; steps 3c and 4c, tests/tsdf_color_reference.py) compile-time forms of the integration
//                and of the emit pass: 16 x 3 more accumulators per thread, and a vertex's colour from its edge's two voxels
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>

#include <algorithm>

#include "grid_hash.hpp"
#include "launchers_tsdf.hpp"

namespace gmf {
namespace {

constexpr int kThreads = 256;
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int kHalo = kTsdfRes + 2;                  // 18
constexpr int kHaloVoxels = kHalo * kHalo * kHalo;   // 5832

int blocks(long long n, int per) { return (int)((n + per - 1) / per); }

// unit indices are within +-kTsdfMaxIndex and g < kTsdfMaxFragments, so no key is all ones; ascending keys are ascending
// (fragment, x, y, z)
GMF_DEVINL unsigned long long pack_key(int g, int x, int y, int z) {
  return ((unsigned long long)g << 48) | ((unsigned long long)(x + 32768) << 32) | ((unsigned long long)(y + 32768) << 16) |
         (unsigned long long)(z + 32768);
}
GMF_DEVINL void unpack_key(unsigned long long k, int& g, int& x, int& y, int& z) {
  g = (int)(k >> 48);
  x = (int)((k >> 32) & 0xffff) - 32768;
  y = (int)((k >> 16) & 0xffff) - 32768;
  z = (int)(k & 0xffff) - 32768;
}

// the part g with off[g] <= i < off[g + 1] (parts may be empty; off[0] <= i < off[n])
GMF_DEVINL int part_of(const int* __restrict__ off, int n, int i) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// step 1 of the contract: metres, 0 = no measurement
GMF_DEVINL float depth_value(const void* __restrict__ depth, bool u16, size_t i, float scale, float trunc) {
  float d;
  if (u16) {
    d = (float)static_cast<const unsigned short*>(depth)[i] / scale;
  } else {
    d = static_cast<const float*>(depth)[i];
    if (!(d >= 0.f) || isinf(d)) d = 0.f;
  }
  return d >= trunc ? 0.f : d;
}

// slot of `key` in a table that holds it, or -1
GMF_DEVINL long long table_find(const unsigned long long* __restrict__ table, unsigned long long tmask, unsigned long long key,
                                unsigned long long h) {
  for (unsigned long long probe = 0; probe <= tmask; ++probe) {
    const unsigned long long cur = table[h];
    if (cur == key) return (long long)h;
    if (cur == kEmptyKey) return -1;
    h = (h + 1) & tmask;
  }
  return -1;
}

// ---- allocation ---------------------------------------------------------------------------------------------------------------

// counters: [0] units inserted, [1] TsdfFlag bits
GMF_DEVINL void touch_unit(int g, int x, int y, int z, int frame, unsigned long long tmask, int max_units,
                           unsigned long long* __restrict__ table, int* __restrict__ birth, int* __restrict__ counters) {
  const unsigned long long key = pack_key(g, x, y, z);
  unsigned long long h = cell_hash(g, x, y, z) & tmask;
  for (unsigned long long probe = 0; probe <= tmask; ++probe) {
    unsigned long long cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmptyKey) {
      if (__hip_atomic_load(&counters[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= max_units) break;   // -> overflow
      cur = atomicCAS(&table[h], kEmptyKey, key);
      if (cur == kEmptyKey) {
        if (atomicAdd(&counters[0], 1) >= max_units) atomicOr(&counters[1], kTsdfOverflow);
        cur = key;
      }
    }
    if (cur == key) {
      if (__hip_atomic_load(&birth[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > frame) atomicMin(&birth[h], frame);
      return;
    }
    h = (h + 1) & tmask;
  }
  atomicOr(&counters[1], kTsdfOverflow);
}

__global__ __launch_bounds__(kThreads) void k_tsdf_touch(const void* __restrict__ depth, bool u16, const double* __restrict__ poses,
                                                         const int* __restrict__ frame_off, TsdfParams p, int stride, int rows,
                                                         int cols, double unit_length, unsigned long long tmask, int max_units,
                                                         unsigned long long* __restrict__ table, int* __restrict__ birth,
                                                         int* __restrict__ counters) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long per_frame = (long long)rows * cols;
  if (t >= per_frame * p.F) return;
  const int f = (int)(t / per_frame);
  const int r = (int)(t % per_frame);
  const int i = (r / cols) * stride, j = (r % cols) * stride;
  const float d = depth_value(depth, u16, ((size_t)f * p.H + i) * p.W + j, p.depth_scale, p.depth_trunc);
  if (!(d > 0.f)) return;
  const int g = part_of(frame_off, p.G, f);
  const int frame = f - frame_off[g];
  const double z = (double)d;
  const double x = ((double)j - p.cx) * z / p.fx;
  const double y = ((double)i - p.cy) * z / p.fy;
  const double* P = poses + 16 * (size_t)f;
  int lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    const double w = ((P[4 * a] * x + P[4 * a + 1] * y) + P[4 * a + 2] * z) + P[4 * a + 3];
    const double l = floor((w - p.sdf_trunc) / unit_length), u = floor((w + p.sdf_trunc) / unit_length);
    if (!(l >= -(double)kTsdfMaxIndex && u <= (double)kTsdfMaxIndex)) {      // (a non-finite pose lands here too)
      atomicOr(&counters[1], kTsdfRange);
      return;
    }
    lo[a] = (int)l;
    hi[a] = (int)u;
  }
  for (int ux = lo[0]; ux <= hi[0]; ++ux)
    for (int uy = lo[1]; uy <= hi[1]; ++uy)
      for (int uz = lo[2]; uz <= hi[2]; ++uz) touch_unit(g, ux, uy, uz, frame, tmask, max_units, table, birth, counters);
}

// counters[2]: keys compacted
__global__ __launch_bounds__(kThreads) void k_tsdf_compact(const unsigned long long* __restrict__ table, long long T, int max_units,
                                                           unsigned long long* __restrict__ keys, int* __restrict__ counters) {
  const long long h = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (h >= T) return;
  const unsigned long long k = table[h];
  if (k == kEmptyKey) return;
  const int pos = atomicAdd(&counters[2], 1);
  if (pos < max_units) keys[pos] = k;
}

__global__ __launch_bounds__(kThreads) void k_tsdf_units(const unsigned long long* __restrict__ sorted, int max_units,
                                                         const unsigned long long* __restrict__ table, unsigned long long tmask,
                                                         const int* __restrict__ birth, int G, int* __restrict__ unit_keys,
                                                         int* __restrict__ birth_out, int* __restrict__ frag_count) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= max_units) return;
  const unsigned long long k = sorted[i];
  if (k == kEmptyKey) return;
  int g, x, y, z;
  unpack_key(k, g, x, y, z);
  unit_keys[3 * (size_t)i] = x;
  unit_keys[3 * (size_t)i + 1] = y;
  unit_keys[3 * (size_t)i + 2] = z;
  const long long h = table_find(table, tmask, k, cell_hash(g, x, y, z) & tmask);
  birth_out[i] = h >= 0 ? birth[h] : 0;
  if (g < G) atomicAdd(&frag_count[g], 1);
}

// ---- integration --------------------------------------------------------------------------------------------------------------

// one pass over the call's inputs: the depth value of every pixel, the ray length of every pixel, the extrinsics as float32;
// COLOR: also each pixel's three colour bytes as one word, R | G << 8 | B << 16, so that an update gathers one load and not three
template <bool COLOR>
__global__ __launch_bounds__(kThreads) void k_tsdf_prepare(const void* __restrict__ depth, bool u16, const double* __restrict__ poses_inv,
                                                           TsdfParams p, float* __restrict__ depth_m, float* __restrict__ pixel_scale,
                                                           float* __restrict__ extrinsic, const unsigned char* __restrict__ color,
                                                           unsigned* __restrict__ color_px) {
  const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t hw = (size_t)p.H * p.W;
  if (t < hw * p.F) {
    depth_m[t] = depth_value(depth, u16, t, p.depth_scale, p.depth_trunc);
    if constexpr (COLOR) color_px[t] = (unsigned)color[3 * t] | ((unsigned)color[3 * t + 1] << 8) | ((unsigned)color[3 * t + 2] << 16);
  }
  if (t < hw) {
    const double a = ((double)(int)(t % p.W) - p.cx) / p.fx, b = ((double)(int)(t / p.W) - p.cy) / p.fy;
    pixel_scale[t] = (float)sqrt((a * a + b * b) + 1.0);
  }
  if (t < (size_t)p.F * 12) extrinsic[t] = (float)poses_inv[16 * (t / 12) + t % 12];
}

// the frustum's four side planes through the camera centre, as unnormalised inward normals with their lengths
struct TsdfFrustum {
  float left_z, left_len;      // inside: fx q_x + left_z q_z >= 0
  float right_z, right_len;    // inside: right_z q_z - fx q_x >= 0
  float top_z, top_len;        // fy q_y + top_z q_z >= 0
  float bottom_z, bottom_len;  // bottom_z q_z - fy q_y >= 0
};

// COLOR: step 3c beside step 3 - the column's 16 x 3 colour accumulators stay in registers as tsdf and wt do; color_px [F,H,W] is
// k_tsdf_prepare's packed word per pixel, read only where the voxel is updated; color_out [U,16,16,16,3]
template <bool COLOR>
__global__ __launch_bounds__(kThreads) void k_tsdf_integrate(const float* __restrict__ depth_m, const float* __restrict__ pixel_scale,
                                                             const float* __restrict__ extrinsic, const int* __restrict__ frame_off,
                                                             const int* __restrict__ unit_keys, const int* __restrict__ unit_off,
                                                             const int* __restrict__ birth, int G, int H, int W, float fx, float fy,
                                                             float cx, float cy, double voxel_length, float neg_trunc, float inv_trunc,
                                                             float radius, TsdfFrustum fr, float* __restrict__ tsdf_out,
                                                             float* __restrict__ weight_out, const unsigned* __restrict__ color_px,
                                                             float* __restrict__ color_out) {
  const int u = blockIdx.x;
  const int g = part_of(unit_off, G, u);
  const int k0 = unit_keys[3 * (size_t)u], k1 = unit_keys[3 * (size_t)u + 1], k2 = unit_keys[3 * (size_t)u + 2];
  const int first = frame_off[g], frames = frame_off[g + 1] - first;
  const int lx = threadIdx.x >> 4, ly = threadIdx.x & 15;
  const float wx = (float)(((double)(kTsdfRes * k0 + lx) + 0.5) * voxel_length);
  const float wy = (float)(((double)(kTsdfRes * k1 + ly) + 0.5) * voxel_length);
  float wz[kTsdfRes], tsdf[kTsdfRes], wt[kTsdfRes];
  float col[COLOR ? 3 * kTsdfRes : 1];      // [z][channel], the order of color_out
#pragma unroll
  for (int z = 0; z < kTsdfRes; ++z) {
    wz[z] = (float)(((double)(kTsdfRes * k2 + z) + 0.5) * voxel_length);
    tsdf[z] = 0.f;
    wt[z] = 0.f;
    if constexpr (COLOR) col[3 * z] = col[3 * z + 1] = col[3 * z + 2] = 0.f;
  }
  // the unit's bounding sphere (centre in float32; `radius` has the slack for that and for the per-voxel rounding)
  const float sx = (float)((double)(kTsdfRes * k0 + 8) * voxel_length), sy = (float)((double)(kTsdfRes * k1 + 8) * voxel_length),
              sz = (float)((double)(kTsdfRes * k2 + 8) * voxel_length);
  const float u_hi = (float)W - 1e-4f, v_hi = (float)H - 1e-4f;
  const size_t hw = (size_t)H * W;
  for (int f = max(birth[u], 0); f < frames; ++f) {
    const float* E = extrinsic + 12 * (size_t)(first + f);             // wave-uniform: scalar loads
    const float e00 = E[0], e01 = E[1], e02 = E[2], e03 = E[3], e10 = E[4], e11 = E[5], e12 = E[6], e13 = E[7], e20 = E[8],
                e21 = E[9], e22 = E[10], e23 = E[11];
    {   // wave-uniform: the frame cannot update a voxel whose unit's sphere lies behind the camera or outside one side plane
      const float qx = ((e00 * sx + e01 * sy) + e02 * sz) + e03, qy = ((e10 * sx + e11 * sy) + e12 * sz) + e13,
                  qz = ((e20 * sx + e21 * sy) + e22 * sz) + e23;
      const float slack = radius + 1e-5f * (((fabsf(qx) + fabsf(qy)) + fabsf(qz)) + ((fabsf(sx) + fabsf(sy)) + fabsf(sz)));
      if (qz + slack <= 0.f) continue;
      if (fx * qx + fr.left_z * qz < -slack * fr.left_len) continue;
      if (fr.right_z * qz - fx * qx < -slack * fr.right_len) continue;
      if (fy * qy + fr.top_z * qz < -slack * fr.top_len) continue;
      if (fr.bottom_z * qz - fy * qy < -slack * fr.bottom_len) continue;
    }
    const float* D = depth_m + hw * (size_t)(first + f);
    const float bx = e00 * wx + e01 * wy, by = e10 * wx + e11 * wy, bz = e20 * wx + e21 * wy;
#pragma unroll
    for (int z = 0; z < kTsdfRes; ++z) {
      const float qz = (bz + e22 * wz[z]) + e23;
      if (!(qz > 0.f)) continue;
      const float qx = (bx + e02 * wz[z]) + e03, qy = (by + e12 * wz[z]) + e13;
      const float uf = ((qx * fx) / qz + cx) + 0.5f, vf = ((qy * fy) / qz + cy) + 0.5f;
      if (!(uf >= 1e-4f && uf < u_hi && vf >= 1e-4f && vf < v_hi)) continue;
      const int pix = (int)vf * W + (int)uf;
      const float d = D[pix];
      if (!(d > 0.f)) continue;
      const float sdf = (d - qz) * pixel_scale[pix];
      if (sdf > neg_trunc) {
        const float t = fminf(1.f, sdf * inv_trunc);
        tsdf[z] = (tsdf[z] * wt[z] + t) / (wt[z] + 1.f);
        if constexpr (COLOR) {
          const unsigned c = color_px[hw * (size_t)(first + f) + pix];
          col[3 * z] = (col[3 * z] * wt[z] + (float)(c & 255u)) / (wt[z] + 1.f);
          col[3 * z + 1] = (col[3 * z + 1] * wt[z] + (float)((c >> 8) & 255u)) / (wt[z] + 1.f);
          col[3 * z + 2] = (col[3 * z + 2] * wt[z] + (float)(c >> 16)) / (wt[z] + 1.f);
        }
        wt[z] = wt[z] + 1.f;
      }
    }
  }
  float4* to = reinterpret_cast<float4*>(tsdf_out + (size_t)u * kTsdfUnitVoxels + threadIdx.x * kTsdfRes);
  float4* wo = reinterpret_cast<float4*>(weight_out + (size_t)u * kTsdfUnitVoxels + threadIdx.x * kTsdfRes);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    to[q] = make_float4(tsdf[4 * q], tsdf[4 * q + 1], tsdf[4 * q + 2], tsdf[4 * q + 3]);
    wo[q] = make_float4(wt[4 * q], wt[4 * q + 1], wt[4 * q + 2], wt[4 * q + 3]);
  }
  if constexpr (COLOR) {      // the thread's 48 floats are contiguous
    float4* co = reinterpret_cast<float4*>(color_out + 3 * ((size_t)u * kTsdfUnitVoxels + threadIdx.x * kTsdfRes));
#pragma unroll
    for (int q = 0; q < 12; ++q) co[q] = make_float4(col[4 * q], col[4 * q + 1], col[4 * q + 2], col[4 * q + 3]);
  }
}

// ---- extraction ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_tsdf_index(const int* __restrict__ unit_keys, const int* __restrict__ unit_off, int G,
                                                         int U, unsigned long long tmask, unsigned long long* __restrict__ table,
                                                         int* __restrict__ unit_of) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= U) return;
  const int g = part_of(unit_off, G, i);
  const int x = unit_keys[3 * (size_t)i], y = unit_keys[3 * (size_t)i + 1], z = unit_keys[3 * (size_t)i + 2];
  const unsigned long long key = pack_key(g, x, y, z);
  unsigned long long h = cell_hash(g, x, y, z) & tmask;
  for (unsigned long long probe = 0; probe <= tmask; ++probe) {     // T >= 2 U and the keys are distinct: a slot is found
    if (atomicCAS(&table[h], kEmptyKey, key) == kEmptyKey) {
      unit_of[h] = i;
      return;
    }
    h = (h + 1) & tmask;
  }
}

GMF_DEVINL int halo_at(int x, int y, int z) { return (x * kHalo + y) * kHalo + z; }      // x, y, z in 0..17: local + 1

// all eight corners of the cube with origin (x, y, z) (halo coordinates) observed
GMF_DEVINL bool cube_observed(const float* val, int x, int y, int z) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float v = val[halo_at(x + (c >> 2), y + ((c >> 1) & 1), z + (c & 1))];
    ok = ok && v == v;
  }
  return ok;
}

// Does the edge from local voxel (lx, ly, z) along `axis` yield a vertex?  ta, tb: the tsdf at its two ends.
GMF_DEVINL bool edge_vertex(const float* val, int lx, int ly, int z, int axis, float& ta, float& tb) {
  const int x = lx + 1, y = ly + 1, zz = z + 1;
  const int a = halo_at(x, y, zz);
  ta = val[a];
  tb = val[a + (axis == 0 ? kHalo * kHalo : axis == 1 ? kHalo : 1)];
  if (!(ta == ta && tb == tb && (ta < 0.f) != (tb < 0.f))) return false;
  for (int c = 0; c < 4; ++c) {      // the four cubes around the edge
    const int dp = -(c >> 1), dq = -(c & 1);
    if (axis == 0 ? cube_observed(val, x, y + dp, zz + dq)
                  : axis == 1 ? cube_observed(val, x + dp, y, zz + dq) : cube_observed(val, x + dp, y + dq, zz))
      return true;
  }
  return false;
}

// EMIT false: count[u] = the unit's vertices.  EMIT true: they are written from start[u] on, in (local index, axis) order.
// COLOR (with EMIT): step 4c - a vertex's colour beside its position, the two ends' colours read from the volume `color`
// [U,16,16,16,3] in global memory for the crossing edges only (the far end's unit is in nbr[])
template <bool EMIT, bool COLOR>
__global__ __launch_bounds__(kThreads) void k_tsdf_extract(const int* __restrict__ unit_keys, const int* __restrict__ unit_off, int G,
                                                           const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                           unsigned long long tmask, const unsigned long long* __restrict__ table,
                                                           const int* __restrict__ unit_of, double voxel_length,
                                                           int* __restrict__ count, const int* __restrict__ start,
                                                           float* __restrict__ points, long long max_points,
                                                           const float* __restrict__ color, float* __restrict__ colors) {
  __shared__ float val[kHaloVoxels];          // tsdf of an observed voxel, NaN otherwise
  __shared__ int nbr[27];                     // the unit at offset (dx, dy, dz) in -1..1, or -1
  using Scan = hipcub::BlockScan<int, kThreads>;
  __shared__ typename Scan::TempStorage scan_tmp;
  const int u = blockIdx.x;
  const int g = part_of(unit_off, G, u);
  const int k[3] = {unit_keys[3 * (size_t)u], unit_keys[3 * (size_t)u + 1], unit_keys[3 * (size_t)u + 2]};
  if (threadIdx.x < 27) {
    const int x = k[0] + (int)threadIdx.x / 9 - 1, y = k[1] + ((int)threadIdx.x / 3) % 3 - 1, z = k[2] + (int)threadIdx.x % 3 - 1;
    int n = -1;
    if (threadIdx.x == 13) {
      n = u;
    } else if (abs(x) <= kTsdfMaxIndex && abs(y) <= kTsdfMaxIndex && abs(z) <= kTsdfMaxIndex) {
      const long long h = table_find(table, tmask, pack_key(g, x, y, z), cell_hash(g, x, y, z) & tmask);
      if (h >= 0) n = unit_of[h];
    }
    nbr[threadIdx.x] = n;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kHaloVoxels; i += kThreads) {
    const int hx = i / (kHalo * kHalo) - 1, hy = (i / kHalo) % kHalo - 1, hz = i % kHalo - 1;      // -1..16
    const int n = nbr[((hx < 0 ? 0 : hx > 15 ? 2 : 1) * 3 + (hy < 0 ? 0 : hy > 15 ? 2 : 1)) * 3 + (hz < 0 ? 0 : hz > 15 ? 2 : 1)];
    float v = __builtin_nanf("");
    if (n >= 0) {
      const size_t at = (size_t)n * kTsdfUnitVoxels + (((hx & 15) * kTsdfRes + (hy & 15)) * kTsdfRes + (hz & 15));
      if (weight[at] > 0.f) v = tsdf[at];
    }
    val[i] = v;
  }
  __syncthreads();
  const int lx = threadIdx.x >> 4, ly = threadIdx.x & 15;      // this thread's 16 voxels are consecutive local indices
  float ta, tb;
  int mine = 0, before, total;
  for (int z = 0; z < kTsdfRes; ++z)
    for (int axis = 0; axis < 3; ++axis) mine += edge_vertex(val, lx, ly, z, axis, ta, tb);
  Scan(scan_tmp).ExclusiveSum(mine, before, total);
  if (!EMIT) {
    if (threadIdx.x == 0) count[u] = total;
    return;
  }
  long long at = (long long)start[u] + before;
  for (int z = 0; z < kTsdfRes; ++z)
    for (int axis = 0; axis < 3; ++axis) {
      if (!edge_vertex(val, lx, ly, z, axis, ta, tb)) continue;
      const double px = ((double)(kTsdfRes * k[0] + lx) + 0.5) * voxel_length, py = ((double)(kTsdfRes * k[1] + ly) + 0.5) * voxel_length,
                   pz = ((double)(kTsdfRes * k[2] + z) + 0.5) * voxel_length;
      const double da = fabs((double)ta), db = fabs((double)tb);
      const double move = (da * voxel_length) / (da + db);
      if (at < max_points) {      // (`points` holds what the counting call reported: always, unless the caller's volume changed)
        float* out = points + 3 * (size_t)at;
        out[0] = (float)(axis == 0 ? px + move : px);
        out[1] = (float)(axis == 1 ? py + move : py);
        out[2] = (float)(axis == 2 ? pz + move : pz);
        if constexpr (COLOR) {
          const int bx = lx + (axis == 0), by = ly + (axis == 1), bz = z + (axis == 2);      // 0..16: 16 is the next unit's 0
          const int n = nbr[((1 + (bx >> 4)) * 3 + (1 + (by >> 4))) * 3 + (1 + (bz >> 4))];
          const float* ca = color + 3 * ((size_t)u * kTsdfUnitVoxels + ((lx * kTsdfRes + ly) * kTsdfRes + z));
          const float* cb = color + 3 * ((size_t)max(n, 0) * kTsdfUnitVoxels + (((bx & 15) * kTsdfRes + (by & 15)) * kTsdfRes + (bz & 15)));
          float* cout = colors + 3 * (size_t)at;
#pragma unroll
          for (int c = 0; c < 3; ++c) cout[c] = (float)((((db * (double)ca[c]) + (da * (double)cb[c])) / (da + db)) / 255.0);
        }
      }
      ++at;
    }
}

__global__ void k_tsdf_point_offsets(const int* __restrict__ unit_off, int G, const int* __restrict__ start, int* __restrict__ point_off) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g <= G) point_off[g] = start[unit_off[g]];
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------

void tsdf_alloc_scratch_list(int G, int max_units, TsdfAllocScratch& ws, ArenaList& bufs) {
  size_t sort = 0, scan = 0;
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, sort, (unsigned long long*)nullptr, (unsigned long long*)nullptr, max_units);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (int*)nullptr, (int*)nullptr, G + 1);
  ws.T = tsdf_table_slots(max_units);
  ws.tmp_bytes = sort > scan ? sort : scan;
  bufs.add(ws.table, (size_t)ws.T);
  bufs.add(ws.birth, (size_t)ws.T);
  bufs.add(ws.keys, (size_t)max_units);
  bufs.add(ws.keys_sorted, (size_t)max_units);
  bufs.add(ws.frag_count, (size_t)G + 1);
  bufs.add(ws.counters, 4);
  bufs.add(ws.tmp, ws.tmp_bytes);
}

hipError_t launch_tsdf_allocate(const void* depth, bool depth_u16, const double* poses, const int* frame_offsets, const TsdfParams& p,
                                int stride, int max_units, const TsdfAllocScratch& ws, int* unit_keys, int* birth, int* unit_offsets,
                                int* host2, hipStream_t s) {
  const unsigned long long tmask = (unsigned long long)ws.T - 1;
  hipError_t e = hipMemsetAsync(ws.table, 0xFF, ws.T * 8, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws.birth, 0x7F, ws.T * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws.keys, 0xFF, (size_t)max_units * 8, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws.frag_count, 0, ((size_t)p.G + 1) * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws.counters, 0, 16, s);
  if (e != hipSuccess) return e;
  const int rows = (p.H + stride - 1) / stride, cols = (p.W + stride - 1) / stride;
  const long long pixels = (long long)rows * cols * p.F;
  if (pixels > 0)
    k_tsdf_touch<<<blocks(pixels, kThreads), kThreads, 0, s>>>(depth, depth_u16, poses, frame_offsets, p, stride, rows, cols,
                                                              kTsdfRes * p.voxel_length, tmask, max_units, ws.table, ws.birth,
                                                              ws.counters);
  k_tsdf_compact<<<blocks(ws.T, kThreads), kThreads, 0, s>>>(ws.table, ws.T, max_units, ws.keys, ws.counters);
  size_t tb = ws.tmp_bytes;
  e = hipcub::DeviceRadixSort::SortKeys(ws.tmp, tb, ws.keys, ws.keys_sorted, max_units, 0, 64, s);
  if (e != hipSuccess) return e;
  k_tsdf_units<<<blocks(max_units, kThreads), kThreads, 0, s>>>(ws.keys_sorted, max_units, ws.table, tmask, ws.birth, p.G, unit_keys,
                                                               birth, ws.frag_count);
  tb = ws.tmp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(ws.tmp, tb, ws.frag_count, unit_offsets, p.G + 1, s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host2, ws.counters, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e;
}

hipError_t launch_tsdf_integrate(const void* depth, bool depth_u16, const unsigned char* color, const double* poses_inv,
                                 const int* frame_offsets, const TsdfParams& p, const int* unit_keys, const int* unit_offsets,
                                 const int* birth, int U, const TsdfIntegrateScratch& ws, float* tsdf, float* weight, float* color_out,
                                 hipStream_t s) {
  const size_t pixels = (size_t)p.F * p.H * p.W;
  const size_t work = std::max(pixels, std::max((size_t)p.H * p.W, (size_t)p.F * 12));      // the three tables share one launch
  if (color)
    k_tsdf_prepare<true><<<blocks((long long)work, kThreads), kThreads, 0, s>>>(depth, depth_u16, poses_inv, p, ws.depth_m,
                                                                               ws.pixel_scale, ws.extrinsic, color, ws.color_px);
  else
    k_tsdf_prepare<false><<<blocks((long long)work, kThreads), kThreads, 0, s>>>(depth, depth_u16, poses_inv, p, ws.depth_m,
                                                                                ws.pixel_scale, ws.extrinsic, nullptr, nullptr);
  const float fx = (float)p.fx, fy = (float)p.fy, cx = (float)p.cx, cy = (float)p.cy;
  const float trunc = (float)p.sdf_trunc;
  TsdfFrustum fr;
  fr.left_z = cx + 0.5f;
  fr.right_z = (float)p.W - cx - 0.5f;
  fr.top_z = cy + 0.5f;
  fr.bottom_z = (float)p.H - cy - 0.5f;
  fr.left_len = sqrtf(fx * fx + fr.left_z * fr.left_z);
  fr.right_len = sqrtf(fx * fx + fr.right_z * fr.right_z);
  fr.top_len = sqrtf(fy * fy + fr.top_z * fr.top_z);
  fr.bottom_len = sqrtf(fy * fy + fr.bottom_z * fr.bottom_z);
  // half the unit's diagonal is 0.866 unit lengths; the rest is slack for the rounding of the test itself
  const float radius = (float)(kTsdfRes * p.voxel_length);
  if (color)
    k_tsdf_integrate<true><<<U, kThreads, 0, s>>>(ws.depth_m, ws.pixel_scale, ws.extrinsic, frame_offsets, unit_keys, unit_offsets, birth,
                                                  p.G, p.H, p.W, fx, fy, cx, cy, p.voxel_length, -trunc, 1.0f / trunc, radius, fr, tsdf,
                                                  weight, ws.color_px, color_out);
  else
    k_tsdf_integrate<false><<<U, kThreads, 0, s>>>(ws.depth_m, ws.pixel_scale, ws.extrinsic, frame_offsets, unit_keys, unit_offsets, birth,
                                                   p.G, p.H, p.W, fx, fy, cx, cy, p.voxel_length, -trunc, 1.0f / trunc, radius, fr, tsdf,
                                                   weight, nullptr, nullptr);
  return hipGetLastError();
}

void tsdf_extract_scratch_list(int U, TsdfExtractScratch& ws, ArenaList& bufs) {
  ws.T = tsdf_table_slots(U);
  ws.tmp_bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, ws.tmp_bytes, (int*)nullptr, (int*)nullptr, U + 1);
  bufs.add(ws.table, (size_t)ws.T);
  bufs.add(ws.unit_of, (size_t)ws.T);
  bufs.add(ws.count, (size_t)U + 1);
  bufs.add(ws.start, (size_t)U + 1);
  bufs.add(ws.tmp, ws.tmp_bytes);
}

hipError_t launch_tsdf_extract(const int* unit_keys, const int* unit_offsets, int G, int U, const float* tsdf, const float* weight,
                               const float* color, double voxel_length, const TsdfExtractScratch& ws, float* points, float* colors,
                               long long max_points, int* point_offsets, int* host_count, hipStream_t s) {
  const unsigned long long tmask = (unsigned long long)ws.T - 1;
  hipError_t e = hipMemsetAsync(ws.table, 0xFF, ws.T * 8, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws.count + U, 0, 4, s);
  if (e != hipSuccess) return e;
  k_tsdf_index<<<blocks(U, kThreads), kThreads, 0, s>>>(unit_keys, unit_offsets, G, U, tmask, ws.table, ws.unit_of);
  k_tsdf_extract<false, false><<<U, kThreads, 0, s>>>(unit_keys, unit_offsets, G, tsdf, weight, tmask, ws.table, ws.unit_of,
                                                      voxel_length, ws.count, nullptr, nullptr, 0, nullptr, nullptr);
  size_t tb = ws.tmp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(ws.tmp, tb, ws.count, ws.start, U + 1, s);
  if (e != hipSuccess) return e;
  k_tsdf_point_offsets<<<blocks(G + 1, 64), 64, 0, s>>>(unit_offsets, G, ws.start, point_offsets);
  if (points) {
    if (color)
      k_tsdf_extract<true, true><<<U, kThreads, 0, s>>>(unit_keys, unit_offsets, G, tsdf, weight, tmask, ws.table, ws.unit_of,
                                                        voxel_length, nullptr, ws.start, points, max_points, color, colors);
    else
      k_tsdf_extract<true, false><<<U, kThreads, 0, s>>>(unit_keys, unit_offsets, G, tsdf, weight, tmask, ws.table, ws.unit_of,
                                                         voxel_length, nullptr, ws.start, points, max_points, nullptr, nullptr);
    return hipGetLastError();
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host_count, ws.start + U, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e;
}

}  // namespace gmf
