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

// ---- the mesh: triangles and vertex normals (steps 5 and 6) ------------------------------------------------------------------
//
// k_tsdf_extract above stays as it is; these are new forms beside it, one workgroup per unit over the same 18^3 halo.
//   k_tsdf_mesh_count      vertices and triangles of every unit, and what turns (voxel, axis) into a vertex index without a hash
//                          of edges: a byte per voxel with the three "this axis yields a vertex" bits, and the unit's vertex count
//                          before each (x, y) column
//   k_tsdf_mesh_vertices   step 4's positions (and 4c's colours) with the same statements, and each vertex's normal by gather:
//                          the triangles of the up to four cubes around its edge, recomputed from the halo in ascending triangle
//                          order - no triangle list, no float atomics
//   k_tsdf_mesh_triangles  thread (x, y) emits the triangles of its 16 cube origins, consecutive in output order

// The case table (tools/gen_mc_table.py writes the rows from gmf_amd/_mc_table.py).  In constant address space: a row is one
// 16-byte load, per cube and not per entry, and the table's 4 KB stay in cache; the workgroup's LDS keeps to the halo.
__constant__ __attribute__((aligned(16))) signed char kTriTable[256][16] = {
#include "tsdf_mc_table.inc"
};

struct TriRow { unsigned long long lo, hi; };      // the 16 entries of a row; -1 (0xff) ends it
GMF_DEVINL TriRow tri_row(int cube_case) {
  const ulonglong2 r = *reinterpret_cast<const ulonglong2*>(kTriTable[cube_case]);
  return {r.x, r.y};
}
GMF_DEVINL int row_entry(const TriRow& r, int i) {      // 0..11, or -1
  return (int)(signed char)((i < 8 ? r.lo >> (8 * i) : r.hi >> (8 * (i - 8))) & 0xff);
}
GMF_DEVINL int row_triangles(const TriRow& r) {
  const unsigned long long ends = 0x8080808080808080ull;
  return (16 - __popcll(r.lo & ends) - __popcll(r.hi & ends)) / 3;
}

// cube edge e starts at the cube's origin + (code & 1, (code >> 1) & 1, (code >> 2) & 1) and runs along axis code >> 3
constexpr int kEdgeCode[12] = {0, 9, 2, 8, 4, 13, 6, 12, 16, 17, 19, 18};
constexpr unsigned long long pack_edge_codes() {
  unsigned long long v = 0;
  for (int e = 0; e < 12; ++e) v |= (unsigned long long)kEdgeCode[e] << (5 * e);
  return v;
}
constexpr unsigned long long kEdgeCodes = pack_edge_codes();
GMF_DEVINL int edge_code(int e) { return (int)((kEdgeCodes >> (5 * e)) & 31); }

// nbr[] and the halo, as k_tsdf_extract fills them
GMF_DEVINL void load_halo(const int* __restrict__ unit_keys, int u, int g, const float* __restrict__ tsdf,
                          const float* __restrict__ weight, unsigned long long tmask, const unsigned long long* __restrict__ table,
                          const int* __restrict__ unit_of, int* k, float* val, int* nbr) {
  k[0] = unit_keys[3 * (size_t)u];
  k[1] = unit_keys[3 * (size_t)u + 1];
  k[2] = unit_keys[3 * (size_t)u + 2];
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
}

// step 5's case of the cube with origin (x, y, z) (halo coordinates, 0..16), or -1 unless all eight corners are observed
GMF_DEVINL int cube_case(const float* val, int x, int y, int z) {
  int c = 0;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) {      // corner i at shift[i] = (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1)
    const float v = val[halo_at(x + (((i + 1) >> 1) & 1), y + ((i >> 1) & 1), z + (i >> 2))];
    ok = ok && v == v;
    c |= (v < 0.f ? 1 : 0) << i;
  }
  return ok ? c : -1;
}

// step 4's position of the vertex on the edge from halo voxel (hx, hy, hz) along `axis`, as the float32 that is returned
GMF_DEVINL void edge_point(const float* val, const int* k, int hx, int hy, int hz, int axis, double voxel_length, double* p) {
  const int a = halo_at(hx, hy, hz);
  const double da = fabs((double)val[a]), db = fabs((double)val[a + (axis == 0 ? kHalo * kHalo : axis == 1 ? kHalo : 1)]);
  const double move = (da * voxel_length) / (da + db);
  const double px = ((double)(kTsdfRes * k[0] + hx - 1) + 0.5) * voxel_length, py = ((double)(kTsdfRes * k[1] + hy - 1) + 0.5) * voxel_length,
               pz = ((double)(kTsdfRes * k[2] + hz - 1) + 0.5) * voxel_length;
  p[0] = (double)(float)(axis == 0 ? px + move : px);
  p[1] = (double)(float)(axis == 1 ? py + move : py);
  p[2] = (double)(float)(axis == 2 ? pz + move : pz);
}

// step 6 for the vertex on the edge from local voxel (lx, ly, z) along AXIS: the cubes around the edge in (unit, local index)
// order - the units of one workgroup's halo are listed in the order of their nbr[] slot - and of each the triangles that use the
// edge, in row order: ascending triangle index
template <int AXIS>
GMF_DEVINL void vertex_normal(const float* val, const int* k, int lx, int ly, int z, double voxel_length, float* out) {
  constexpr int P = AXIS == 0 ? 1 : 0, Q = AXIS == 2 ? 1 : 2;
  const int a[3] = {lx + 1, ly + 1, z + 1};
  int key[4], cs[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int o[3] = {a[0], a[1], a[2]};
    o[P] -= c >> 1;
    o[Q] -= c & 1;
    cs[c] = cube_case(val, o[0], o[1], o[2]);
    const int slot = ((o[0] == 0 ? 0 : 1) * 3 + (o[1] == 0 ? 0 : 1)) * 3 + (o[2] == 0 ? 0 : 1);
    const int local = (((o[0] - 1) & 15) * kTsdfRes + ((o[1] - 1) & 15)) * kTsdfRes + ((o[2] - 1) & 15);
    key[c] = cs[c] >= 0 ? slot * kTsdfUnitVoxels + local : 0x7fffffff;
  }
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int done = 0;
  for (int round = 0; round < 4; ++round) {
    int best = -1, best_key = 0x7fffffff, best_case = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (!((done >> c) & 1) && key[c] < best_key) {
        best = c;
        best_key = key[c];
        best_case = cs[c];
      }
    if (best < 0) break;
    done |= 1 << best;
    const int dp = best >> 1, dq = best & 1;
    int o[3] = {a[0], a[1], a[2]};
    o[P] -= dp;
    o[Q] -= dq;
    const int e = AXIS == 0 ? 2 * dp + 4 * dq : AXIS == 1 ? 3 - 2 * dp + 4 * dq : 8 + (dq ? 3 - dp : dp);      // this edge, in that cube
    const TriRow row = tri_row(best_case);
    for (int t = 0; t < 5; ++t) {
      const int e0 = row_entry(row, 3 * t), e1 = row_entry(row, 3 * t + 1), e2 = row_entry(row, 3 * t + 2);
      if (e0 < 0) break;
      if (e0 != e && e1 != e && e2 != e) continue;
      double pi[3], pj[3], pl[3];      // the triangle (v(e0), v(e2), v(e1))
      const int c0 = edge_code(e0), c1 = edge_code(e2), c2 = edge_code(e1);
      edge_point(val, k, o[0] + (c0 & 1), o[1] + ((c0 >> 1) & 1), o[2] + ((c0 >> 2) & 1), c0 >> 3, voxel_length, pi);
      edge_point(val, k, o[0] + (c1 & 1), o[1] + ((c1 >> 1) & 1), o[2] + ((c1 >> 2) & 1), c1 >> 3, voxel_length, pj);
      edge_point(val, k, o[0] + (c2 & 1), o[1] + ((c2 >> 1) & 1), o[2] + ((c2 >> 2) & 1), c2 >> 3, voxel_length, pl);
      const double ax = pj[0] - pi[0], ay = pj[1] - pi[1], az = pj[2] - pi[2];
      const double bx = pl[0] - pi[0], by = pl[1] - pi[1], bz = pl[2] - pi[2];
      sx = sx + (ay * bz - az * by);
      sy = sy + (az * bx - ax * bz);
      sz = sz + (ax * by - ay * bx);
    }
  }
  const double len = sqrt((sx * sx + sy * sy) + sz * sz);
  const bool good = len > 0.0 && !isinf(len);      // (a NaN fails the comparison)
  out[0] = good ? (float)(sx / len) : 0.f;
  out[1] = good ? (float)(sy / len) : 0.f;
  out[2] = good ? (float)(sz / len) : 1.f;
}

// count[u], tri_count[u]: the unit's vertices and triangles.  flags [U,4096]: bit `axis` of a voxel's byte is set when its edge
// along that axis yields a vertex.  col_before [U,256]: the unit's vertices before column (x, y).
__global__ __launch_bounds__(kThreads) void k_tsdf_mesh_count(const int* __restrict__ unit_keys, const int* __restrict__ unit_off, int G,
                                                              const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                              unsigned long long tmask, const unsigned long long* __restrict__ table,
                                                              const int* __restrict__ unit_of, int* __restrict__ count,
                                                              int* __restrict__ tri_count, unsigned char* __restrict__ flags,
                                                              int* __restrict__ col_before) {
  __shared__ float val[kHaloVoxels];
  __shared__ int nbr[27];
  using Scan = hipcub::BlockScan<int, kThreads>;
  __shared__ typename Scan::TempStorage scan_tmp;
  const int u = blockIdx.x;
  int k[3];
  load_halo(unit_keys, u, part_of(unit_off, G, u), tsdf, weight, tmask, table, unit_of, k, val, nbr);
  const int lx = threadIdx.x >> 4, ly = threadIdx.x & 15;
  float ta, tb;
  int mine = 0, tris = 0, before, total, tri_total;
  unsigned long long lo = 0, hi = 0;
  for (int z = 0; z < kTsdfRes; ++z) {
    unsigned long long bits = 0;
    for (int axis = 0; axis < 3; ++axis) bits |= (unsigned long long)edge_vertex(val, lx, ly, z, axis, ta, tb) << axis;
    mine += __popcll(bits);
    if (z < 8) lo |= bits << (8 * z); else hi |= bits << (8 * (z - 8));
    const int c = cube_case(val, lx + 1, ly + 1, z + 1);
    if (c > 0 && c < 255) tris += row_triangles(tri_row(c));
  }
  *reinterpret_cast<ulonglong2*>(flags + (size_t)u * kTsdfUnitVoxels + threadIdx.x * kTsdfRes) = make_ulonglong2(lo, hi);
  Scan(scan_tmp).ExclusiveSum(mine, before, total);
  col_before[(size_t)u * kThreads + threadIdx.x] = before;
  __syncthreads();
  Scan(scan_tmp).ExclusiveSum(tris, before, tri_total);
  if (threadIdx.x == 0) {
    count[u] = total;
    tri_count[u] = tri_total;
  }
}

// totals[0], totals[1]: the call's vertices and triangles, side by side for one read-back
__global__ void k_tsdf_mesh_offsets(const int* __restrict__ unit_off, int G, int U, const int* __restrict__ start,
                                    const int* __restrict__ tri_start, int* __restrict__ point_off, int* __restrict__ tri_off,
                                    int* __restrict__ totals) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g <= G) {
    point_off[g] = start[unit_off[g]];
    tri_off[g] = tri_start[unit_off[g]];
  }
  if (g == 0) {
    totals[0] = start[U];
    totals[1] = tri_start[U];
  }
}

// k_tsdf_extract<true, COLOR>'s vertices, by its statements, and normals [max_points,3] beside them
template <bool COLOR>
__global__ __launch_bounds__(kThreads) void k_tsdf_mesh_vertices(const int* __restrict__ unit_keys, const int* __restrict__ unit_off, int G,
                                                                 const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                 unsigned long long tmask, const unsigned long long* __restrict__ table,
                                                                 const int* __restrict__ unit_of, double voxel_length,
                                                                 const int* __restrict__ start, const int* __restrict__ col_before,
                                                                 float* __restrict__ points, float* __restrict__ normals,
                                                                 long long max_points, const float* __restrict__ color,
                                                                 float* __restrict__ colors) {
  __shared__ float val[kHaloVoxels];
  __shared__ int nbr[27];
  const int u = blockIdx.x;
  int k[3];
  load_halo(unit_keys, u, part_of(unit_off, G, u), tsdf, weight, tmask, table, unit_of, k, val, nbr);
  const int lx = threadIdx.x >> 4, ly = threadIdx.x & 15;
  float ta, tb;
  long long at = (long long)start[u] + col_before[(size_t)u * kThreads + threadIdx.x];
  for (int z = 0; z < kTsdfRes; ++z)
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
      if (!edge_vertex(val, lx, ly, z, axis, ta, tb)) continue;
      const double px = ((double)(kTsdfRes * k[0] + lx) + 0.5) * voxel_length, py = ((double)(kTsdfRes * k[1] + ly) + 0.5) * voxel_length,
                   pz = ((double)(kTsdfRes * k[2] + z) + 0.5) * voxel_length;
      const double da = fabs((double)ta), db = fabs((double)tb);
      const double move = (da * voxel_length) / (da + db);
      if (at < max_points) {
        float* out = points + 3 * (size_t)at;
        out[0] = (float)(axis == 0 ? px + move : px);
        out[1] = (float)(axis == 1 ? py + move : py);
        out[2] = (float)(axis == 2 ? pz + move : pz);
        float* nout = normals + 3 * (size_t)at;
        if (axis == 0) vertex_normal<0>(val, k, lx, ly, z, voxel_length, nout);
        else if (axis == 1) vertex_normal<1>(val, k, lx, ly, z, voxel_length, nout);
        else vertex_normal<2>(val, k, lx, ly, z, voxel_length, nout);
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

// The index, counted from the fragment's first vertex (`first`: start[] of the fragment's first unit), of the vertex on the edge
// from voxel (bx, by, bz) along `axis`; the coordinates are local to the workgroup's unit, 0..16, 16 being the next unit's 0.
GMF_DEVINL int vertex_index(const int* nbr, const unsigned char* __restrict__ flags, const int* __restrict__ col_before,
                            const int* __restrict__ start, int first, int bx, int by, int bz, int axis) {
  const int n = max(nbr[((1 + (bx >> 4)) * 3 + (1 + (by >> 4))) * 3 + (1 + (bz >> 4))], 0);      // (the voxel is observed: its unit exists)
  const int col = (bx & 15) * kTsdfRes + (by & 15), z = bz & 15;
  const ulonglong2 f = *reinterpret_cast<const ulonglong2*>(flags + (size_t)n * kTsdfUnitVoxels + col * kTsdfRes);
  const int below = z < 8 ? __popcll(f.x & ((1ull << (8 * z)) - 1)) : __popcll(f.x) + __popcll(f.y & ((1ull << (8 * (z - 8))) - 1));
  const unsigned own = (unsigned)((z < 8 ? f.x >> (8 * z) : f.y >> (8 * (z - 8))) & 7);
  return (start[n] - first) + col_before[(size_t)n * kThreads + col] + below + __popc(own & ((1u << axis) - 1));
}

// step 5: triangles [max_triangles,3], from tri_start[u] on, in (local index of the cube's origin, row) order
__global__ __launch_bounds__(kThreads) void k_tsdf_mesh_triangles(const int* __restrict__ unit_keys, const int* __restrict__ unit_off, int G,
                                                                  const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                  unsigned long long tmask, const unsigned long long* __restrict__ table,
                                                                  const int* __restrict__ unit_of, const unsigned char* __restrict__ flags,
                                                                  const int* __restrict__ col_before, const int* __restrict__ start,
                                                                  const int* __restrict__ tri_start, int* __restrict__ triangles,
                                                                  long long max_triangles) {
  __shared__ float val[kHaloVoxels];
  __shared__ int nbr[27];
  using Scan = hipcub::BlockScan<int, kThreads>;
  __shared__ typename Scan::TempStorage scan_tmp;
  const int u = blockIdx.x;
  const int g = part_of(unit_off, G, u);
  int k[3];
  load_halo(unit_keys, u, g, tsdf, weight, tmask, table, unit_of, k, val, nbr);
  const int lx = threadIdx.x >> 4, ly = threadIdx.x & 15;
  int mine = 0, before;
  for (int z = 0; z < kTsdfRes; ++z) {
    const int c = cube_case(val, lx + 1, ly + 1, z + 1);
    if (c > 0 && c < 255) mine += row_triangles(tri_row(c));
  }
  Scan(scan_tmp).ExclusiveSum(mine, before);
  const int first = start[unit_off[g]];
  long long at = (long long)tri_start[u] + before;
  for (int z = 0; z < kTsdfRes; ++z) {
    const int c = cube_case(val, lx + 1, ly + 1, z + 1);
    if (!(c > 0 && c < 255)) continue;
    const TriRow row = tri_row(c);
    for (int t = 0; t < 5; ++t) {
      const int e0 = row_entry(row, 3 * t);
      if (e0 < 0) break;
      if (at < max_triangles) {
        const int c0 = edge_code(e0), c1 = edge_code(row_entry(row, 3 * t + 2)), c2 = edge_code(row_entry(row, 3 * t + 1));
        int* out = triangles + 3 * (size_t)at;      // (v(e0), v(e2), v(e1))
        out[0] = vertex_index(nbr, flags, col_before, start, first, lx + (c0 & 1), ly + ((c0 >> 1) & 1), z + ((c0 >> 2) & 1), c0 >> 3);
        out[1] = vertex_index(nbr, flags, col_before, start, first, lx + (c1 & 1), ly + ((c1 >> 1) & 1), z + ((c1 >> 2) & 1), c1 >> 3);
        out[2] = vertex_index(nbr, flags, col_before, start, first, lx + (c2 & 1), ly + ((c2 >> 1) & 1), z + ((c2 >> 2) & 1), c2 >> 3);
      }
      ++at;
    }
  }
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

void tsdf_mesh_scratch_list(int U, TsdfMeshScratch& ws, ArenaList& bufs) {
  ws.T = tsdf_table_slots(U);
  ws.tmp_bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, ws.tmp_bytes, (int*)nullptr, (int*)nullptr, U + 1);
  bufs.add(ws.table, (size_t)ws.T);
  bufs.add(ws.unit_of, (size_t)ws.T);
  bufs.add(ws.count, (size_t)U + 1);
  bufs.add(ws.start, (size_t)U + 1);
  bufs.add(ws.tri_count, (size_t)U + 1);
  bufs.add(ws.tri_start, (size_t)U + 1);
  bufs.add(ws.flags, (size_t)U * kTsdfUnitVoxels);
  bufs.add(ws.col_before, (size_t)U * kThreads);
  bufs.add(ws.totals, 2);
  bufs.add(ws.tmp, ws.tmp_bytes);
}

hipError_t launch_tsdf_extract_mesh(const int* unit_keys, const int* unit_offsets, int G, int U, const float* tsdf, const float* weight,
                                    const float* color, double voxel_length, const TsdfMeshScratch& ws, float* points, float* normals,
                                    float* colors, long long max_points, int* triangles, long long max_triangles, int* point_offsets,
                                    int* triangle_offsets, int* host_counts, hipStream_t s) {
  const unsigned long long tmask = (unsigned long long)ws.T - 1;
  hipError_t e = hipMemsetAsync(ws.table, 0xFF, ws.T * 8, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws.count + U, 0, 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws.tri_count + U, 0, 4, s);
  if (e != hipSuccess) return e;
  k_tsdf_index<<<blocks(U, kThreads), kThreads, 0, s>>>(unit_keys, unit_offsets, G, U, tmask, ws.table, ws.unit_of);
  k_tsdf_mesh_count<<<U, kThreads, 0, s>>>(unit_keys, unit_offsets, G, tsdf, weight, tmask, ws.table, ws.unit_of, ws.count, ws.tri_count,
                                           ws.flags, ws.col_before);
  size_t tb = ws.tmp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(ws.tmp, tb, ws.count, ws.start, U + 1, s);
  tb = ws.tmp_bytes;
  if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(ws.tmp, tb, ws.tri_count, ws.tri_start, U + 1, s);
  if (e != hipSuccess) return e;
  k_tsdf_mesh_offsets<<<blocks(G + 1, 64), 64, 0, s>>>(unit_offsets, G, U, ws.start, ws.tri_start, point_offsets, triangle_offsets, ws.totals);
  if (points) {
    if (color)
      k_tsdf_mesh_vertices<true><<<U, kThreads, 0, s>>>(unit_keys, unit_offsets, G, tsdf, weight, tmask, ws.table, ws.unit_of, voxel_length,
                                                        ws.start, ws.col_before, points, normals, max_points, color, colors);
    else
      k_tsdf_mesh_vertices<false><<<U, kThreads, 0, s>>>(unit_keys, unit_offsets, G, tsdf, weight, tmask, ws.table, ws.unit_of, voxel_length,
                                                         ws.start, ws.col_before, points, normals, max_points, nullptr, nullptr);
    k_tsdf_mesh_triangles<<<U, kThreads, 0, s>>>(unit_keys, unit_offsets, G, tsdf, weight, tmask, ws.table, ws.unit_of, ws.flags,
                                                 ws.col_before, ws.start, ws.tri_start, triangles, max_triangles);
    return hipGetLastError();
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host_counts, ws.totals, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e;
}

}  // namespace gmf
