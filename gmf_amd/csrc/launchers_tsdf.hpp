// Internal C++ launch entry points of the fragment builder (tsdf_kernels.hip): TSDF fusion of posed depth frames to a cloud.
// Public C ABI: include/gmf_hip.h (gmf_tsdf_allocate, gmf_tsdf_integrate, gmf_tsdf_extract, and the RGB8 forms
// gmf_tsdf_integrate_color, gmf_tsdf_extract_color; the mesh: gmf_tsdf_extract_mesh).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "arena_list.hpp"

namespace gmf {

constexpr int kTsdfRes = 16;                   // voxels along a unit's edge (open3d's volume_unit_resolution)
constexpr int kTsdfUnitVoxels = 4096;
constexpr int kTsdfMaxIndex = 32767;           // a unit index is 16 bits of the packed (fragment, x, y, z) key
constexpr int kTsdfMaxFragments = 65535;       // the fragment is the key's other 16 bits; all ones is the empty slot

enum TsdfFlag { kTsdfOverflow = 1, kTsdfRange = 2 };

// one camera and one volume per call
struct TsdfParams {
  int G, F, H, W;
  double fx, fy, cx, cy;
  double voxel_length, sdf_trunc;
  float depth_scale, depth_trunc;
};

// slots of the open-addressing table over `units` keys: a power of two, at least twice the keys
inline long long tsdf_table_slots(long long units) {
  long long t = 1024;
  while (t < 2 * units) t <<= 1;
  return t;
}

// The device buffers of one gmf_tsdf_allocate call, listed once (arena_list.hpp).
struct TsdfAllocScratch {
  long long T = 0;
  size_t tmp_bytes = 0;
  unsigned long long* table = nullptr;        // [T] packed key of the slot's unit (all ones: empty)
  int* birth = nullptr;                       // [T] smallest frame (within its fragment) that touches the slot's unit
  unsigned long long* keys = nullptr;         // [max_units] the table's keys, compacted (all ones behind the last)
  unsigned long long* keys_sorted = nullptr;  // [max_units]
  int* frag_count = nullptr;                  // [G + 1] units of each fragment (0 at [G])
  int* counters = nullptr;                    // [4] units inserted, TsdfFlag bits, units compacted
  char* tmp = nullptr;                        // hipcub sort / scan storage
};
void tsdf_alloc_scratch_list(int G, int max_units, TsdfAllocScratch& ws, ArenaList& bufs);

// depth [F,H,W] (uint16 sensor values or float32 metres), poses [F,16] camera-to-world (fp64), frame_offsets [G+1], all on the
// device.  Out: unit_keys [max_units,3], birth [max_units] (the first `units` rows are written), unit_offsets [G+1].  Writes the
// unit count and the TsdfFlag bits to host2 after synchronising the stream.
hipError_t launch_tsdf_allocate(const void* depth, bool depth_u16, const double* poses, const int* frame_offsets, const TsdfParams& p,
                                int stride, int max_units, const TsdfAllocScratch& ws, int* unit_keys, int* birth, int* unit_offsets,
                                int* host2, hipStream_t s);

// The device buffers of one gmf_tsdf_integrate or gmf_tsdf_integrate_color call.
struct TsdfIntegrateScratch {
  float* depth_m = nullptr;                   // [F,H,W] the depth value of every pixel (metres, 0: no measurement)
  float* pixel_scale = nullptr;               // [H,W] length of the pixel's ray at z = 1
  float* extrinsic = nullptr;                 // [F,12] the first three rows of each inverse pose as float32
  unsigned* color_px = nullptr;               // [F,H,W] R | G << 8 | B << 16 of every pixel (the colour call only)
};
inline void tsdf_integrate_scratch_list(const TsdfParams& p, bool color, TsdfIntegrateScratch& ws, ArenaList& bufs) {
  bufs.add(ws.depth_m, (size_t)p.F * p.H * p.W);
  bufs.add(ws.pixel_scale, (size_t)p.H * p.W);
  bufs.add(ws.extrinsic, (size_t)p.F * 12);
  if (color) bufs.add(ws.color_px, (size_t)p.F * p.H * p.W);
}

// poses_inv [F,16] world-to-camera (fp64); unit_keys [U,3], unit_offsets [G+1], birth [U] as launch_tsdf_allocate wrote them.
// Out: tsdf, weight [U,16,16,16] float32, every voxel written.  color [F,H,W,3] uint8 (null: the colour-free form, color_out is
// not touched): color_out [U,16,16,16,3] float32 as well, every voxel written.  2 launches, no host synchronisation.
hipError_t launch_tsdf_integrate(const void* depth, bool depth_u16, const unsigned char* color, const double* poses_inv,
                                 const int* frame_offsets, const TsdfParams& p, const int* unit_keys, const int* unit_offsets,
                                 const int* birth, int U, const TsdfIntegrateScratch& ws, float* tsdf, float* weight, float* color_out,
                                 hipStream_t s);

// The device buffers of one gmf_tsdf_extract call.
struct TsdfExtractScratch {
  long long T = 0;
  size_t tmp_bytes = 0;
  unsigned long long* table = nullptr;        // [T] packed key -> slot
  int* unit_of = nullptr;                     // [T] the slot's unit
  int* count = nullptr;                       // [U + 1] vertices of each unit (0 at [U])
  int* start = nullptr;                       // [U + 1] exclusive scan of count
  char* tmp = nullptr;
};
void tsdf_extract_scratch_list(int U, TsdfExtractScratch& ws, ArenaList& bufs);

// points null: counts only - point_offsets [G+1] is written and the vertex count goes to *host_count after synchronising the
// stream.  Otherwise points [max_points,3] is written as well (a vertex past max_points is dropped) and nothing is read back
// (host_count is not touched).  color [U,16,16,16,3] (null: no colours): the emitting call writes colors [max_points,3] beside
// points, under the same guard.
hipError_t launch_tsdf_extract(const int* unit_keys, const int* unit_offsets, int G, int U, const float* tsdf, const float* weight,
                               const float* color, double voxel_length, const TsdfExtractScratch& ws, float* points, float* colors,
                               long long max_points, int* point_offsets, int* host_count, hipStream_t s);

// The device buffers of one gmf_tsdf_extract_mesh call.
struct TsdfMeshScratch {
  long long T = 0;
  size_t tmp_bytes = 0;
  unsigned long long* table = nullptr;        // [T] packed key -> slot
  int* unit_of = nullptr;                     // [T] the slot's unit
  int* count = nullptr;                       // [U + 1] vertices of each unit (0 at [U])
  int* start = nullptr;                       // [U + 1] exclusive scan of count
  int* tri_count = nullptr;                   // [U + 1] triangles of each unit (0 at [U])
  int* tri_start = nullptr;                   // [U + 1] exclusive scan of tri_count
  unsigned char* flags = nullptr;             // [U,4096] bit `axis`: the voxel's edge along that axis yields a vertex
  int* col_before = nullptr;                  // [U,256] the unit's vertices before column (x, y)
  int* totals = nullptr;                      // [2] the call's vertices and triangles, read back together
  char* tmp = nullptr;
};
void tsdf_mesh_scratch_list(int U, TsdfMeshScratch& ws, ArenaList& bufs);

// The mesh of the volume.  points null: counts only - point_offsets and triangle_offsets
// [G+1] are written and the vertex and triangle counts go to host_counts[0..1] after synchronising the stream.  Otherwise points
// and normals [max_points,3], colors [max_points,3] (with `color`) and triangles [max_triangles,3] are written as well, a row past
// its cap dropped, and nothing is read back.  Triangle entries count from the fragment's first vertex.
hipError_t launch_tsdf_extract_mesh(const int* unit_keys, const int* unit_offsets, int G, int U, const float* tsdf, const float* weight,
                                    const float* color, double voxel_length, const TsdfMeshScratch& ws, float* points, float* normals,
                                    float* colors, long long max_points, int* triangles, long long max_triangles, int* point_offsets,
                                    int* triangle_offsets, int* host_counts, hipStream_t s);

}  // namespace gmf
