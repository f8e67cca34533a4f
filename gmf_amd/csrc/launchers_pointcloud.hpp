// Internal C++ launch entry points of the point-cloud descriptor kernels (pointcloud_kernels.hip): radius-bounded kNN on a
// hashed grid, normals, colour gradients, FPFH and the two voxel grids.
// Public C ABI: include/gmf_hip.h (gmf_radius_knn, gmf_estimate_normals, gmf_color_gradients, gmf_compute_fpfh,
// gmf_voxel_down_sample, gmf_voxel_down_sample_color, gmf_voxel_select).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "arena_list.hpp"

namespace gmf {

constexpr int kKnnMaxNN = 256;      // largest max_nn of the radius search (the per-wave LDS survivor buffer)

// Device scratch of one radius search (taken from the handle's workspace by the caller).  The table has T = the next power of
// two >= 2N slots (N = all rows of the batch), fixed by N alone.
struct KnnScratch {
  long long T;                // table slots
  int* slot;                  // [N] slot of each row's cell
  int* cnt;                   // [T + 1] rows per slot (zeroed; the scatter counts it back down)
  int* start;                 // [T + 1] exclusive scan of cnt: slot s holds rows start[s] .. start[s+1)
  float4* cell_pts;           // [N] the rows in slot order, .w = the row's index (bits)
  char* scan_tmp;             // hipcub scan storage
  size_t scan_bytes;
};

// Appends the scratch of a search over N rows to a call's workspace list (arena_carve then fills the pointers); T and
// scan_bytes are set here.
void knn_scratch_list(long long N, KnnScratch& s, ArenaList& bufs);
// The table alone, for a search of one's own (ICP's, solver_kernels.hip): one memset, k_grid_count, the scan, k_grid_scatter.
// h: the cell edge; the slot of a row is cell_hash(its cloud, its cell) & (T - 1) (grid_hash.hpp).  Fills start and cell_pts.
hipError_t launch_grid_build(const float* pts, const int* offsets, int B, long long N, double h, const KnnScratch& ws,
                             hipStream_t s);
// idx [N, max_nn] (row within its cloud, -1 padding), d2 [N, max_nn] (fp64, 0 padding; may be null), count [N].
hipError_t launch_radius_knn(const float* pts, const int* offsets, int B, long long N, double radius, int max_nn,
                             const KnnScratch& ws, int* idx, double* d2, int* count, hipStream_t s);
hipError_t launch_normals(const float* pts, const int* offsets, int B, long long N, const int* idx, const int* count,
                          int max_nn, float* normals, hipStream_t s);
// open3d's InitializePointCloudForColoredICP over the lists of launch_radius_knn: intensity [N], gradients [N, 3].
hipError_t launch_color_gradient(const float* pts, const float* normals, const float* intensity, const int* offsets, int B,
                                 long long N, const int* idx, const int* count, int max_nn, float* gradients, hipStream_t s);
// spfh: [N, 33] fp64 scratch
hipError_t launch_fpfh(const float* pts, const float* normals, const int* offsets, int B, long long N, const int* idx,
                       const double* d2, const int* count, int max_nn, double* spfh, float* features, hipStream_t s);

// Device scratch of one voxel grid.
struct VoxelScratch {
  long long T;
  int* table;                 // [T] a row of the slot's voxel (-1: empty)
  int* rep;                   // [T] smallest row of the slot's voxel
  int* slot;                  // [N] each row's slot (-1: the row was rejected)
  int* head;                  // [N + 1] 1 = the row is its voxel's smallest
  int* vid;                   // [N + 1] exclusive scan of head: dense voxel id of a head row, voxel count at [N]
  unsigned long long* key;    // [N] (voxel id << 32 | row) of every row
  unsigned long long* key_sorted;
  int* vstart;                // [N + 1] first sorted position of each voxel
  double* lo;                 // [B * 3] voxel grid origin of each cloud
  int* flag;                  // [1] nonzero: a voxel index outside int32, or a non-finite coordinate
  char* tmp;                  // hipcub scan / sort storage
  size_t tmp_bytes;
};

// Appends the scratch of a voxel grid over N rows of B clouds to a call's workspace list; T and tmp_bytes are set here.
void voxel_scratch_list(long long N, int B, VoxelScratch& s, ArenaList& bufs);
// mean = true: voxel_down_sample (origin min - v/2, out_pts [nv, 3] the fp64 means stored as fp32); false: voxel_select
// (origin 0, out_idx [nv] the smallest row of each voxel, within its cloud).  out_offsets [B + 1].  Writes the voxel count and
// the range flag to `host2` after synchronising the stream.  colors [N, 3] (mean only, may be null): out_colors [nv, 3] is the
// fp64 mean of each voxel's colours over the same rows in the same order, stored as fp32 (open3d's AccumulatedPoint).
hipError_t launch_voxel(const float* pts, const int* offsets, int B, long long N, double voxel, bool mean,
                        const VoxelScratch& ws, float* out_pts, int* out_idx, int* out_offsets, int* host2, hipStream_t s,
                        const float* colors = nullptr, float* out_colors = nullptr);

}  // namespace gmf
