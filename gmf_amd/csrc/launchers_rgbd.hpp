// Internal C++ launch entry points of the RGB-D odometry (rgbd_kernels.hip): image pyramids of colour and depth frames,
// z-buffered pixel correspondences and the hybrid-term Gauss-Newton iteration of open3d 0.9's compute_rgbd_odometry.
// Public C ABI: include/gmf_hip.h (gmf_rgbd_pyramids, gmf_rgbd_correspondences, gmf_rgbd_odometry).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "arena_list.hpp"

namespace gmf {

constexpr int kRgbdMaxLevels = 8;
constexpr int kRgbdPlanes = 6;                 // I, D, Idx, Idy, Ddx, Ddy
constexpr int kRgbdChunk = 2048;               // target pixels one workgroup of the walk reduces: a function of the level alone
constexpr int kRgbdSlots = 32;                 // doubles of one workgroup's partial sums (28 used, the count in the last)
constexpr int kRgbdTrace = 65;                 // doubles of one traced iteration: A 36, b 6, r2, x 6, the pose 16
constexpr size_t kRgbdMapBytes = (size_t)1 << 30;   // the correspondence maps of the pairs that run together stay below this

enum RgbdColor { kRgbdGray8 = 0, kRgbdRgb8 = 1, kRgbdFloat = 2 };

// the frames of one call and their pyramid: level l is [F,6,h_l,w_l] float32 at offset(l) of one buffer
struct RgbdShape {
  int F, H, W, levels;
  int h(int l) const { return H >> l; }
  int w(int l) const { return W >> l; }
  size_t pixels(int l) const { return (size_t)h(l) * w(l); }
  size_t offset(int l) const {
    size_t o = 0;
    for (int j = 0; j < l; ++j) o += (size_t)F * kRgbdPlanes * pixels(j);
    return o;
  }
};

struct RgbdCamera { double fx, fy, cx, cy; };

// The device buffers of one gmf_rgbd_pyramids call.
struct RgbdPyramidScratch {
  float* raw_i = nullptr;                      // [F,H,W] the intensity before the Gaussian; later the blurred level on its way down
  float* raw_d = nullptr;                      // [F,H,W] the depth in metres (NaN: no measurement) before the Gaussian
};
inline void rgbd_pyramid_scratch_list(const RgbdShape& s, RgbdPyramidScratch& ws, ArenaList& bufs) {
  bufs.add(ws.raw_i, (size_t)s.F * s.H * s.W);
  bufs.add(ws.raw_d, (size_t)s.F * s.H * s.W);
}

// color [F,H,W] uint8, [F,H,W,3] uint8 or [F,H,W] float32; depth [F,H,W] uint16 or float32.  Out: every level of `planes`.
// 3 + 4 per level launches, no host synchronisation.
hipError_t launch_rgbd_pyramids(const void* color, int color_kind, const void* depth, bool depth_u16, const RgbdShape& s,
                                float depth_scale, float depth_trunc, float min_depth, float max_depth,
                                const RgbdPyramidScratch& ws, float* planes, hipStream_t st);

// pairs that run together: as many as keep their level-0 maps below kRgbdMapBytes, and no more than a grid's y extent
inline int rgbd_pair_chunk(const RgbdShape& s, int E) {
  size_t fit = kRgbdMapBytes / (s.pixels(0) * 8);
  if (fit > 65535) fit = 65535;
  return (int)(fit < 1 ? 1 : fit > (size_t)E ? (size_t)E : fit);
}
inline int rgbd_walk_blocks(size_t pixels) { return (int)((pixels + kRgbdChunk - 1) / kRgbdChunk); }

// The device buffers of one gmf_rgbd_correspondences or gmf_rgbd_odometry call.
struct RgbdOdometryScratch {
  unsigned long long* map = nullptr;           // [chunk, H*W] per target pixel (float bits of d_s) << 32 | source pixel; all ones: none
  double* partial = nullptr;                   // [chunk, blocks, kRgbdSlots] per-workgroup sums of the walk
  double* pose = nullptr;                      // [chunk,16] the current T
  double* scale = nullptr;                     // [chunk,2] s_src, s_tgt
  int* failed = nullptr;                       // [chunk]
};
inline void rgbd_odometry_scratch_list(const RgbdShape& s, int E, RgbdOdometryScratch& ws, ArenaList& bufs) {
  const size_t c = (size_t)rgbd_pair_chunk(s, E);
  bufs.add(ws.map, c * s.pixels(0));
  bufs.add(ws.partial, c * rgbd_walk_blocks(s.pixels(0)) * kRgbdSlots);
  bufs.add(ws.pose, c * 16);
  bufs.add(ws.scale, c * 2);
  bufs.add(ws.failed, c);
}

// Step 4 of the contract at one level under given poses.  Out: map_out [E,h,w] int32.  A pair that names a frame outside
// 0..F-1 gets a map of -1.
hipError_t launch_rgbd_correspondences(const float* planes, const RgbdShape& s, int level, const int* pair_src, const int* pair_tgt, int E,
                                       const double* transformation, const RgbdCamera& K, double max_depth_diff,
                                       const RgbdOdometryScratch& ws, int* map_out, hipStream_t st);

// Steps 4-8.  iterations [levels] on the host, coarsest level first.  Out: success [E] (bytes 0/1), transformation [E,16],
// information [E,36]; optionally scales [E,2], trace_n [E,sum iterations] and trace [E,sum iterations,kRgbdTrace], of which an
// iteration that does not run (a failed pair) writes nothing.  3 launches per iteration, no host synchronisation.
hipError_t launch_rgbd_odometry(const float* planes, const RgbdShape& s, const int* pair_src, const int* pair_tgt, int E,
                                const double* odo_init, const RgbdCamera& K, double max_depth_diff, const int* iterations,
                                const RgbdOdometryScratch& ws, unsigned char* success, double* transformation, double* information,
                                double* scales, int* trace_n, double* trace, hipStream_t st);

}  // namespace gmf
