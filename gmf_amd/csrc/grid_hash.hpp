// The hashed uniform search grid's cell arithmetic, shared by the radius search (pointcloud_kernels.hip: it builds the table) and
// the grid nearest-neighbour searches of ICP and of the feature-matching RANSAC (solver_kernels.hip: they only read one).  Both must name a row's cell and slot identically.
// grid_coord rounds twice (one fp64 product, one floor) and has nothing to contract, so it gives the same integer in a
// translation unit built with or without -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#ifndef GMF_DEVINL
#define GMF_DEVINL __device__ __forceinline__
#endif

namespace gmf {

GMF_DEVINL unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// cell_hash in three steps, so that a search over a block of cells hashes x once per column and (x, y) once per row
GMF_DEVINL unsigned long long cell_hash_x(int b, long long x) {
  return mix64((unsigned long long)x * 0x9E3779B97F4A7C15ull ^ ((unsigned long long)b << 40));
}
GMF_DEVINL unsigned long long cell_hash_y(unsigned long long kx, long long y) {
  return mix64(kx ^ (unsigned long long)y * 0xC2B2AE3D27D4EB4Full);
}
GMF_DEVINL unsigned long long cell_hash_z(unsigned long long kxy, long long z) {
  return mix64(kxy ^ (unsigned long long)z * 0x165667B19E3779F9ull);
}

GMF_DEVINL unsigned long long cell_hash(int b, long long x, long long y, long long z) {
  return cell_hash_z(cell_hash_y(cell_hash_x(b, x), y), z);
}

// search-grid cell of a coordinate (clamped so that a huge or non-finite one still gives a defined integer)
GMF_DEVINL long long grid_coord(float p, double inv_h) {
  const double c = fmin(fmax(floor((double)p * inv_h), -1e15), 1e15);
  return (long long)c;
}

}  // namespace gmf
