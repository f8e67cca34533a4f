// The launch plan of point-to-plane ICP's split step (solver_kernels.hip: k_icp_plane_partials, k_icp_plane_solve): every pair's
// source rows cut into parts of kIcpPlaneRows rows counted from the pair's first row, one workgroup and one partial of
// kIcpPlaneSums doubles per part.  Which rows a part holds depends on the pair alone, so a pair's partials - and every bit
// computed from them - do not depend on its neighbours in the batch or on the bound the grid was sized with.  No handle and no
// HIP here: the plan is plain host code, compiled and tested on its own (tests/abi_cpp/icp_plane_plan_host.cpp).
#pragma once
#include <stddef.h>

namespace gmf {

constexpr int kIcpPlaneRows = 512;   // R: source rows per workgroup of k_icp_plane_partials (two per thread)
constexpr int kIcpPlaneSums = 29;    // |C|, sum d^2, the 21 upper entries of A = sum J J^T (row-major), the 6 of b = sum J r

struct IcpPlanePlan {
  int parts;                         // workgroups (and partial slots) per pair: ceil(max_src / R), at least 1
  long long blocks;                  // the grid of k_icp_plane_partials: B * parts (one dimension)
  size_t partial_doubles;            // scratch: blocks * kIcpPlaneSums doubles; pair b's part p at (b * parts + p) * kIcpPlaneSums
};

// the parts that hold rows of a pair with ns source rows (the others return at once and their slots are never read)
// (constexpr: the solving kernel calls it too)
constexpr int icp_plane_pair_parts(int ns) { return ns <= 0 ? 0 : (int)(((long long)ns + kIcpPlaneRows - 1) / kIcpPlaneRows); }

// max_src: an upper bound of every pair's source rows.  false: the grid does not fit one launch dimension (2^31 - 1 blocks).
inline bool icp_plane_plan(int B, long long max_src, IcpPlanePlan& p) {
  if (B < 1 || max_src < 1 || max_src >= (1LL << 31)) return false;
  p.parts = icp_plane_pair_parts((int)max_src);
  p.blocks = (long long)B * p.parts;
  if (p.blocks >= (1LL << 31)) return false;
  p.partial_doubles = (size_t)p.blocks * kIcpPlaneSums;
  return true;
}

// the slot of pair b's part p in the scratch (in doubles)
inline size_t icp_plane_slot(const IcpPlanePlan& p, int b, int part) { return ((size_t)b * p.parts + part) * kIcpPlaneSums; }

}  // namespace gmf
