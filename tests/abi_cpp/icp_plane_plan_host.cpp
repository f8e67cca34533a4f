// The launch plan of point-to-plane ICP's split step (gmf_amd/csrc/icp_plane_plan.hpp) on its own: built by the host compiler
// with -fsanitize=address,undefined (tests/test_icp_plane_host.py).  Over ragged batches with sizes around R and around the
// workgroup's 256 threads: a pair's parts tile its rows exactly, a part beyond them owns none, every (pair, part) has a slot of
// its own inside the scratch, and neither a pair's parts nor their rows move with the batch or with the bound given.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gmf_amd/csrc/icp_plane_plan.hpp"

#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c)) {                                                              \
      std::printf("icp_plane_plan_host: %s failed (line %d)\n", #c, __LINE__); \
      return 1;                                                              \
    }                                                                        \
  } while (0)

constexpr int R = gmf::kIcpPlaneRows;

// what k_icp_plane_partials does with block x, on the host: the slots are written into an exactly sized malloc'ed array
static int check_batch(const std::vector<int>& ns, long long max_src) {
  const int B = (int)ns.size();
  gmf::IcpPlanePlan plan;
  CHECK(gmf::icp_plane_plan(B, max_src, plan));
  CHECK(plan.parts >= 1 && (long long)plan.parts * R >= max_src && (long long)(plan.parts - 1) * R < max_src);
  CHECK(plan.blocks == (long long)B * plan.parts);
  CHECK(plan.partial_doubles == (size_t)plan.blocks * gmf::kIcpPlaneSums);
  double* part = static_cast<double*>(std::malloc(plan.partial_doubles * sizeof(double)));
  CHECK(part);
  for (size_t i = 0; i < plan.partial_doubles; ++i) part[i] = -1.0;
  for (long long x = 0; x < plan.blocks; ++x) {
    const int b = (int)(x / plan.parts), pt = (int)(x % plan.parts);
    if ((long long)pt * R >= ns[b]) continue;                       // a part behind the pair's rows
    const int left = ns[b] - pt * R, rows = left < R ? left : R;
    CHECK(pt < gmf::icp_plane_pair_parts(ns[b]));
    double* slot = part + gmf::icp_plane_slot(plan, b, pt);
    for (int e = 0; e < gmf::kIcpPlaneSums; ++e) {
      CHECK(slot[e] == -1.0);                                       // nobody else's slot
      slot[e] = e == 0 ? rows : 0.0;
    }
  }
  // what k_icp_plane_solve reads: the pair's parts in ascending order hold all its rows, once
  for (int b = 0; b < B; ++b) {
    const int np = gmf::icp_plane_pair_parts(ns[b]);
    CHECK(np <= plan.parts);
    CHECK(np == (ns[b] + R - 1) / R);
    long long rows = 0;
    for (int p = 0; p < np; ++p) {
      const double n = part[gmf::icp_plane_slot(plan, b, p)];
      CHECK(n >= 1 && n <= R && (n == R || p + 1 == np));           // only a pair's last part is short
      rows += (long long)n;
    }
    CHECK(rows == ns[b]);
    for (int p = np; p < plan.parts; ++p) CHECK(part[gmf::icp_plane_slot(plan, b, p)] == -1.0);
  }
  std::free(part);
  return 0;
}

int main() {
  const std::vector<int> gpu = {1, 5, 255, 256, 257, R - 1, R, R + 1, 2 * R + 3, 40};      // the GPU test's ragged batch
  if (check_batch(gpu, 2 * R + 3)) return 1;
  if (check_batch(gpu, 7 * R)) return 1;                                  // a loose bound (device offsets: the total)
  if (check_batch({2 * R + 3}, 2 * R + 3)) return 1;                      // a pair alone
  if (check_batch({1}, 1)) return 1;
  if (check_batch({R}, R)) return 1;
  if (check_batch({R + 1, 1}, R + 1)) return 1;
  if (check_batch({50000, 3, 100000}, 100000)) return 1;
  // a pair's parts depend on its rows alone
  CHECK(gmf::icp_plane_pair_parts(0) == 0 && gmf::icp_plane_pair_parts(1) == 1 && gmf::icp_plane_pair_parts(R) == 1);
  CHECK(gmf::icp_plane_pair_parts(R + 1) == 2 && gmf::icp_plane_pair_parts(2147483647) == (2147483647LL + R - 1) / R);
  // refusals: nothing to do, or a grid that does not fit one launch dimension
  gmf::IcpPlanePlan plan;
  CHECK(!gmf::icp_plane_plan(0, 10, plan));
  CHECK(!gmf::icp_plane_plan(1, 0, plan));
  CHECK(!gmf::icp_plane_plan(1, 1LL << 31, plan));
  CHECK(gmf::icp_plane_plan(1, (1LL << 31) - 1, plan) && plan.parts == (int)(((1LL << 31) - 1 + R - 1) / R));
  CHECK(!gmf::icp_plane_plan(1 << 20, 1LL << 20, plan));                  // 2^20 pairs x 2^20 / R parts: 2^31 blocks at R = 512
  CHECK(gmf::icp_plane_plan((1 << 20) - 1, 1LL << 20, plan) && plan.blocks == ((1LL << 20) - 1) * ((1 << 20) / R));
  std::printf("icp_plane_plan_host: ok\n");
  return 0;
}
