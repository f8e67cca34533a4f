// Host plan of a ragged batch (gmf_encoder_forward_ragged / gmf_pose_head_ragged): the per-pair table the kernels read.  Plain
// host code, no handle and no HIP: gmf_api.cpp fills a ring slot with it, and it is checked on its own
// (tests/abi_cpp/host_table_host.cpp).
#pragma once
#include <algorithm>
#include <vector>

namespace gmf {

// Ragged batches: pair b owns rows [row0, row0 + n) of the caller's packed row-major tensors ([sum n, ...]); S = int(n * ratio)
// seeds and k = min(k, n - 1) neighbours in the pose head.  The table is built on the host from the caller's per-pair sizes and
// uploaded with the call.  Kernels take a nullable pointer: null = the uniform batch [B, N, ...].  Internally every pair keeps
// a slot of tiles(max n) tiles; a pair's tiles beyond its own are neither computed nor read.
// ord [r5]: the attention grid's pair SLOT -> pair map of a ragged batch.  The attention items are dealt to the 8 XCDs in contiguous runs of
// slots (attn_item), and an item costs n^2: with the pairs in the caller's order an XCD's share of the work is whatever its four pairs
// happen to be (32 pairs with N ~ U[4000, 5500]: +-9 % around the mean, and the launch ends with the slowest XCD).  plan_pair_table
// deals the pairs to the XCD runs longest first, each to the run with the least work so far.  Results do not depend on it.
struct PairTab { int row0, n, S, k, ord, pad0, pad1, pad2; };

enum PairPlanStatus { kPairPlanOk = 0, kPairPlanEmptyPair = 1, kPairPlanTooManyRows = 2 };

// The two refusals of a ragged batch: a pair with n <= 0; 2^31 or more rows.  A caller asks before it takes somewhere to put the table.
inline PairPlanStatus check_pair_sizes(const int* n_points, int B) {
  long long rows = 0;
  for (int b = 0; b < B; ++b) {
    if (n_points[b] <= 0) return kPairPlanEmptyPair;
    rows += n_points[b];
  }
  return rows > 0x7fffffffLL ? kPairPlanTooManyRows : kPairPlanOk;
}

// The table of B pairs of n_points[b] rows -> tab[0..B); returns max n, sum n and max S.  ratio < 0: the encoder's table (S = 0,
// k unused).  A batch check_pair_sizes refuses comes back with that status and nothing written.
inline PairPlanStatus plan_pair_table(const int* n_points, int B, double ratio, int k, PairTab* tab, int* n_max, long long* n_sum,
                                      int* s_max) {
  if (const PairPlanStatus bad = check_pair_sizes(n_points, B)) return bad;
  int row = 0, nm = 0, sm = 0;
  for (int b = 0; b < B; ++b) {
    const int n = n_points[b];
    const int Sb = ratio >= 0.0 ? (int)((double)n * ratio) : 0;     // S = int(N * ratio)   PointDSC.py:244
    tab[b] = PairTab{row, n, Sb, k, b, 0, 0, 0};
    row += n;
    nm = n > nm ? n : nm;
    sm = Sb > sm ? Sb : sm;
  }
  *n_max = nm;
  *n_sum = row;
  if (s_max) *s_max = sm;
  // slot -> pair: the pairs longest first, each into the XCD run (B / 8 consecutive slots; the first B % 8 runs hold one more) with
  // the least n^2 so far that still has a free slot; within a run longest first (PairTab::ord)
  std::vector<int> by_len(B);
  for (int b = 0; b < B; ++b) by_len[b] = b;
  std::stable_sort(by_len.begin(), by_len.end(), [&](int a, int c) { return n_points[a] > n_points[c]; });
  const int runs = B < 8 ? 1 : 8;
  std::vector<std::vector<int>> run(runs);
  std::vector<double> load(runs, 0.0);
  std::vector<int> cap(runs);
  for (int r = 0; r < runs; ++r) cap[r] = B / runs + (r < B % runs ? 1 : 0);
  for (int b : by_len) {
    int best = -1;
    for (int r = 0; r < runs; ++r)
      if ((int)run[r].size() < cap[r] && (best < 0 || load[r] < load[best])) best = r;
    run[best].push_back(b);
    load[best] += (double)n_points[b] * (double)n_points[b];
  }
  int slot = 0;
  for (int r = 0; r < runs; ++r)
    for (int b : run[r]) tab[slot++].ord = b;
  return kPairPlanOk;
}

}  // namespace gmf
