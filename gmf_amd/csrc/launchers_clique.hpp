// Internal C++ launch entry points of the maximum-clique baseline (clique_kernels.hip).
// Public C ABI: include/gmf_hip.h (gmf_max_clique, gmf_pmc_graph).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "arena_list.hpp"

namespace gmf {

constexpr int kPmcMaxN = 8192;      // rows of one pair, at most: a vertex set is two 64-bit words per lane of one wave
constexpr int kPmcWaves = 256;      // search waves per pair: each checks the step budget before it expands a node, so the count
                                    // passes the budget by one per wave at most (gmf_amd/clique.py: STEP_SLACK)

constexpr int kPmcLocal = 384;      // a root with at most this many later neighbours is searched in LDS

enum PmcMetric { kPmcSquared = 0, kPmcLength = 1 };

// words of one bit row of the call: every pair's rows have this stride
inline int pmc_row_words(int max_n) { return (max_n + 63) / 64; }

// The device buffers of one gmf_max_clique call, listed once (arena_list.hpp).
struct PmcScratch {
  unsigned long long* bits = nullptr;      // [total_rows, ld] the graph in the caller's row order
  unsigned long long* bits2 = nullptr;     // [total_rows, ld] the graph renumbered by the degeneracy order
  int* order = nullptr;                    // [total_rows] order[p] = the row that became vertex p
  unsigned long long* hbest = nullptr;     // [B] key of the starting clique
  unsigned long long* best = nullptr;      // [B] key of the incumbent of the search
  unsigned long long* steps = nullptr;     // [B] nodes expanded
  int* next_root = nullptr;                // [B] ticket counter of the roots
  int* stopped = nullptr;                  // [B] 1: the budget ended the search
  unsigned long long* wave_key = nullptr;  // [B, kPmcWaves] key of the best clique each wave recorded
  unsigned short* wave_best = nullptr;     // [B, kPmcWaves, max_n] its members
};
inline void pmc_scratch_list(int B, long long total_rows, int max_n, PmcScratch& ws, ArenaList& bufs) {
  const size_t ld = (size_t)pmc_row_words(max_n);
  bufs.add(ws.bits, (size_t)total_rows * ld);
  bufs.add(ws.bits2, (size_t)total_rows * ld);
  bufs.add(ws.order, (size_t)total_rows);
  bufs.add(ws.hbest, (size_t)B);
  bufs.add(ws.best, (size_t)B);
  bufs.add(ws.steps, (size_t)B);
  bufs.add(ws.next_root, (size_t)B);
  bufs.add(ws.stopped, (size_t)B);
  bufs.add(ws.wave_key, (size_t)B * kPmcWaves);
  bufs.add(ws.wave_best, (size_t)B * kPmcWaves * (size_t)max_n);
}

// corr [total_rows,6], offsets [B+1] on the device; bits [total_rows, pmc_row_words(max_n)], degree [total_rows].  One launch.
hipError_t launch_pmc_graph(const float* corr, const int* offsets, int B, long long total_rows, int max_n, float threshold,
                            int metric, unsigned long long* bits, int* degree, hipStream_t s);

// The whole call: graph, degeneracy order, starting clique, search, labels, pose.  7 launches on `s`, no host synchronisation.
// local_rows (0..kPmcLocal): roots with at most this many candidates are searched in LDS; the tree, and the clique, are the same.
hipError_t launch_max_clique(const float* corr, const float* src, const float* tgt, const int* offsets, int B, long long total_rows,
                             int max_n, float threshold, int metric, long long max_steps, int local_rows, const PmcScratch& ws,
                             float* labels, float* T_out, int* size_out, int* exact_out, long long* steps_out, int* degree_out, hipStream_t s);

}  // namespace gmf
