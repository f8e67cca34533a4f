// Internal C++ launch entry points of multiway registration (posegraph_kernels.hip): the information matrices of E edges over
// F shared clouds and the pose-graph optimiser.
// Public C ABI: include/gmf_hip.h (gmf_information_matrix, gmf_posegraph_optimize).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launchers_pointcloud.hpp"
#include "posegraph_plan.hpp"

namespace gmf {

// Device scratch of one information-matrix call.
struct InfoScratch {
  KnnScratch grid;            // the hashed grid over all rows of the F clouds
  double* part;               // [n_chunks * kInfoPart] the chunks' partial sums
};
constexpr int kInfoPart = 10;   // the nine distinct sums of G^T G and the count

void info_scratch_list(long long N, long n_chunks, InfoScratch& s, ArenaList& bufs);
// cloud_off [F + 1], esrc / etgt [E], chunks, edge_chunk0 [E + 1]: device copies of the host plan.  T [E * 16] fp64.
// info [E * 36], count [E], nn [sum of the edges' source rows] or null.
hipError_t launch_information_matrix(const float* pts, const int* cloud_off, int F, long long N, const int* esrc, const int* etgt,
                                     int E, const InfoChunk* chunks, long n_chunks, const int* edge_chunk0, const double* T, float tau,
                                     const InfoScratch& ws, double* info, int* count, long long* nn, hipStream_t s);

// The criteria of one optimisation (open3d's GlobalOptimizationConvergenceCriteria and GlobalOptimizationOption).
struct PoseGraphOptions {
  int max_iteration, max_iteration_lm, reference_node;
  double min_relative_increment, min_relative_residual_increment, min_right_term, min_residual;
  double edge_prune_threshold, preference_loop_closure;
};
constexpr int kPoseGraphStats = 4;       // per graph and pass: iterations, rejected steps, stop code, edges that took part

// Device scratch of one optimisation: G graphs, N nodes and M edges in all, D = the sum over the graphs of (6 n)^2.
struct PoseGraphScratch {
  double* H;                  // [D] the normal matrix of each graph
  double* L;                  // [D] H + lambda I and then its factor
  double* b;                  // [6 N] right-hand side
  double* delta;              // [6 N]
  double* trial;              // [16 N] trial poses
  double* JM;                 // [M * 78] per edge: J_s (36), l J^T Lambda J (36), l J^T Lambda zeta (6)
  unsigned char* alive;       // [M] the edge takes part in the current pass
  int* elist;                 // [M] per graph, the alive edges in edge order
  double* ev;                 // [M] per graph, each alive edge's share of the residual, in elist's order
};
void posegraph_scratch_list(long long N, long long M, long long D, PoseGraphScratch& s, ArenaList& bufs);
// poses [16 N] in / out.  node_off, edge_off [G + 1], hoff [G + 1] (offsets into H), node_list0 [N + 1], list [2 M]: device copies
// of the host plan.  stats [G * 2 * kPoseGraphStats] int, resid [G * 2] final residual per pass,
// trace [G * 2 * (max_iteration + 1) * 2] (residual, lambda; NaN padded) or null.
hipError_t launch_posegraph(double* poses, const int* node_off, const int* edge_off, const long long* hoff, int G, const int* esrc,
                            const int* etgt, const double* X, const double* Lambda, const unsigned char* uncertain,
                            const unsigned char* mask, const int* node_list0, const NodeEdge* list, const PoseGraphOptions& opt,
                            const PoseGraphScratch& ws, double* line_process, unsigned char* kept, int* stats, double* resid,
                            double* trace, int* status, int status_bit, hipStream_t s);

}  // namespace gmf
