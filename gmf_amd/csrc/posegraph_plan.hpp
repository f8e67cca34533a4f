// The host plans of multiway registration (posegraph_kernels.hip): the chunk table of the information matrices and the per-node
// edge lists of the pose-graph optimiser.  No handle and no HIP here: plain host code, compiled and tested on its own
// (tests/abi_cpp/posegraph_plan_host.cpp).
#pragma once
#include <stddef.h>

namespace gmf {

constexpr int kInfoChunk = 256;      // source rows per chunk: 32 passes of the 8 rows a 256-thread workgroup searches at once

// rows [row0, row0 + n) of edge `edge`'s source cloud, counted from the cloud's first row, so an edge's chunks do not depend on
// the other edges of the call; out0: where the chunk's rows start in the packed nn output (edge after edge)
struct InfoChunk { int edge, row0, n, out0; };

// -1: an edge names a cloud outside [0, F); -2: more than 2^31 - 1 chunks or output rows.  Otherwise the number of chunks.
// cloud_off [F + 1] ascending row offsets, src / tgt [E] cloud indices.  *out_rows: the sum of the edges' source rows.
inline long info_chunk_count(const int* cloud_off, int F, const int* src, const int* tgt, int E, long* out_rows) {
  long n = 0, rows = 0;
  for (int e = 0; e < E; ++e) {
    if (src[e] < 0 || src[e] >= F || tgt[e] < 0 || tgt[e] >= F) return -1;
    const long ns = (long)cloud_off[src[e] + 1] - cloud_off[src[e]];
    n += (ns + kInfoChunk - 1) / kInfoChunk;
    rows += ns;
  }
  if (n >= (1L << 31) || rows >= (1L << 31)) return -2;
  *out_rows = rows;
  return n;
}

// chunks [info_chunk_count] in edge order and edge_chunk0 [E + 1]: edge e owns chunks [edge_chunk0[e], edge_chunk0[e + 1]).
// Returns the number of chunks written.
inline long info_plan_chunks(const int* cloud_off, const int* src, int E, InfoChunk* chunks, int* edge_chunk0) {
  long c = 0, out = 0;
  for (int e = 0; e < E; ++e) {
    edge_chunk0[e] = (int)c;
    const int ns = cloud_off[src[e] + 1] - cloud_off[src[e]];
    for (int r = 0; r < ns; r += kInfoChunk) {
      const int left = ns - r;
      chunks[c++] = InfoChunk{e, r, left < kInfoChunk ? left : kInfoChunk, (int)(out + r)};
    }
    out += ns;
  }
  edge_chunk0[E] = (int)c;
  return c;
}

// ---- the optimiser's per-node edge lists --------------------------------------------------------------------------------------

constexpr int kPoseGraphMaxNodes = 256;        // per graph: H is 6n x 6n fp64 in the workspace, twice
constexpr int kPoseGraphMaxEdges = 65536;      // per graph

// one incidence: edge `edge` (numbered within the call) touches the list's node; `other`: the node at its far end (within the
// graph); sign: +1 when the list's node is the edge's source, -1 when it is the target
struct NodeEdge { int edge, other, sign; };

// 0: fine; -1: offsets do not ascend from 0; -2: an edge names a node outside its graph; -3: an edge joins a node to itself;
// -4: a graph is larger than what is built.  node_off / edge_off [G + 1]; src / tgt [m] node indices within the graph.
inline int posegraph_check(const int* node_off, const int* edge_off, int G, const int* src, const int* tgt) {
  if (node_off[0] != 0 || edge_off[0] != 0) return -1;
  for (int g = 0; g < G; ++g) {
    const long n = (long)node_off[g + 1] - node_off[g], m = (long)edge_off[g + 1] - edge_off[g];
    if (n < 1 || m < 0) return -1;
    if (n > kPoseGraphMaxNodes || m > kPoseGraphMaxEdges) return -4;
    for (int k = edge_off[g]; k < edge_off[g + 1]; ++k) {
      if (src[k] < 0 || src[k] >= n || tgt[k] < 0 || tgt[k] >= n) return -2;
      if (src[k] == tgt[k]) return -3;
    }
  }
  return 0;
}

// node_list0 [total nodes + 1] and list [2 m]: node v (numbered within the call) owns list[node_list0[v] .. node_list0[v + 1]),
// its incident edges in edge order.  A counting sort, so the order inside a list is the edge order.
inline void posegraph_node_lists(const int* node_off, const int* edge_off, int G, const int* src, const int* tgt, int* node_list0,
                                 NodeEdge* list) {
  const int N = node_off[G];
  for (int v = 0; v <= N; ++v) node_list0[v] = 0;
  for (int g = 0; g < G; ++g)
    for (int k = edge_off[g]; k < edge_off[g + 1]; ++k) {
      ++node_list0[node_off[g] + src[k] + 1];
      ++node_list0[node_off[g] + tgt[k] + 1];
    }
  for (int v = 0; v < N; ++v) node_list0[v + 1] += node_list0[v];
  // fill front to back with a moving cursor kept in the table itself: shift back afterwards
  for (int g = 0; g < G; ++g)
    for (int k = edge_off[g]; k < edge_off[g + 1]; ++k) {
      const int s = node_off[g] + src[k], t = node_off[g] + tgt[k];
      list[node_list0[s]++] = NodeEdge{k, tgt[k], 1};
      list[node_list0[t]++] = NodeEdge{k, src[k], -1};
    }
  for (int v = N; v > 0; --v) node_list0[v] = node_list0[v - 1];
  node_list0[0] = 0;
}

}  // namespace gmf
