// The host plans of multiway registration (gmf_amd/csrc/posegraph_plan.hpp) on their own: built by the host compiler with
// -fsanitize=address,undefined (tests/test_posegraph_host.py).  The chunk table tiles every edge's source rows exactly, in row
// order, never into another edge; the per-node edge lists hold every edge twice, in edge order, with the far node and the sign.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gmf_amd/csrc/posegraph_plan.hpp"

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::printf("posegraph_plan_host: %s failed (line %d)\n", #c, __LINE__); \
      return 1;                                                               \
    }                                                                         \
  } while (0)

static int check_chunks(const std::vector<int>& n, const std::vector<int>& src, const std::vector<int>& tgt) {
  const int F = (int)n.size(), E = (int)src.size();
  std::vector<int> off(F + 1, 0);
  for (int f = 0; f < F; ++f) off[f + 1] = off[f] + n[f];
  long rows = -1;
  const long want = gmf::info_chunk_count(off.data(), F, src.data(), tgt.data(), E, &rows);
  CHECK(want >= 0);
  // exactly `want` chunks and E + 1 entries: the sanitizer sees any write behind either
  gmf::InfoChunk* chunks = static_cast<gmf::InfoChunk*>(std::malloc(want ? want * sizeof(gmf::InfoChunk) : 1));
  int* c0 = static_cast<int*>(std::malloc((E + 1) * sizeof(int)));
  CHECK(chunks && c0);
  CHECK(gmf::info_plan_chunks(off.data(), src.data(), E, chunks, c0) == want);
  CHECK(c0[0] == 0 && c0[E] == want);
  long c = 0, out = 0;
  for (int e = 0; e < E; ++e) {
    const int ns = n[src[e]];
    CHECK(c0[e] == c);
    CHECK(c0[e + 1] - c0[e] == (ns + gmf::kInfoChunk - 1) / gmf::kInfoChunk);
    int row = 0;
    for (; c < c0[e + 1]; ++c) {
      const gmf::InfoChunk& k = chunks[c];
      CHECK(k.edge == e);
      CHECK(k.row0 == row);                                       // the edge's rows in order, no gap and no overlap
      CHECK(k.out0 == out + row);
      CHECK(k.n >= 1 && k.n <= gmf::kInfoChunk);
      CHECK(k.n == gmf::kInfoChunk || c + 1 == c0[e + 1]);         // only an edge's last chunk is short
      row += k.n;
      CHECK(row <= ns);                                           // never past the source cloud
    }
    CHECK(row == ns);
    out += ns;
  }
  CHECK(c == want && out == rows);
  std::free(chunks);
  std::free(c0);
  return 0;
}

static int check_lists(const std::vector<int>& nn, const std::vector<std::vector<int>>& es, const std::vector<std::vector<int>>& et) {
  const int G = (int)nn.size();
  std::vector<int> noff(G + 1, 0), eoff(G + 1, 0), src, tgt;
  for (int g = 0; g < G; ++g) {
    noff[g + 1] = noff[g] + nn[g];
    eoff[g + 1] = eoff[g] + (int)es[g].size();
    src.insert(src.end(), es[g].begin(), es[g].end());
    tgt.insert(tgt.end(), et[g].begin(), et[g].end());
  }
  CHECK(gmf::posegraph_check(noff.data(), eoff.data(), G, src.data(), tgt.data()) == 0);
  const int N = noff[G], M = eoff[G];
  int* l0 = static_cast<int*>(std::malloc((N + 1) * sizeof(int)));
  gmf::NodeEdge* list = static_cast<gmf::NodeEdge*>(std::malloc(M ? 2 * M * sizeof(gmf::NodeEdge) : 1));
  CHECK(l0 && list);
  gmf::posegraph_node_lists(noff.data(), eoff.data(), G, src.data(), tgt.data(), l0, list);
  CHECK(l0[0] == 0 && l0[N] == 2 * M);
  std::vector<int> seen(M, 0);
  for (int g = 0; g < G; ++g)
    for (int v = 0; v < nn[g]; ++v) {
      const int a = l0[noff[g] + v], b = l0[noff[g] + v + 1];
      CHECK(a <= b);
      for (int x = a; x < b; ++x) {
        const gmf::NodeEdge& ne = list[x];
        CHECK(ne.edge >= eoff[g] && ne.edge < eoff[g + 1]);       // an edge of this graph
        CHECK(x == a || list[x - 1].edge < ne.edge);              // in edge order, each once
        CHECK(ne.sign == 1 || ne.sign == -1);
        if (ne.sign == 1) CHECK(src[ne.edge] == v && tgt[ne.edge] == ne.other);
        else CHECK(tgt[ne.edge] == v && src[ne.edge] == ne.other);
        ++seen[ne.edge];
      }
    }
  for (int k = 0; k < M; ++k) CHECK(seen[k] == 2);
  std::free(l0);
  std::free(list);
  return 0;
}

int main() {
  if (check_chunks({1, 63, 64, 65, 257, 200}, {0, 1, 2, 3, 4, 4, 5}, {5, 5, 0, 3, 5, 0, 5})) return 1;
  if (check_chunks({700, 300, 512}, {0, 1, 2, 1, 0}, {1, 1, 1, 1, 2})) return 1;      // three chunks, a shared target, source == target
  if (check_chunks({5}, {}, {})) return 1;                                             // E = 0
  if (check_chunks({255, 256, 257, 513, 100000}, {0, 1, 2, 3, 4}, {4, 3, 2, 1, 0})) return 1;
  {
    const std::vector<int> n{4}, s{0, 7}, t{1, 0};
    std::vector<int> off{0, 4};
    long rows = 0;
    CHECK(gmf::info_chunk_count(off.data(), 1, s.data(), t.data(), 2, &rows) == -1);   // a cloud index out of range
  }
  if (check_lists({12, 2, 3}, {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 0, 2, 0, 11}, {0}, {0, 1, 0, 2}},
                  {{1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 5, 9, 11, 3}, {1}, {1, 2, 2, 0}})) return 1;
  if (check_lists({1, 3}, {{}, {0, 0}}, {{}, {1, 1}})) return 1;                       // a graph without edges, a doubled edge
  {
    const int noff[2] = {0, 3}, eoff[2] = {0, 1};
    int s = 1, t = 1;
    CHECK(gmf::posegraph_check(noff, eoff, 1, &s, &t) == -3);                          // a self loop
    t = 3;
    CHECK(gmf::posegraph_check(noff, eoff, 1, &s, &t) == -2);
    const int big[2] = {0, gmf::kPoseGraphMaxNodes + 1};
    t = 0;
    CHECK(gmf::posegraph_check(big, eoff, 1, &s, &t) == -4);
  }
  std::printf("posegraph_plan_host: ok\n");
  return 0;
}
