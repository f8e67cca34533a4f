// The launch decision of gmf_gemm_f32 (gmf_amd/csrc/gemm_plan.hpp) on its own: built by the host compiler with
// -fsanitize=address,undefined (tests/test_gemm_plan_host.py).
//  1. Reads the case table the GPU test runs (tests/golden/gemm_forms_table.txt, path in argv[1]), applies the argument checks of
//     gmf_gemm_f32 to every line, and prints one line per case: the GemmPlan fields, the k-steps of the first and of the last split,
//     and for the register-direct kernel which operand loaders run.  The test asserts from those lines that the table reaches
//     every form.
//  2. Invariants of every such plan, written out here independently of the plan code.
//  3. The same invariants over a grid of geometries, and a census of the forms that grid reaches: a form no geometry reaches
//     is printed as `unreached` (there is none today; the test asserts that).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../gmf_amd/csrc/gemm_plan.hpp"

using gmf::GemmGeom;
using gmf::GemmPlan;

static std::string g_where = "start";

#define CHECK(c)                                                                                      \
  do {                                                                                                \
    if (!(c)) {                                                                                       \
      std::printf("gemm_plan_host: %s failed (line %d) at %s\n", #c, __LINE__, g_where.c_str());      \
      return 1;                                                                                       \
    }                                                                                                 \
  } while (0)

// one table line; the columns in file order
struct Case {
  long ta, tb, M, N, K, lda, ldb, ldc, a_off, b_off, c_off, batch, sa, sb, sc, alpha2, bias, res, relu, flags;
};
constexpr int kCols = 20;

static GemmGeom geom_of(const Case& c) {
  // the buffers of the GPU test are 16-byte aligned: an operand's alignment is its offset's
  return GemmGeom{c.ta != 0, c.tb != 0, (int)c.M, (int)c.N, (int)c.K, c.lda, c.ldb, c.sa, c.sb, (int)c.batch,
                  (int)((c.a_off * 4) % 16), (int)((c.b_off * 4) % 16)};
}

static int check_plan(const GemmGeom& g, const GemmPlan& p, int wanted) {
  CHECK(p.kchunk > 0 && p.kchunk % 16 == 0);
  CHECK(p.ksplits >= 1 && p.ksplits <= wanted && wanted <= 128);                  // the workspace holds `wanted` partial tiles
  CHECK((long)(p.ksplits - 1) * p.kchunk < g.K && (long)p.ksplits * p.kchunk >= g.K);   // no empty split, none missing
  CHECK((p.bm == 128 || p.bm == 64) && (p.bn == 128 || p.bn == 64));
  if (p.bn == 64) CHECK(p.lds && p.bm == 64);                                    // k_gemm_f32 has no 64-column form
  if (p.lds) {
    // what k_gemm_lds's 16-byte fetches rely on: pieces of 4 along the contiguous dimension of each operand
    CHECK(g.a_mod16 == 0 && g.b_mod16 == 0 && g.lda % 4 == 0 && g.ldb % 4 == 0 && g.sA % 4 == 0 && g.sB % 4 == 0);
    CHECK((g.ta ? g.M : g.K) % 4 == 0 && (g.tb ? g.K : g.N) % 4 == 0 && g.K >= 4 && g.M >= 4 && g.N >= 4);
  }
  if (p.ksplits > 1) {
    CHECK(g.K >= 256 && p.kchunk >= 64);
    const long tiles = (long)((g.M + p.bm - 1) / p.bm) * ((g.N + p.bn - 1) / p.bn) * g.batch;
    CHECK(tiles < 384);
    CHECK((long)g.M * g.N * g.batch * 4 * wanted <= (48L << 20) || wanted == 1);
    CHECK(p.reduce_groups == (p.ksplits > 64 ? 16 : p.ksplits > 32 ? 8 : p.ksplits > 16 ? 4 : p.ksplits > 8 ? 2 : 1));
  } else {
    CHECK(p.reduce_groups == 0 && p.kchunk >= g.K);
  }
  return 0;
}

static std::string form_name(const GemmGeom& g, const GemmPlan& p) {
  char buf[64];
  std::snprintf(buf, sizeof buf, "%s<%c%c,%dx%d>%s", p.lds ? "lds" : "f32", g.ta ? 'T' : 'N', g.tb ? 'T' : 'N', p.bm, p.bn,
                p.ksplits > 1 ? "+splitk" : "");
  return buf;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: gemm_plan_host TABLE\n");
    return 2;
  }
  std::FILE* fh = std::fopen(argv[1], "r");
  if (!fh) {
    std::printf("gemm_plan_host: cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<Case> cases;
  char line[1024];
  while (std::fgets(line, sizeof line, fh)) {
    if (line[0] == '#' || line[0] == '\n') continue;
    long v[kCols];
    int n = 0;
    for (char* tok = std::strtok(line, " \t\n"); tok && n < kCols; tok = std::strtok(nullptr, " \t\n")) v[n++] = std::strtol(tok, nullptr, 10);
    g_where = "table line " + std::to_string(cases.size());
    CHECK(n == kCols);
    Case c;
    std::memcpy(&c, v, sizeof c);
    cases.push_back(c);
  }
  std::fclose(fh);
  static_assert(sizeof(Case) == kCols * sizeof(long), "Case is the table line");

  // ---- 1, 2: the table ----
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case& c = cases[i];
    g_where = "case " + std::to_string(i);
    // the argument checks of gmf_gemm_f32, and what the GPU test's buffers need: no overlap between batches of C
    CHECK(c.M > 0 && c.N > 0 && c.K > 0 && c.batch > 0);
    CHECK(c.lda >= (c.ta ? c.M : c.K) && c.ldb >= (c.tb ? c.K : c.N) && c.ldc >= c.N);
    CHECK(c.batch == 1 || (c.sa >= 0 && c.sb >= 0 && c.sc >= (c.M - 1) * c.ldc + c.N));
    CHECK(c.sa == 0 || c.batch == 1 || c.sa >= ((c.ta ? c.K : c.M) - 1) * c.lda + (c.ta ? c.M : c.K));
    CHECK(c.sb == 0 || c.batch == 1 || c.sb >= ((c.tb ? c.N : c.K) - 1) * c.ldb + (c.tb ? c.K : c.N));
    CHECK(c.a_off >= 0 && c.b_off >= 0 && c.c_off >= 0);
    CHECK(c.alpha2 == 2 || c.alpha2 == 1 || c.alpha2 == -4);                     // alpha = alpha2 / 2 in {1, 0.5, -2}
    CHECK(64 * c.K * 2 <= (1L << 24));                                           // integer data stays exact: |sum| <= 64 K (+ epilogue)
    const GemmGeom g = geom_of(c);
    const int wanted = gmf::gemm_ksplits_wanted(g);
    CHECK(c.batch * (long)wanted <= 65535);
    const GemmPlan p = gmf::gemm_plan(g);
    if (check_plan(g, p, wanted)) return 1;
    // a launch without a workspace never splits
    const GemmPlan p1 = gmf::gemm_plan(g, 1);
    CHECK(p1.ksplits == 1 && p1.reduce_groups == 0 && p1.lds == p.lds && p1.bm == p.bm && p1.bn == p.bn);
    const int len_first = p.ksplits > 1 ? p.kchunk : (int)c.K, len_last = (int)c.K - (p.ksplits - 1) * p.kchunk;
    // k_gemm_f32: the 16-byte loaders of the k-contiguous operand, as the kernel decides them
    const int vecA = !g.ta && g.lda % 4 == 0 && g.sA % 4 == 0 && g.a_mod16 == 0;
    const int vecB = g.tb && g.ldb % 4 == 0 && g.sB % 4 == 0 && g.b_mod16 == 0;
    // the same product as a call of its own (batch 1): 1 when it takes the same plan, so that its bits can be compared
    GemmGeom g1 = g;
    g1.batch = 1;
    const GemmPlan q = gmf::gemm_plan(g1);
    const int alone_same = q.lds == p.lds && q.bm == p.bm && q.bn == p.bn && q.ksplits == p.ksplits && q.kchunk == p.kchunk;
    std::printf("case %zu form %s lds %d bm %d bn %d ksplits %d kchunk %d groups %d wanted %d len_first %d len_last %d vecA %d vecB %d "
                "alone_same %d flags %ld\n",
                i, form_name(g, p).c_str(), p.lds ? 1 : 0, p.bm, p.bn, p.ksplits, p.kchunk, p.reduce_groups, wanted, len_first, len_last,
                vecA, vecB, alone_same, c.flags);
  }

  // ---- 3: a grid of geometries ----
  std::set<std::string> reached;
  std::set<int> groups;
  const int dims[] = {1, 3, 4, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 256, 1000, 1001, 4096};
  const int ks[] = {1, 3, 4, 15, 16, 17, 64, 100, 255, 256, 257, 260, 576, 1000, 1088, 2112, 4160, 5000, 8192, 100000};
  const int batches[] = {1, 2, 7, 96, 200, 512, 600};
  long plans = 0;
  for (int ta = 0; ta < 2; ++ta)
    for (int tb = 0; tb < 2; ++tb)
      for (int M : dims)
        for (int N : dims)
          for (int K : ks)
            for (int batch : batches)
              for (int mis = 0; mis < 2; ++mis) {
                const long lda = (ta ? M : K) + (mis ? 1 : 0), ldb = tb ? K : N;
                GemmGeom g{ta != 0, tb != 0, M, N, K, lda, ldb, (ta ? K : M) * lda, (tb ? N : K) * ldb, batch, mis ? 4 : 0, 0};
                g_where = "grid " + std::to_string(ta) + std::to_string(tb) + " " + std::to_string(M) + "x" + std::to_string(N) + "x" +
                          std::to_string(K) + " batch " + std::to_string(batch) + " mis " + std::to_string(mis);
                const int wanted = gmf::gemm_ksplits_wanted(g);
                const GemmPlan p = gmf::gemm_plan(g);
                if (check_plan(g, p, wanted)) return 1;
                reached.insert(form_name(g, p));
                groups.insert(p.reduce_groups);
                ++plans;
              }
  int unreached = 0;
  for (int lds = 0; lds < 2; ++lds)
    for (int ta = 0; ta < 2; ++ta)
      for (int tb = 0; tb < 2; ++tb)
        for (int tile = 0; tile < (lds ? 3 : 2); ++tile)
          for (int split = 0; split < 2; ++split) {
            GemmGeom g{ta != 0, tb != 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0};
            GemmPlan p{lds != 0, tile == 0 ? 128 : 64, tile == 2 ? 64 : 128, split ? 2 : 1, 16, 0};
            if (!reached.count(form_name(g, p))) {
              std::printf("unreached %s\n", form_name(g, p).c_str());
              ++unreached;
            }
          }
  for (int G : {0, 1, 2, 4, 8, 16})
    if (!groups.count(G)) {
      std::printf("unreached groups %d\n", G);
      ++unreached;
    }
  std::printf("grid plans %ld forms %zu unreached %d\n", plans, reached.size(), unreached);
  std::printf("gemm_plan_host: ok\n");
  return 0;
}
