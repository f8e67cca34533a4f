// Host-only check of the host-table list (gmf_amd/csrc/host_table.hpp) and of the ragged batch's plan (gmf_amd/csrc/pair_plan.hpp),
// meant to be built with
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all host_table_host.cpp
// a. Lists of 1, 3, 5 and 7 parts of mixed element sizes over a malloc'ed block of exactly bytes(): every part 16-byte aligned,
//    inside the block, in list order and apart; every byte of every part is written through the typed host pointer, so an
//    under-count is a heap overflow the sanitizer reports.  The three real layouts against the offset ladders they replaced.
// b. plan_pair_table: two orders derived by hand, the sizes, the seeds, a permutation at every B, the two refusals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../gmf_amd/csrc/corr_plan.hpp"
#include "../../gmf_amd/csrc/host_table.hpp"
#include "../../gmf_amd/csrc/pair_plan.hpp"
#include "../../gmf_amd/csrc/posegraph_plan.hpp"

namespace {

int fails = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++fails; } \
  } while (0)

struct E12 { int a, b, c; };
struct E48 { int v[12]; };              // the size of gmf::MatchPair (launchers.hpp: twelve ints)
static_assert(sizeof(E12) == 12 && sizeof(E48) == 48 && sizeof(gmf::NodeEdge) == 12 && sizeof(gmf::CorrChunk) == 16 &&
                  sizeof(gmf::InfoChunk) == 16 && sizeof(gmf::PairTab) == 32, "element sizes the layouts below assume");

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// One list under test: the block, a made-up device base, and what every part so far claimed.
struct Run {
  HostTable tab;
  struct Part { size_t off, bytes; };
  std::vector<Part> parts;
  template <typename T>
  HostPart<T> add(size_t count) {
    const HostPart<T> p = tab.add<T>(count);
    parts.push_back({p.off, count * sizeof(T)});
    return p;
  }
};

template <typename T>
void fill(char* block, HostPart<T> p, size_t count) {
  char* const dev_base = reinterpret_cast<char*>(uintptr_t(1) << 40);      // never dereferenced
  T* hp = p.host(block);
  const T* dp = p.dev(dev_base);
  CHECK(reinterpret_cast<char*>(hp) - block == reinterpret_cast<const char*>(dp) - dev_base);
  CHECK((reinterpret_cast<uintptr_t>(dp) & 15) == 0);
  if (count) std::memset(hp, 0x5A, count * sizeof(T));
  for (size_t i = 0; i < count; ++i) hp[i] = T{};                         // ... and as elements of T
}

void check_layout(const Run& r, const char* block) {
  CHECK(!r.tab.overflowed());
  CHECK(r.tab.n == (int)r.parts.size());
  size_t end = 0;
  for (size_t i = 0; i < r.parts.size(); ++i) {
    const Run::Part& p = r.parts[i];
    CHECK(p.off == r.tab.off[i] && p.bytes == r.tab.len[i]);
    CHECK(p.off % 16 == 0);
    CHECK(((reinterpret_cast<uintptr_t>(block) + p.off) & 15) == 0);       // malloc's block is 16-byte aligned
    CHECK(p.off >= end && p.off - end < 16);                               // list order, apart, no more than the alignment between
    CHECK(p.off + p.bytes <= r.tab.bytes());
    end = p.off + p.bytes;
  }
  CHECK(end == r.tab.bytes());                                             // nothing behind the last part
}

// 1, 3, 5 and 7 parts; `c` runs over counts that leave every residue mod 16 in the byte sizes, with 0 and 1 among them
void run_lists(size_t c) {
  {
    Run r;
    const auto a = r.add<E12>(c);
    char* block = static_cast<char*>(std::malloc(r.tab.bytes() ? r.tab.bytes() : 1));
    fill(block, a, c);
    check_layout(r, block);
    CHECK(r.tab.bytes() == c * 12);
    std::free(block);
  }
  {
    Run r;
    const auto a = r.add<E48>(c + 1);
    const auto b = r.add<int>(c);
    const auto d = r.add<unsigned char>(c + 3);
    char* block = static_cast<char*>(std::malloc(r.tab.bytes()));
    fill(block, a, c + 1); fill(block, b, c); fill(block, d, c + 3);
    check_layout(r, block);
    std::free(block);
  }
  {
    Run r;
    const auto a = r.add<unsigned char>(c);
    const auto b = r.add<long long>(1);
    const auto d = r.add<E12>(c);
    const auto e = r.add<int>(0);
    const auto f = r.add<unsigned char>(c + 5);
    char* block = static_cast<char*>(std::malloc(r.tab.bytes()));
    fill(block, a, c); fill(block, b, 1); fill(block, d, c); fill(block, e, 0); fill(block, f, c + 5);
    check_layout(r, block);
    CHECK(r.parts[3].bytes == 0 && r.parts[4].off == r.parts[3].off);      // the empty part took nothing
    std::free(block);
  }
  {
    Run r;
    const auto a = r.add<int>(c + 1);
    const auto b = r.add<int>(c + 1);
    const auto d = r.add<long long>(c + 1);
    const auto e = r.add<unsigned char>(0);
    const auto f = r.add<E48>(c);
    const auto g = r.add<unsigned char>(2 * c + 1);
    const auto k = r.add<E12>(c);
    char* block = static_cast<char*>(std::malloc(r.tab.bytes()));
    fill(block, a, c + 1); fill(block, b, c + 1); fill(block, d, c + 1); fill(block, e, 0); fill(block, f, c);
    fill(block, g, 2 * c + 1); fill(block, k, c);
    check_layout(r, block);
    std::free(block);
  }
}

// the three real tables against the ladders gmf_api.cpp spelled out before this list existed
void run_real_layouts() {
  {                                                       // correspondences: B = 3, n_chunks = 5
    const size_t B = 3, n_chunks = 5;
    HostTable t;
    const auto pairs = t.add<E48>(B + 1);
    const auto c0 = t.add<int>(B + 1);
    const auto ck = t.add<gmf::CorrChunk>(n_chunks);
    const size_t o_c0 = align_up((B + 1) * 48, 16);
    const size_t o_ck = o_c0 + align_up((B + 1) * sizeof(int), 16);
    const size_t tab_bytes = o_ck + n_chunks * sizeof(gmf::CorrChunk);
    CHECK(pairs.off == 0 && c0.off == o_c0 && ck.off == o_ck && t.bytes() == tab_bytes && !t.overflowed());
  }
  {                                                       // information matrix: F = 4, E = 6, n_chunks = 9
    const size_t F = 4, E = 6, n_chunks = 9;
    HostTable t;
    const auto off = t.add<int>(F + 1);
    const auto src = t.add<int>(E);
    const auto tgt = t.add<int>(E);
    const auto c0 = t.add<int>(E + 1);
    const auto ck = t.add<gmf::InfoChunk>(n_chunks);
    const size_t o_src = align_up((F + 1) * sizeof(int), 16);
    const size_t o_tgt = o_src + align_up(E * sizeof(int), 16);
    const size_t o_c0 = o_tgt + align_up(E * sizeof(int), 16);
    const size_t o_ck = o_c0 + align_up((E + 1) * sizeof(int), 16);
    const size_t tab_bytes = o_ck + n_chunks * sizeof(gmf::InfoChunk);
    CHECK(off.off == 0 && src.off == o_src && tgt.off == o_tgt && c0.off == o_c0 && ck.off == o_ck && t.bytes() == tab_bytes);
  }
  for (size_t M : {(size_t)0, (size_t)11}) {              // pose graph: G = 2, N = 7, without and with edges
    const size_t G = 2, N = 7;
    HostTable t;
    const auto no = t.add<int>(G + 1);
    const auto eo = t.add<int>(G + 1);
    const auto ho = t.add<long long>(G + 1);
    const auto es = t.add<int>(M);
    const auto et = t.add<int>(M);
    const auto n0 = t.add<int>(N + 1);
    const auto li = t.add<gmf::NodeEdge>(2 * M);
    const size_t o_eo = align_up((G + 1) * sizeof(int), 16);
    const size_t o_ho = o_eo + align_up((G + 1) * sizeof(int), 16);
    const size_t o_es = o_ho + align_up((G + 1) * sizeof(long long), 16);
    const size_t o_et = o_es + align_up(M * sizeof(int), 16);
    const size_t o_n0 = o_et + align_up(M * sizeof(int), 16);
    const size_t o_li = o_n0 + align_up((N + 1) * sizeof(int), 16);
    const size_t tab_bytes = o_li + 2 * M * sizeof(gmf::NodeEdge);
    CHECK(no.off == 0 && eo.off == o_eo && ho.off == o_ho && es.off == o_es && et.off == o_et && n0.off == o_n0 && li.off == o_li);
    CHECK(t.bytes() == tab_bytes && !t.overflowed() && t.n == 7);
  }
}

void run_overflow() {
  // the arrays sit in a heap block of exactly their size: a write past either is a sanitizer report
  HostTable* t = static_cast<HostTable*>(std::malloc(sizeof(HostTable)));
  *t = HostTable{};
  for (int i = 0; i < HostTable::kMax; ++i) t->add<int>(3);
  CHECK(!t->overflowed());
  const size_t before = t->bytes();
  const HostTable copy = *t;
  t->add<E48>(100);
  CHECK(t->overflowed());
  CHECK(t->bytes() == before);
  CHECK(std::memcmp(t->off, copy.off, sizeof copy.off) == 0 && std::memcmp(t->len, copy.len, sizeof copy.len) == 0);
  std::free(t);
}

struct Plan { std::vector<gmf::PairTab> tab; int n_max = -1, s_max = -1; long long n_sum = -1; gmf::PairPlanStatus st; };
Plan plan(const std::vector<int>& n, double ratio, int k) {
  Plan p;
  // exactly B entries on the heap: the sanitizer sees a write behind them
  gmf::PairTab* raw = static_cast<gmf::PairTab*>(std::malloc(n.size() * sizeof(gmf::PairTab)));
  p.st = gmf::plan_pair_table(n.data(), (int)n.size(), ratio, k, raw, &p.n_max, &p.n_sum, &p.s_max);
  if (p.st == gmf::kPairPlanOk) p.tab.assign(raw, raw + n.size());
  std::free(raw);
  return p;
}

void check_rows(const std::vector<int>& n, const Plan& p, double ratio, int k) {
  int row = 0, smax = 0;
  for (size_t b = 0; b < n.size(); ++b) {
    const int S = ratio >= 0.0 ? (int)((double)n[b] * ratio) : 0;
    CHECK(p.tab[b].row0 == row && p.tab[b].n == n[b] && p.tab[b].S == S && p.tab[b].k == k);
    CHECK(p.tab[b].pad0 == 0 && p.tab[b].pad1 == 0 && p.tab[b].pad2 == 0);
    row += n[b];
    smax = S > smax ? S : smax;
  }
  CHECK(p.n_sum == row && p.s_max == smax);
}

void run_pair_plan() {
  {
    // B = 10: eight runs of 2, 2, 1, 1, 1, 1, 1, 1 slots.  Longest first, stable: 1, 3 (9), 6 (8), 4 (7), 8 (6), 0 (5), 9 (4), 2 (3),
    // 7 (2), 5 (1); each to the run with the least sum n^2 that still has a free slot, the lowest run on ties
    const std::vector<int> n{5, 9, 3, 9, 7, 1, 8, 2, 6, 4};
    const int want[10] = {1, 7, 3, 5, 6, 4, 8, 0, 9, 2};
    const Plan p = plan(n, 0.5, 40);
    CHECK(p.st == gmf::kPairPlanOk && p.n_max == 9 && p.n_sum == 54 && p.s_max == 4);
    for (int s = 0; s < 10; ++s) CHECK(p.tab[s].ord == want[s]);
    check_rows(n, p, 0.5, 40);
    const Plan e = plan(n, -1.0, 0);                       // the encoder's table: no seeds
    CHECK(e.st == gmf::kPairPlanOk && e.s_max == 0);
    for (int s = 0; s < 10; ++s) CHECK(e.tab[s].S == 0 && e.tab[s].ord == want[s]);
    check_rows(n, e, -1.0, 0);
  }
  {
    const std::vector<int> n{3, 5, 5, 1};                  // fewer than 8 pairs: one run, longest first, stable
    const int want[4] = {1, 2, 0, 3};
    const Plan p = plan(n, 0.5, 7);
    CHECK(p.st == gmf::kPairPlanOk && p.n_max == 5 && p.n_sum == 14 && p.s_max == 2);
    for (int s = 0; s < 4; ++s) CHECK(p.tab[s].ord == want[s]);
    check_rows(n, p, 0.5, 7);
  }
  std::mt19937 rng(20240607);
  for (int B = 1; B <= 40; ++B) {
    std::vector<int> n(B);
    for (int& v : n) v = 1 + (int)(rng() % 6000);
    const Plan p = plan(n, 0.1, 40);
    CHECK(p.st == gmf::kPairPlanOk);
    std::vector<int> seen(B, 0);
    for (int s = 0; s < B; ++s)
      if (p.tab[s].ord >= 0 && p.tab[s].ord < B) ++seen[p.tab[s].ord];
    for (int b = 0; b < B; ++b) CHECK(seen[b] == 1);
    check_rows(n, p, 0.1, 40);
  }
  {
    // the refusals, asked for alone and from the plan, which then writes neither the table nor the sizes
    int n_max = -7, s_max = -7;
    long long n_sum = -7;
    const int empty[3] = {4, 0, 2};
    gmf::PairTab guard[3];
    std::memset(guard, 0x5A, sizeof guard);
    gmf::PairTab same[3];
    std::memcpy(same, guard, sizeof guard);
    CHECK(gmf::check_pair_sizes(empty, 3) == gmf::kPairPlanEmptyPair);
    CHECK(gmf::plan_pair_table(empty, 3, 0.5, 1, guard, &n_max, &n_sum, &s_max) == gmf::kPairPlanEmptyPair);
    const int big[2] = {1 << 30, 1 << 30};                 // 2^31 rows
    CHECK(gmf::check_pair_sizes(big, 2) == gmf::kPairPlanTooManyRows);
    CHECK(gmf::plan_pair_table(big, 2, 0.5, 1, guard, &n_max, &n_sum, &s_max) == gmf::kPairPlanTooManyRows);
    CHECK(std::memcmp(guard, same, sizeof guard) == 0 && n_max == -7 && n_sum == -7 && s_max == -7);
    const int most[2] = {1 << 30, (1 << 30) - 1};          // 2^31 - 1 rows: the last that fits
    CHECK(gmf::check_pair_sizes(most, 2) == gmf::kPairPlanOk);
    CHECK(gmf::plan_pair_table(most, 2, -1.0, 0, guard, &n_max, &n_sum, nullptr) == gmf::kPairPlanOk);
    CHECK(n_max == (1 << 30) && n_sum == 0x7fffffffLL);
  }
}

}  // namespace

int main() {
  for (size_t c = 0; c <= 17; ++c) run_lists(c);
  run_lists(1000);
  run_real_layouts();
  run_overflow();
  run_pair_plan();
  std::printf(fails ? "host_table_host: %d checks failed\n" : "host_table_host: ok\n", fails);
  return fails ? 1 : 0;
}
