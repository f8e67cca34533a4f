// The launch decisions of the sparse engine (gmf_amd/csrc/sparse_conv_plan.hpp) on their own: built by the host compiler with
// -fsanitize=address,undefined (tests/test_sparse_forms_host.py).  Reads lines of plain geometry from the file in argv[1], one
// launch per line, prints the plan of each and checks its invariants, written out here independently of the plan code:
//   conv K cin cout nsplit cap_out n_out     -> groups, the row bound of every group, the first offset of every slice
//   wgrad narrow K nnz n_0 .. n_{K-1}        -> nslots, P, chunks used, the longest chunk's tiles, multi-tile chunks with a ragged tail
//   narrow K cin cout cap_out                -> lanes per row, rows per workgroup, W in LDS or global, grid
//   head cap_out                             -> grid
//   bnm cap n                                -> chunks and the row bound of every chunk
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../gmf_amd/csrc/sparse_conv_plan.hpp"

static int g_line = 0;

#define CHECK(c)                                                                                  \
  do {                                                                                            \
    if (!(c)) {                                                                                   \
      std::printf("sparse_plan_host: %s failed (source line %d) at input line %d\n", #c, __LINE__, g_line); \
      return 1;                                                                                   \
    }                                                                                             \
  } while (0)

static int do_conv(std::istringstream& in) {
  long long K, cin, cout, nsplit, cap_out, n_out;
  CHECK(in >> K >> cin >> cout >> nsplit >> cap_out >> n_out);
  CHECK(K >= 1 && K <= 1024 && nsplit >= 1 && nsplit <= K && n_out >= 0 && n_out <= cap_out && cap_out >= 1);
  const int G = gmf::sparse_conv_row_groups((int)K, (int)cin, (int)cout, (int)nsplit, cap_out);
  CHECK(G >= 1 && G <= 65535);                                        // gridDim.z
  if (K * cin * cout * 4 > (16LL << 20)) CHECK(G == 1);
  std::printf("conv groups %d rows", G);
  int prev = 0;
  for (int g = 0; g <= G; ++g) {                                      // the groups partition 0..n_out, ascending
    const int b = gmf::sparse_conv_group_begin((int)n_out, g, G);
    CHECK(b >= prev && b <= n_out);
    if (g == 0) CHECK(b == 0);
    if (g == G) CHECK(b == n_out);
    prev = b;
    std::printf(" %d", b);
  }
  std::printf(" slices");
  std::vector<int> owner((size_t)K, -1);
  prev = 0;
  for (int s = 0; s <= nsplit; ++s) {                                 // the slices partition 0..K, none empty (nsplit <= K)
    const int b = gmf::slice_begin(s, (int)nsplit, (int)K);
    if (s == 0) CHECK(b == 0);
    if (s > 0) CHECK(b > prev);
    if (s == nsplit) CHECK(b == K);
    if (s > 0)
      for (int d = prev; d < b; ++d) owner[(size_t)d] = s - 1;
    prev = b;
    std::printf(" %d", b);
  }
  for (int d = 0; d < K; ++d) CHECK(owner[(size_t)d] == gmf::slice_of(d, (int)nsplit, (int)K));   // slice_of agrees with slice_begin
  std::printf("\n");
  return 0;
}

static int do_wgrad(std::istringstream& in) {
  long long narrow, K, nnz;
  CHECK(in >> narrow >> K >> nnz);
  CHECK(K >= 1 && K <= 1024 && nnz >= 0);
  std::vector<long long> n((size_t)K);
  long long sum = 0;
  for (auto& v : n) {
    CHECK(in >> v);
    CHECK(v >= 0);
    sum += v;
  }
  CHECK(sum == nnz);
  const int nslots = narrow ? gmf::sparse_wgrad_narrow_slots((int)K) : gmf::sparse_wgrad_slots((int)K);
  const int P = gmf::sparse_wgrad_chunk(nnz, (int)K, nslots);
  CHECK(P >= gmf::kWgradMinChunk);
  long long chunks = 0, longest = 0, multi_ragged = 0, multi = 0;
  for (long long v : n) {
    const long long c = (v + P - 1) / P;
    chunks += c;
    for (long long i = 0; i < c; ++i) {
      const long long len = (i + 1) * P <= v ? P : v - i * P;
      CHECK(len >= 1 && len <= P);
      const long long tiles = (len + 63) / 64;
      if (tiles > longest) longest = tiles;
      if (tiles > 1) ++multi;
      if (tiles > 1 && len % 64) ++multi_ragged;
    }
  }
  CHECK(chunks <= nslots);                                           // every chunk has a slot: partial holds nslots tiles
  std::printf("wgrad nslots %d P %d chunks %lld longest_tiles %lld multi_tile %lld multi_tile_ragged %lld\n", nslots, P, chunks, longest,
              multi, multi_ragged);
  return 0;
}

static int do_narrow(std::istringstream& in) {
  long long K, cin, cout, cap_out;
  CHECK(in >> K >> cin >> cout >> cap_out);
  CHECK(K >= 1 && K <= 1024 && cin >= 1 && cin <= 8 && cout >= 1 && cout <= 64 && cap_out >= 1);
  const int L = gmf::sparse_narrow_lanes((int)cout), per = gmf::sparse_narrow_rows_per_wg((int)cout);
  CHECK((L == 16 || L == 32 || L == 64) && L >= cout && (L == 16 || L / 2 < cout) && per == 4 * (64 / L));
  const bool lds = gmf::sparse_narrow_lds((int)K, (int)cin, (int)cout);
  CHECK(lds == (K * cin * cout * 4 <= 65536));                       // the dynamic LDS of a launch stays within 64 KiB
  const int grid = gmf::sparse_narrow_grid(cap_out, (int)K, (int)cin, (int)cout);
  CHECK(grid >= 1 && grid <= (lds ? 768 : 4096) && ((long long)grid * per >= cap_out || grid == (lds ? 768 : 4096)));
  std::printf("narrow lanes %d rows_per_wg %d lds %d grid %d strides %lld\n", L, per, lds ? 1 : 0, grid,
              (cap_out + (long long)grid * per - 1) / ((long long)grid * per));
  return 0;
}

static int do_head(std::istringstream& in) {
  long long cap_out;
  CHECK(in >> cap_out);
  CHECK(cap_out >= 1);
  const int grid = gmf::sparse_head_grid(cap_out);
  CHECK(grid >= 1 && grid <= 1024 && ((long long)grid * 4 >= cap_out || grid == 1024));
  std::printf("head grid %d strides %lld\n", grid, (cap_out + (long long)grid * 4 - 1) / ((long long)grid * 4));
  return 0;
}

static int do_bnm(std::istringstream& in) {
  long long cap, n;
  CHECK(in >> cap >> n);
  CHECK(cap >= 1 && n >= 0 && n <= cap);
  const int nch = gmf::bnm_chunks(cap);
  CHECK(nch >= 1 && nch <= 64 && (nch == 64 || (long long)nch * 256 >= cap));
  std::printf("bnm chunks %d rows", nch);
  long long prev = 0;
  for (int c = 0; c <= nch; ++c) {                                    // the chunks partition 0..cap, ascending
    const long long b = gmf::bnm_chunk_begin(cap, c, nch);
    CHECK(b >= prev && b <= cap);
    if (c == 0) CHECK(b == 0);
    if (c == nch) CHECK(b == cap);
    prev = b;
    std::printf(" %lld", b);
  }
  std::printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: sparse_plan_host GEOMETRY_FILE\n");
    return 2;
  }
  std::FILE* fh = std::fopen(argv[1], "r");
  if (!fh) {
    std::printf("sparse_plan_host: cannot open %s\n", argv[1]);
    return 2;
  }
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, fh)) > 0) text.append(buf, got);
  std::fclose(fh);
  std::istringstream all(text);
  std::string line;
  while (std::getline(all, line)) {
    ++g_line;
    if (line.empty() || line[0] == '#') continue;
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    int rc;
    if (kind == "conv") rc = do_conv(in);
    else if (kind == "wgrad") rc = do_wgrad(in);
    else if (kind == "narrow") rc = do_narrow(in);
    else if (kind == "head") rc = do_head(in);
    else if (kind == "bnm") rc = do_bnm(in);
    else {
      std::printf("sparse_plan_host: unknown kind '%s' at input line %d\n", kind.c_str(), g_line);
      return 2;
    }
    if (rc) return rc;
  }
  std::printf("sparse_plan_host: ok\n");
  return 0;
}
