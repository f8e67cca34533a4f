// The chunk plan of the correspondence chain (gmf_amd/csrc/corr_plan.hpp) on its own: built by the host compiler with
// -fsanitize=address,undefined (tests/test_correspondences_host.py).  Over the GPU tests' batch, a batch of empty pairs and a few
// sizes around the chunk length: the chunks tile every pair exactly, in row order, and none crosses a pair.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gmf_amd/csrc/corr_plan.hpp"

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::printf("corr_plan_host: %s failed (line %d)\n", #c, __LINE__); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

static int check_batch(const std::vector<int>& n0) {
  const int B = (int)n0.size();
  std::vector<int> off0(B + 1, 0);
  for (int b = 0; b < B; ++b) off0[b + 1] = off0[b] + n0[b];
  const long want = gmf::corr_chunk_count(off0.data(), B);
  // exactly `want` chunks and B + 1 entries: the sanitizer sees any write behind either
  gmf::CorrChunk* chunks = static_cast<gmf::CorrChunk*>(std::malloc(want ? want * sizeof(gmf::CorrChunk) : 1));
  int* pc0 = static_cast<int*>(std::malloc((B + 1) * sizeof(int)));
  CHECK(chunks && pc0);
  CHECK(gmf::corr_plan_chunks(off0.data(), B, chunks, pc0) == want);
  CHECK(pc0[0] == 0 && pc0[B] == want);
  long c = 0;
  for (int b = 0; b < B; ++b) {
    CHECK(pc0[b] == c);
    CHECK(pc0[b + 1] - pc0[b] == (n0[b] + gmf::kCorrChunk - 1) / gmf::kCorrChunk);
    int row = off0[b];
    for (; c < pc0[b + 1]; ++c) {
      const gmf::CorrChunk& k = chunks[c];
      CHECK(k.pair == b);
      CHECK(k.row0 == row);                                       // the pair's rows in order, no gap and no overlap
      CHECK(k.n >= 1 && k.n <= gmf::kCorrChunk);
      CHECK(k.n == gmf::kCorrChunk || c + 1 == pc0[b + 1]);        // only a pair's last chunk is short
      CHECK(k.first == (row == off0[b] ? 1 : 0));
      row += k.n;
      CHECK(row <= off0[b + 1]);                                  // never into the next pair
    }
    CHECK(row == off0[b + 1]);
  }
  CHECK(c == want);
  std::free(chunks);
  std::free(pc0);
  return 0;
}

int main() {
  if (check_batch({301, 5, 1, 0, 64, 0, 130, 700, 1500})) return 1;       // the GPU tests' source sizes
  if (check_batch({0, 0, 0, 0})) return 1;
  if (check_batch({0})) return 1;
  if (check_batch({255, 256, 257, 0, 512, 513, 1})) return 1;
  if (check_batch({100000})) return 1;
  std::printf("corr_plan_host: ok\n");
  return 0;
}
