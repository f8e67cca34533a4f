// The dual-use image of a key tile's high fp16 plane (gmf_amd/csrc/kv_share_layout.hpp) against the two fragment-major images it
// replaces, on the host: a tile of distinct values is written through off(), both kinds of LDS read are emulated lane for lane
// (ds_read_b128 by rows; ds_read_b64_tr_b16: lane 4 q + p of a 16-lane group supplies the address of row q and of the four values
// that lanes 4 p .. 4 p + 3 receive, lane i receives column i), and every lane of every fragment must hold exactly what the K image
// (16-byte unit s * 64 + lane) and the V image (unit (2 db + s2) * 64 + lane) give it.  Also: off() is a bijection on the 8 KiB, every
// address is aligned for its instruction, the addresses decompose into the two bases and the immediates the kernel uses, and both
// kinds of read touch no bank twice within a lane group (bank of byte a = (a / 4) % 64).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../gmf_amd/csrc/kv_share_layout.hpp"

using namespace gmf::kvshare;

static int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
      ++failures;                                          \
    }                                                      \
  } while (0)

// mfma_core.hpp: register r (0..15) of a 32-wide block on a lane of half h
static unsigned frag_feature(unsigned r, unsigned h) { return 8 * (r >> 2) + 4 * h + (r & 3); }
static uint16_t value(unsigned key, unsigned channel) { return (uint16_t)(1 + key * 128 + channel); }   // distinct, never 0

// the lane groups of one LDS cycle
static const std::vector<std::vector<unsigned>>& groups_b128() {
  static std::vector<std::vector<unsigned>> g;
  if (g.empty()) {
    const unsigned first[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                   {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    for (unsigned half = 0; half < 2; ++half)
      for (unsigned k = 0; k < 2; ++k) {
        std::vector<unsigned> v;
        for (unsigned e = 0; e < 16; ++e) v.push_back(32 * half + first[k][e]);
        g.push_back(v);
      }
  }
  return g;
}
static std::vector<std::vector<unsigned>> groups_halves() {
  std::vector<std::vector<unsigned>> g(2);
  for (unsigned l = 0; l < 64; ++l) g[l >> 5].push_back(l);
  return g;
}
// extra LDS cycles of one wave instruction: per group, the largest number of DISTINCT addresses on one bank, minus one
static unsigned conflicts(const unsigned (&addr)[64], unsigned bytes, const std::vector<std::vector<unsigned>>& groups) {
  unsigned extra = 0;
  for (const auto& grp : groups) {
    std::vector<std::vector<unsigned>> on_bank(64);
    for (unsigned l : grp)
      for (unsigned b = 0; b < bytes / 4; ++b) {
        auto& v = on_bank[(addr[l] / 4 + b) % 64];
        bool seen = false;
        for (unsigned a : v) seen = seen || a == addr[l] + 4 * b;
        if (!seen) v.push_back(addr[l] + 4 * b);
      }
    unsigned worst = 1;
    for (const auto& v : on_bank) worst = v.size() > worst ? (unsigned)v.size() : worst;
    extra += worst - 1;
  }
  return extra;
}

int main() {
  // ---- off() is a bijection of (row, chunk) onto the 512 aligned 16-byte units of the plane ----
  {
    std::vector<int> hit(kPlaneBytes / 16, 0);
    for (unsigned row = 0; row < 32; ++row)
      for (unsigned ch = 0; ch < 16; ++ch) {
        const unsigned o = off(row, ch);
        CHECK(o % 16 == 0 && o + 16 <= kPlaneBytes, "off(%u, %u) = %u", row, ch, o);
        if (o % 16 == 0 && o + 16 <= kPlaneBytes) ++hit[o / 16];
      }
    for (unsigned u = 0; u < kPlaneBytes / 16; ++u) CHECK(hit[u] == 1, "unit %u written %d times", u, hit[u]);
  }
  // ---- the tile, written as the linear kernel writes it: lane (h, key) stores its 8 values of k-step s at off(key, 2 s + h) ----
  std::vector<uint16_t> img(kPlaneBytes / 2, 0), k_img(8 * 64 * 8, 0), v_img(8 * 64 * 8, 0);
  for (unsigned s = 0; s < 8; ++s)
    for (unsigned lane = 0; lane < 64; ++lane) {
      const unsigned h = lane >> 5, key = lane & 31;
      for (unsigned e = 0; e < 8; ++e) {
        const unsigned channel = 32 * (s >> 1) + frag_feature(8 * (s & 1) + e, h);
        img[off(key, 2 * s + h) / 2 + e] = value(key, channel);
        k_img[(s * 64 + lane) * 8 + e] = value(key, channel);                       // store_block_v8 on a K block: slot 2 mb + half = s
      }
    }
  for (unsigned db = 0; db < 4; ++db)                                                // ... on a V^T block: the lane's feature, 16 keys
    for (unsigned s2 = 0; s2 < 2; ++s2)
      for (unsigned lane = 0; lane < 64; ++lane)
        for (unsigned e = 0; e < 8; ++e)
          v_img[((2 * db + s2) * 64 + lane) * 8 + e] = value(frag_feature(8 * s2 + e, lane >> 5), 32 * db + (lane & 31));
  for (unsigned u = 0; u < kPlaneBytes / 2; ++u) CHECK(img[u] != 0, "element %u of the plane not written", u);

  unsigned row_conf = 0, tr_conf = 0;
  // ---- row reads: S = K Q'^T, k-step s ----
  for (unsigned s = 0; s < 8; ++s) {
    unsigned addr[64];
    for (unsigned lane = 0; lane < 64; ++lane) {
      addr[lane] = row_read_addr(lane, s);
      CHECK(addr[lane] % 16 == 0 && addr[lane] + 16 <= kPlaneBytes, "row read s %u lane %u: address %u", s, lane, addr[lane]);
      CHECK(addr[lane] == row_read_addr(lane, s & 1) + 512 * (s >> 1), "row read s %u lane %u: base + immediate", s, lane);
      if (addr[lane] % 16 || addr[lane] + 16 > kPlaneBytes) continue;
      CHECK(std::memcmp(&img[addr[lane] / 2], &k_img[(s * 64 + lane) * 8], 16) == 0, "row read s %u lane %u differs from the K image", s, lane);
    }
    row_conf += conflicts(addr, 16, groups_b128());
  }
  // ---- transposed reads: O^T += V^T P^T, feature block db, k-step s2, the two key groups e2 of the operand ----
  for (unsigned db = 0; db < 4; ++db)
    for (unsigned s2 = 0; s2 < 2; ++s2)
      for (unsigned e2 = 0; e2 < 2; ++e2) {
        unsigned addr[64];
        bool ok = true;
        for (unsigned lane = 0; lane < 64; ++lane) {
          const unsigned kg = 4 * s2 + 2 * e2 + (lane >> 5);
          addr[lane] = tr_read_addr(lane, db, kg);
          const bool in = addr[lane] % 8 == 0 && addr[lane] + 8 <= kPlaneBytes;
          CHECK(in, "transposed read db %u s2 %u e2 %u lane %u: address %u", db, s2, e2, lane, addr[lane]);
          ok = ok && in;
          CHECK(addr[lane] == tr_read_addr(lane, 0, 2 * e2 + (lane >> 5)) + 512 * db + 4096 * s2,
                "transposed read db %u s2 %u e2 %u lane %u: base + immediate", db, s2, e2, lane);
        }
        if (!ok) continue;
        for (unsigned lane = 0; lane < 64; ++lane) {
          const unsigned g16 = lane >> 4, col = lane & 15;
          for (unsigned q = 0; q < 4; ++q) {                // element q of the result = row q of the block, column `col`
            const unsigned supplier = 16 * g16 + 4 * q + (col >> 2);
            const uint16_t got = img[addr[supplier] / 2 + (col & 3)];
            const uint16_t want = v_img[((2 * db + s2) * 64 + lane) * 8 + 4 * e2 + q];
            CHECK(got == want, "transposed read db %u s2 %u e2 %u lane %u element %u: %u, the V image has %u", db, s2, e2, lane, q, got, want);
          }
        }
        tr_conf += conflicts(addr, 8, groups_halves());
      }
  CHECK(row_conf == 0, "row reads: %u extra LDS cycles per tile", row_conf);
  CHECK(tr_conf == 0, "transposed reads: %u extra LDS cycles per tile", tr_conf);
  // the bank rule itself sees a conflict where there is one: all lanes of a half on one column of plain 256-byte rows
  {
    unsigned addr[64];
    for (unsigned lane = 0; lane < 64; ++lane) addr[lane] = 256 * (lane & 31);
    CHECK(conflicts(addr, 8, groups_halves()) == 2 * 31, "the conflict count of a 32-way read");
  }
  std::printf("row reads: 8, extra LDS cycles %u; transposed reads: 16, extra LDS cycles %u\n", row_conf, tr_conf);
  if (failures) { std::printf("kv_share_layout_host: %d failures\n", failures); return 1; }
  std::printf("kv_share_layout_host: ok\n");
  return 0;
}
