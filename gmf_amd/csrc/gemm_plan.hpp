// The launch decision of gmf_gemm_f32 (train_kernels.hip): which of the two kernels, which workgroup tile, how many k-splits of
// what depth, and how many wave-groups the split-K reduction runs in.  No handle and no HIP here: operand alignment comes in as
// plain integers (pointer value mod 16), so the plan is plain host code, compiled and tested on its own
// (tests/abi_cpp/gemm_plan_host.cpp over tests/golden/gemm_forms_table.txt).
#pragma once

namespace gmf {

// C[b] = alpha op(A[b]) op(B[b]): op(A) is M x K, op(B) is K x N, row strides lda / ldb and batch strides sA / sB in floats;
// a_mod16 / b_mod16: the operand's base address modulo 16 bytes
struct GemmGeom {
  bool ta, tb;
  int M, N, K;
  long lda, ldb, sA, sB;
  int batch;
  int a_mod16, b_mod16;
};

struct GemmPlan {
  bool lds;              // k_gemm_lds (operands staged through LDS), else k_gemm_f32 (operands straight into registers)
  int bm, bn;            // workgroup tile: 128 x 128, 64 x 128, or (k_gemm_lds only) 64 x 64
  int ksplits;           // k-splits that run, after kchunk was rounded up to whole 16-deep steps
  int kchunk;            // contraction indices per split, a multiple of 16
  int reduce_groups;     // wave-groups of k_gemm_reduce (1, 2, 4, 8, 16); 0 without split-K: no reduction runs
};

// the LDS-staged kernel needs 16-byte pieces along each operand's contiguous dimension
inline bool gemm_lds_ok(const GemmGeom& g) {
  const bool a_ok = g.a_mod16 == 0 && g.lda % 4 == 0 && g.sA % 4 == 0 && (g.ta ? g.M % 4 == 0 : g.K % 4 == 0);
  const bool b_ok = g.b_mod16 == 0 && g.ldb % 4 == 0 && g.sB % 4 == 0 && (g.tb ? g.K % 4 == 0 : g.N % 4 == 0);
  return a_ok && b_ok && g.K >= 4 && g.M >= 4 && g.N >= 4;
}

// Workgroup tile of a product: 128 x 128 when that alone gives the chip two workgroups per CU; else 64-row tiles, and 64-column
// tiles too (LDS-staged kernel only) when the 64 x 128 tiling would still have to split a contraction it can do whole
inline void gemm_tile(const GemmGeom& g, bool lds_ok, int* bm, int* bn) {
  const long t128 = (long)((g.M + 127) / 128) * ((g.N + 127) / 128) * g.batch;
  *bm = (t128 < 512 && g.M > 64) ? 64 : 128;
  *bn = 128;
  const long t64 = (long)((g.M + *bm - 1) / *bm) * ((g.N + 127) / 128) * g.batch;
  if (lds_ok && *bm == 64 && t64 < 384 && g.K >= 256 && g.N > 64) *bn = 64;
}

// The k-splits a call asks for (its split-K workspace holds this many partial tiles per output): few output tiles and a long
// contraction (weight gradients: K = every row of the batch) split K so that the launch has ~768 workgroups, each split at
// least 64 deep, the partial tiles at most ~48 MB (written and read once by k_gemm_reduce)
inline int gemm_ksplits_wanted(const GemmGeom& g) {
  int bm, bn;
  gemm_tile(g, gemm_lds_ok(g), &bm, &bn);
  const long tiles = (long)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn) * g.batch;
  if (tiles >= 384 || g.K < 256) return 1;
  long s = (768 + tiles - 1) / tiles;
  if (g.K / 64 < s) s = g.K / 64;
  const long out_bytes = (long)g.M * g.N * g.batch * 4;
  long cap = (48L << 20) / out_bytes;
  if (cap < 1) cap = 1;
  if (cap < s) s = cap;
  if (s > 128) s = 128;
  return (int)(s < 1 ? 1 : s);
}

// The plan of a launch that may use up to `ksplits` partial tiles per output (gemm_ksplits_wanted(g), or 1 without a workspace)
inline GemmPlan gemm_plan(const GemmGeom& g, int ksplits) {
  GemmPlan p;
  if (ksplits < 1) ksplits = 1;
  p.kchunk = (g.K + ksplits - 1) / ksplits;
  p.kchunk = (p.kchunk + 15) / 16 * 16;
  p.ksplits = (g.K + p.kchunk - 1) / p.kchunk;
  p.lds = gemm_lds_ok(g);          // anything else takes the register-direct kernel
  gemm_tile(g, p.lds, &p.bm, &p.bn);
  p.reduce_groups = p.ksplits <= 1 ? 0 : p.ksplits > 64 ? 16 : p.ksplits > 32 ? 8 : p.ksplits > 16 ? 4 : p.ksplits > 8 ? 2 : 1;
  return p;
}

inline GemmPlan gemm_plan(const GemmGeom& g) { return gemm_plan(g, gemm_ksplits_wanted(g)); }

}  // namespace gmf
