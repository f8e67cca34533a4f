// Internal C++ launch entry points of the encoder, matching, validation, training and image kernels, with the structs their
// kernels take by value (PvGuard, LazyCompat) and the two argument blocks of the encoder's layer launches (ForwardBuffers, LayerRun).
// The other kernel families have a launchers_*.hpp each.  The public C ABI is include/gmf_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "layer_weights.hpp"
#include "pair_plan.hpp"

namespace gmf {

// struct PairTab, the per-pair table of a ragged batch, and its host plan: pair_plan.hpp
// struct Tuning, the per-handle knobs with their table, and the plan of an encoder forward: encoder_plan.hpp (free of HIP)
// struct LayerWeights, one layer's weight pointers, and the layout of a kv_fold block: layer_weights.hpp (free of HIP)

// The "pv_fp8" guard (gmf_set_tuning "pv_fp8" = 1, the default): which of a layer's pairs run the P V cross products of
// the spatial-consistency attention on the fp8 pipe is decided ON THE DEVICE, per pair, from a statistic the previous kernel
// left behind - the largest squared row norm of the layer's input f - against the layer's threshold (gmf_encoder_weights::
// pv_guard).  Every kernel that writes a V image or multiplies one evaluates the same comparison on the same two words, so the
// writer and the reader of a pair's V tiles always agree on their format.
constexpr int kPvStatStride = 32;    // words between two pairs' statistics: one 128-byte line each.  (Packed into one line, the 5 000 device-scope
                                    // atomics of k_front_h2<3> - every wave of every pair within microseconds - serialised at the memory side:
                                    // 30 -> 64 us for that kernel; a line per pair lets the pairs' updates proceed in parallel.)
struct PvGuard {
  const unsigned* stat = nullptr;   // [B][kPvStatStride] float bits of max row |f_l|^2 per pair (word 0 of its line), complete before the layer's first launch; null: unguarded
  const float* thr2 = nullptr;      // the layer's threshold: fp8 cross products while stat <= *thr2
  unsigned* stat_next = nullptr;    // [B] the NEXT layer's statistic: raised (atomic maximum) by whoever produces f_{l+1}; null: nobody asks
};

// "compat_16": the exact cache of the guarded 16-bit form, built lazily by one more workgroup role of the layer's linear launch (the
// launch between the attention that completes the layer's statistic and the attention that streams the cache): ceil(tiles / 4)
// workgroups per pair, which return at once unless the pair trips the guard at `layer` and tripped it at no earlier layer - then
// they write the pair's fp32 tiles, the bytes k_compat_build<0> writes, once per forward.  Both facts come from the words every
// other kernel of the guard compares (the comparison of pv_planes_on, so a NaN statistic trips): no flag, no atomic, no order
// between workgroups.
struct LazyCompat {
  float* c_dense = nullptr;         // the fp32 cache [B, tiles, tiles, 1024]; null: no such role in the launch
  const float* pts8 = nullptr;      // the packed key points (k_pack_pts8)
  const unsigned* fstat = nullptr;  // [layer][B][kPvStatStride] the guard's statistics from layer 0 on
  const float* thr2 = nullptr;      // [layer] the guard's thresholds from layer 0 on
  int layer = 0;
  float inv_sig2 = 0.f;
};

// What one encoder forward fixes before its layer loop: the compat cache (built once per batch by launch_compat_build, k_compat_build:
// [B, tiles, tiles, 1024] floats), the key-split partials, the pair table and V's scale words.  `half` and `fmt` are the plan's
// (encoder_plan.hpp, EncoderPlan).
struct ForwardBuffers {
  const float* dense = nullptr;      // the cache; element format `fmt` (k_compat_build): 0 = fp32 (4 KiB per tile); 16-bit, 2 KiB per tile:
  int fmt = 0;                       // 1 = fp16 c (with `half`), 2 = fixed point rint(65535 c)
  bool half = false;                 // `dense` holds fp16 tiles and the attention multiplies one fp16 product: the throughput numerics
                                     // mode (Tuning::precision = 1), large grids only
  // "compat_16" (EncoderPlan::c16_guard): non-null = `dense` holds the 16-bit cache (fmt = 2) for the pairs the guard lets through at a
  // layer, and this is the exact fp32 cache of the pairs it trips (the layer's linear launch fills it: LazyCompat)
  const float* dense_fb = nullptr;
  float* part_o = nullptr;           // key-split workspace: [max splits][B * tiles] P32 tile images (or nullptr)
  float* part_ml = nullptr;          // ... [max splits][B * tiles][32][2] row maximum, row sum
  const PairTab* ptab = nullptr;     // ragged batch: per-pair rows (device), else null
  unsigned* v_scale = nullptr;       // non-null: the layers' V images carry e4m3 cross planes (store_block_v8) and these are their
                                     // scale words, [B * tiles][64]; k_linear_h2 writes both, k_scattn_h2p<3, *, true> reads them
};

// What one layer of it fixes, built in one place from (plan, layer view, buffers): gmf_api_encoder.cpp, layer_run
struct LayerRun {
  LayerWeights w;
  PvGuard guard;                     // per pair: e4m3 cross planes or V's low fp16 plane (with ForwardBuffers::v_scale)
  // What the attention epilogue (and the merge) runs on: the launchers read these, never w.tail_* / w.next_*.  epi_wst, epi_vec:
  // fc_message, weights (split-fp16) and vectors - the layer's own or, under "kv_fold", the composed ones.  epi_next_*: the fused forms,
  // every layer but the last - non-null = the NEXT layer's PointCN (w.next_*) is applied to the block output and f_{l+1} is stored
  // instead of feat; null: the block output itself (the forms with a front kernel per layer)
  const float* epi_wst = nullptr;
  const float* epi_vec = nullptr;
  const float* epi_next_wst = nullptr;
  const float* epi_next_bias = nullptr;
  // qw_wst non-null: no Q' image exists - every attention workgroup projects its own Q' in its prologue from the layer's f image
  // (qf_img), four weight stages (qw_wst) and a bias (qw_bias, 128 floats); parity kernels of the pipelined form only
  const float* qf_img = nullptr;
  const float* qw_wst = nullptr;
  const float* qw_bias = nullptr;
  // "kv_fold" (EncoderPlan::kv_fold): non-null = the K and V images hold the layer input f, epi_* / qw_* are the composed weights of
  // the layer's kv_fold block, qf_img is always the layer's f image, and these are Wq'^T bk [128] | bk . bq'
  const float* kvf_vec = nullptr;
  LazyCompat lazy;                   // "compat_16": one more role of the layer's linear launch
};

hipError_t launch_compat_build(const float* pts8, float* c_dense, int B, int N, int tiles, float sigma_d, int fmt, hipStream_t s,
                               const PairTab* ptab = nullptr);
hipError_t launch_front(int mode, const float* in, const float* wst, const float* vecs, float* f, float* q, float* k,
                        float* v, int B, int N, int tiles, hipStream_t s);
hipError_t launch_scattn_fp32(const float* q, const float* k, const float* v, const float* pts8, const float* fus,
                              const float* wst, const float* vecs, float* out, int B, int N, int tiles, float sigma_d,
                              hipStream_t s);
hipError_t launch_scattn_h2(const float* q, const float* k, const float* v, const float* pts8, const float* fus, const float* wst,
                            const float* vecs, float* out, int B, int N, int tiles, float sigma_d, hipStream_t s, const float* c_dense);
// the cached, pipelined attention (scattn_variant 18): n_full items per XCD whole, the rest split `ksplits` ways by keys
hipError_t launch_scattn_h2p(const float* q, const float* k, const float* v, const float* fus, float* out, int B, int N, int tiles,
                             const ForwardBuffers& fb, const LayerRun& lr, int n_full, int ksplits, hipStream_t s);
hipError_t launch_scattn_dense(const float* q, const float* k, const float* v, const float* compat, const float* fus,
                               const float* wst, const float* vecs, float* out, int B, int N, int tiles, hipStream_t s);
hipError_t launch_ctx_prep(bool pe, const float* ctx, const float* wst, const float* vecs, float* out, int B, int T,
                           int ttiles, int sets, int wst_stride, int vec_stride, hipStream_t s);
hipError_t launch_fusion_attn(bool pe, const float* x, const float* ctx_img, const float* wst, const float* vecs,
                              float* x1, int B, int N, int tiles, int T, int ttiles, hipStream_t s);
hipError_t launch_fusion_ff(const float* x1, const float* wst, const float* vecs, float* x2, int B, int tiles, hipStream_t s);
hipError_t launch_head(const float* feat_img, const float* wst, const float* vecs, float* logits, float* feat_n,
                       float* feat_rm, int B, int N, int tiles, hipStream_t s, int* status = nullptr, const PairTab* ptab = nullptr,
                       const unsigned* pv_stat = nullptr, const float* pv_thr2 = nullptr, int n_layers = 0);   // pv_*: the "pv_fp8" guard's
                       // statistics [n_layers][B] and thresholds - a tripped layer sets GMF_STATUS_PV_GUARDED (informational)
hipError_t launch_ctx_prep_w(bool pe, const float* ctx, const float* wst, const float* vecs, float* out, int B, int T,
                             int ttiles, hipStream_t s);
hipError_t launch_fusion_attn_w(bool pe, const float* x, const float* ctx_img, const float* wst, const float* vecs,
                                float* x1, int B, int N, int tiles, int T, int ttiles, hipStream_t s);
hipError_t launch_fusion_ff_w(const float* x1, const float* wst, const float* vecs, float* x2, int B, int tiles, hipStream_t s);
hipError_t launch_ctx_prep_w_h2(bool pe, const float* ctx, const float* wst_h2, const float* vecs, float* out, int B, int T,
                                int ttiles, hipStream_t s, bool rowmajor = false);
hipError_t launch_fusion_attn_w_h2(bool pe, const float* x, const float* ctx_img, const float* wst_h2, const float* vecs,
                                   float* x1, int B, int N, int tiles, int T, int ttiles, hipStream_t s, bool tile_form = true);
hipError_t launch_fusion_ff_w_h2(const float* x1, const float* wst_h2, const float* vecs, float* x2, int B, int tiles, hipStream_t s,
                                 float* part = nullptr, int hs = 1, float* out_rm = nullptr, long o_sb = 0, long o_sr = 0,
                                 long o_sk = 0, int n_rows = 0, int* status = nullptr);
int plan_ff_split_w(int base_wgs);
// split: one workgroup per output (Q' + f | K | V); mode 3: corr_pos -> layer0 -> PointCN -> f only; ptab, v_scale, guard: as in
// ForwardBuffers and LayerRun, null / empty where the caller has none (it serves forms that build neither struct, so it takes the fields)
hipError_t launch_front_h2(int mode, bool split, const float* in, const float* wst, const float* vecs, float* f, float* q, float* k,
                           float* v, int B, int N, int tiles, const PairTab* ptab, unsigned* v_scale, PvGuard guard, hipStream_t s);
// all linear stages of one layer from f (k_linear_h2); roles: as two workgroup roles per row block (needs q); q null: no Q' image
// (LayerRun::qf_img); lr.kvf_vec non-null: "kv_fold" - q~ from the block's four stages and Wk^T bq', K and V become images of f
hipError_t launch_linear_h2(bool roles, bool one_product, const float* f, const float* ctx_img, float* q, float* k, float* v, float* x2,
                            int B, int N, int tiles, int T, int ttiles, const ForwardBuffers& fb, const LayerRun& lr, hipStream_t s);
// small grids: three launches per layer (k_small_front_fattn | k_small_attn_ff | k_scattn_merge); tile_role, tile_merge: the
// cross-attention role and the merge per query tile (Tuning::small_fattn_tile, Tuning::small_merge_tile)
hipError_t launch_small_front_fattn(bool tile_role, const float* f, const float* ctx_img, float* q, float* k, float* v, float* x1, int B,
                                    int N, int tiles, int T, int ttiles, const ForwardBuffers& fb, const LayerRun& lr, hipStream_t s);
hipError_t launch_small_attn_ff_merge(bool tile_merge, const float* q, const float* k, const float* v, const float* x1, float* ff_part,
                                      int ff_hs, float* out, int B, int N, int tiles, int ksplits, const ForwardBuffers& fb,
                                      const LayerRun& lr, hipStream_t s);
hipError_t launch_ctx_prep_h2(bool pe, const float* ctx, const float* wst, const float* vecs, float* out, int B, int T,
                              int ttiles, int sets, int wst_stride, int vec_stride, hipStream_t s, bool rowmajor = false);
hipError_t launch_fusion_attn_h2(bool pe, const float* x, const float* ctx_img, const float* wst, const float* vecs,
                                 float* x1, int B, int N, int tiles, int T, int ttiles, hipStream_t s, bool rowmajor = false);
// [r5] small grids: the forward's prologue as three launches of two roles each (encoder_h2.hip, k_pro_*)
hipError_t launch_pro_ctx_pts(const float* p_tokens, const float* wst, const float* vecs, float* f1ctx, int B, int T, int ttiles,
                              const float* src, const float* tgt, float* pts8, int N, hipStream_t s, const PairTab* ptab,
                              unsigned* zero_words, int n_zero);
hipError_t launch_pro_fattn_compat(const float* q_tokens, const float* f1ctx, const float* wst, const float* vecs, float* x1t, int B,
                                   int T, int ttiles, const float* pts8, float* c_dense, int N, int tiles, float sigma_d,
                                   hipStream_t s, const PairTab* ptab);
// hs > 1: the feed-forward role in hs hidden splits into `part`; the caller runs launch_ff_reduce_h2 next
hipError_t launch_pro_ff_front(const float* x1t, const float* wst, const float* vecs, float* imgfeat, int B, int ttiles, float* part,
                               int hs, const float* corr_pos, const float* fwst, const float* fvecs, float* f, float* q, float* k,
                               float* v, int N, int tiles, hipStream_t s, const PairTab* ptab, PvGuard guard);
hipError_t launch_ff_reduce_h2(const float* part, const float* x1, const float* vecs, float* x2, int B, int tiles, int hs, hipStream_t s);
// hs > 1: the 16 hidden chunks over hs workgroups per row block, partials in `part`, then the reduction
hipError_t launch_fusion_ff_h2(const float* x1, const float* wst, const float* vecs, float* x2, int B, int tiles, hipStream_t s,
                               float* part = nullptr, int hs = 1);
int padded_desc_width(int d);
hipError_t launch_nn_match(const float* F0, const float* F1, float* f0_img, float* f1_img, float* norm2, unsigned long long* best, int* idx,
                           float* dist, int N0, int N1, int d, int mode, hipStream_t s);
// Batched matching over B ragged pairs (gmf_nn_match_batched).  Pair b owns rows [row0, row0 + n0) of F0 and [key0, key0 + n1) of
// F1.  Its query rows are packed into whole 32-row tiles from tile `tile0` of the F0 image, its keys into whole stages from stage
// `stage0` of the F1 image (and of the norms), and its workgroups are [wg0, wg0 + wgx * ks): wgx query blocks of four tiles times ks
// key splits.  Entry B of the table holds the totals (an empty range), so every prefix search has its end.
struct MatchPair { int row0, n0, key0, n1, tile0, stage0, stages, wg0, wgx, ks, pad0, pad1; };
static_assert(sizeof(MatchPair) == 48, "tests/abi_cpp/host_table_host.cpp lays the correspondence table out with a 48-byte stand-in");
struct MatchTotals { long tiles0, stages, wgs, rows0; int tps; };
// fills tab[0 .. B] from the B + 1 host offsets; false: a pair has queries and no keys
bool plan_nn_match_batched(const int* off0, const int* off1, int B, int K, MatchPair* tab, MatchTotals* tot);
hipError_t launch_nn_match_batched(const float* F0, const float* F1, float* f0_img, float* f1_img, float* norm2, unsigned long long* best,
                                   const MatchPair* tab, int B, const MatchTotals& tot, int d, int mode, int global_index, int* idx,
                                   float* dist, hipStream_t s);
hipError_t launch_seed_dist(const float* featn_img, const int* seeds, float* dist, int B, int N, int S, hipStream_t s, const PairTab* ptab = nullptr);
hipError_t launch_pack_p32(const float* src, float* dst, int B, int n_rows, int K, long sb, long sr, long sk, hipStream_t s, const PairTab* ptab = nullptr);
// row-major [B, n_rows, 128] -> split-fp16 plane image (the operand image of launch_seed_dist)
hipError_t launch_pack_rows_h2(const float* src, float* dst, int B, int n_rows, hipStream_t s, const PairTab* ptab = nullptr,
                               const float* copy_src = nullptr, float* copy_dst = nullptr, long n_copy = 0);
hipError_t launch_unpack_p32(const float* src, float* dst, int B, int n_rows, int K, long sb, long sr, long sk, hipStream_t s, int* status = nullptr);
hipError_t launch_pack_pts8(const float* src, const float* tgt, float* dst, int B, int N, hipStream_t s, const PairTab* ptab = nullptr,
                            unsigned* zero_words = nullptr, int n_zero = 0);   // zero_words: n_zero words cleared by the same launch (PvGuard statistics)

// validation step (row f-4, forward half): validation_kernels.hip
size_t similarity_image_floats(int B, int N);
int sm_fused_parts_per_pair(int B, int N);
int sm_parts_per_pair(int B, int N);
int classification_parts(int B, int N);
int transformation_slices(int B, int N);
// sigma_dev (everywhere below): non-null = the kernels read sigma from this device address instead (gmf_set_sigma_device)
hipError_t launch_similarity_matrix(const float* feat_n, float* img, float* M, int B, int N, int ldm, float sigma,
                                    hipStream_t s, const float* sigma_dev = nullptr);
hipError_t launch_sm_loss_fused(const float* feat_n, const float* gt, float* img, double* part, double* pair_loss, int B,
                                int N, float sigma, int balanced, float* out, hipStream_t s, const float* sigma_dev = nullptr);
hipError_t launch_sm_loss(const float* M, int ldm, const float* gt, double* part, double* pair_loss, int B, int N,
                          int balanced, float* out, hipStream_t s);
int sm_backward_parts(int B, int N);
hipError_t launch_sm_backward(const float* feat_n, const float* gt, float* img, float* timg, float* consts, double* dsig_part,
                              int B, int N, float sigma, int balanced, float* dF, float* dsigma, hipStream_t s,
                              const float* sigma_dev = nullptr);
hipError_t launch_classification_loss(const float* pred, const float* gt, const float* weight, double* part, int B, int N,
                                      int balanced, float* out, hipStream_t s);
hipError_t launch_transformation_loss(const float* trans, const float* gt_trans, const float* src, const float* tgt,
                                      const float* probs, double* part, int B, int N, float re_thre, float te_thre,
                                      float* out, hipStream_t s);

// training primitives (row f-4): train_kernels.hip
int gemm_ksplits(bool ta, bool tb, const float* A, const float* B, int M, int N, int K, long lda, long ldb, long sA, long sB,
                 int batch);
hipError_t launch_gemm_f32(bool ta, bool tb, const float* A, const float* B, float* C, const float* bias, const float* R, int M, int N,
                           int K, long lda, long ldb, long ldc, long sA, long sB, long sC, int batch, float alpha, float* part,
                           int ksplits, int relu, hipStream_t s);
hipError_t launch_lcpe(bool backward, const float* x, const float* w, const float* bias, float* y, int rows, int L, int C, hipStream_t s);
hipError_t launch_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long rows, int C,
                         hipStream_t s);
hipError_t launch_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* dx_add,
                         float* dx, long rows, int C, hipStream_t s);
hipError_t launch_softmax(bool backward, const float* a, const float* b, const float* mul, float* out, long rows, int T, float scale,
                          hipStream_t s);
hipError_t launch_geglu(bool backward, const float* hdn, const float* dg, float* out, long rows, int H, hipStream_t s);
int colsum_chunks(long rows);
hipError_t launch_colsum(const float* x, const float* y, const float* mean, const float* rstd, const float* cmean, const float* crstd,
                         int center_x, int shift, int L, long rows, int C, float* part, float* out, hipStream_t s,
                         const float* relu_y = nullptr, bool dual = false, float* out2 = nullptr);
hipError_t launch_bn_finish(const float* sum, const float* sumsq, float* mean, float* rstd, float* run_mean, float* run_var, int C,
                            long rows, float eps, float momentum, hipStream_t s);
// y = relu?((x - mean) rstd gamma + beta (+ residual)); residual may be nullptr
hipError_t launch_bn_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* y,
                           long rows, int C, int relu, const float* residual, hipStream_t s);
hipError_t launch_bn_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* sdy,
                         const float* sdyx, float* dx, long rows, int C, hipStream_t s, const float* relu_y = nullptr);
hipError_t launch_relu_bwd(const float* dy, const float* y, float* out, long total, hipStream_t s);
hipError_t launch_bce_bwd(const float* pred, const float* gt, const float* weight, float* dpred, float* pw_scratch, int balanced,
                          long total, hipStream_t s);
hipError_t launch_sm_dense_bwd(const float* M, long ldm, const float* gt, float* consts, float* dM, int B, int N, int balanced,
                               hipStream_t s);
hipError_t launch_normalize(bool backward, const float* a, const float* dy, float* nrm, float* out, long rows, int C, hipStream_t s);
hipError_t launch_compat_dense(const float* src, const float* tgt, float* out, int B, int N, float sigma_d, hipStream_t s);
hipError_t launch_sim_bwd_G(const float* S, const float* dM, float* G, float* rowdsig, int B, int N, float sigma, hipStream_t s,
                            const float* sigma_dev = nullptr);

// image encoder epilogue (row f-1): image_kernels.hip
hipError_t launch_stem_h2(const float* x, long sb, long sc, long sh, long sw, const float* wimg, const float* bias, float* y,
                          int B, int H, int W, hipStream_t s, bool small_grid = true);   // small_grid: Tuning::conv_small
hipError_t launch_bias_relu_nhwc(float* y, const float* bias, const float* residual, long n_pixels, int C, hipStream_t s);
hipError_t launch_conv_nhwc_h2(const Tuning& tune, const float* x, const float* wimg, const float* bias, const float* residual, float* y, int B,
                               int H, int W, int cin, int cout, int ks, int stride, int relu, hipStream_t s);

}  // namespace gmf
