// C ABI of libgmf_hip.so, the encoder family (see include/gmf_hip.h): the packing helpers, the staged entry points, the encoder
// forward (uniform and ragged), one NonLocalBlock and one FusionLayer.  The launch decisions of a forward are made once, in
// plan_encoder (encoder_plan.hpp); this file reserves the workspace and issues the launches the plan names.
#include <algorithm>
#include <string>

#include "api_common.hpp"

extern "C" {

int gmf_pack_rows_p32(gmf_handle* h, const float* src, long long sb, long long sr, long long sk, int B, int n_rows,
                      int K, float* dst, gmf_stream_t stream) {
  GMF_REQUIRE(h && src && dst, GMF_ERR_BAD_ARG, "pack_rows_p32: null pointer");
  GMF_REQUIRE(B > 0 && n_rows > 0 && K > 0 && K % 8 == 0, GMF_ERR_UNSUPPORTED_SHAPE, "pack_rows_p32: K must be a positive multiple of 8");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_pack_p32(src, dst, B, n_rows, K, sb, sr, sk, S(stream)));
  return GMF_OK;
}

int gmf_unpack_rows_p32(gmf_handle* h, const float* src_img, int B, int n_rows, int K, float* dst, long long sb,
                        long long sr, long long sk, gmf_stream_t stream) {
  GMF_REQUIRE(h && src_img && dst, GMF_ERR_BAD_ARG, "unpack_rows_p32: null pointer");
  GMF_REQUIRE(B > 0 && n_rows > 0 && K > 0 && K % 8 == 0, GMF_ERR_UNSUPPORTED_SHAPE, "unpack_rows_p32: K must be a positive multiple of 8");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_unpack_p32(src_img, dst, B, n_rows, K, sb, sr, sk, S(stream)));
  return GMF_OK;
}

int gmf_pack_pts8(gmf_handle* h, const float* src, const float* tgt, int B, int N, float* dst, gmf_stream_t stream) {
  GMF_REQUIRE(h && src && tgt && dst, GMF_ERR_BAD_ARG, "pack_pts8: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "pack_pts8: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_pack_pts8(src, tgt, dst, B, N, S(stream)));
  return GMF_OK;
}

// ---------------------------------------------------------------------------------------------
int gmf_front_forward(gmf_handle* h, int first, const float* in, const float* wst, const float* vecs, float* f,
                      float* q, float* k, float* v, int B, int N, gmf_stream_t stream) {
  GMF_REQUIRE(h && in && wst && vecs && f && q && k && v, GMF_ERR_BAD_ARG, "front_forward: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "front_forward: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_front(first ? 1 : 0, in, wst, vecs, f, q, k, v, B, N, tiles_of(N), S(stream)));
  return GMF_OK;
}

int gmf_scattn_forward(gmf_handle* h, const float* q, const float* k, const float* v, const float* pts8,
                       const float* fusion2_out, const float* wst, const float* vecs, float* out, int B, int N,
                       float sigma_d, gmf_stream_t stream) {
  GMF_REQUIRE(h && q && k && v && pts8 && fusion2_out && wst && vecs && out, GMF_ERR_BAD_ARG, "scattn_forward: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "scattn_forward: empty input");
  GMF_REQUIRE(sigma_d > 0.f, GMF_ERR_BAD_ARG, "scattn_forward: sigma_d must be positive");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_scattn_fp32(q, k, v, pts8, fusion2_out, wst, vecs, out, B, N, tiles_of(N), sigma_d, S(stream)));
  return GMF_OK;
}

int gmf_scattn_forward_dense(gmf_handle* h, const float* q, const float* k, const float* v, const float* attention,
                             const float* fusion2_out, const float* wst, const float* vecs, float* out, int B, int N,
                             gmf_stream_t stream) {
  GMF_REQUIRE(h && q && k && v && attention && fusion2_out && wst && vecs && out, GMF_ERR_BAD_ARG, "scattn_forward_dense: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "scattn_forward_dense: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_scattn_dense(q, k, v, attention, fusion2_out, wst, vecs, out, B, N, tiles_of(N), S(stream)));
  return GMF_OK;
}

int gmf_fusion_ctx_prepare(gmf_handle* h, int pe, const float* ctx, const float* wst, const float* vecs, float* out,
                           int B, int T, int sets, int wst_stride, int vec_stride, gmf_stream_t stream) {
  GMF_REQUIRE(h && ctx && wst && vecs && out, GMF_ERR_BAD_ARG, "fusion_ctx_prepare: null pointer");
  GMF_REQUIRE(B > 0 && T > 0 && sets > 0, GMF_ERR_UNSUPPORTED_SHAPE, "fusion_ctx_prepare: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_ctx_prep(pe != 0, ctx, wst, vecs, out, B, T, tiles_of(T), sets, wst_stride, vec_stride, S(stream)));
  return GMF_OK;
}

int gmf_fusion_attn_forward(gmf_handle* h, int pe, const float* x, const float* ctx_img, const float* wst,
                            const float* vecs, float* x1, int B, int N, int T, gmf_stream_t stream) {
  GMF_REQUIRE(h && x && ctx_img && wst && vecs && x1, GMF_ERR_BAD_ARG, "fusion_attn_forward: null pointer");
  GMF_REQUIRE(B > 0 && N > 0 && T > 0, GMF_ERR_UNSUPPORTED_SHAPE, "fusion_attn_forward: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_fusion_attn(pe != 0, x, ctx_img, wst, vecs, x1, B, N, tiles_of(N), T, tiles_of(T), S(stream)));
  return GMF_OK;
}

int gmf_fusion_ff_forward(gmf_handle* h, const float* x1, const float* wst, const float* vecs, float* x2, int B,
                          int N, gmf_stream_t stream) {
  GMF_REQUIRE(h && x1 && wst && vecs && x2, GMF_ERR_BAD_ARG, "fusion_ff_forward: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "fusion_ff_forward: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_fusion_ff(x1, wst, vecs, x2, B, tiles_of(N), S(stream)));
  return GMF_OK;
}

int gmf_classifier_forward(gmf_handle* h, const float* feat_img, const float* wst, const float* vecs, float* logits,
                           float* feat_n, float* feat, int B, int N, gmf_stream_t stream) {
  GMF_REQUIRE(h && feat_img && wst && vecs && logits && feat_n, GMF_ERR_BAD_ARG, "classifier_forward: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "classifier_forward: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_head(feat_img, wst, vecs, logits, feat_n, feat, B, N, tiles_of(N), S(stream), h->status_dev));
  return GMF_OK;
}

// ---------------------------------------------------------------------------------------------
static int check_weights(gmf_handle* h, const gmf_encoder_weights* w) {
  GMF_REQUIRE(w, GMF_ERR_BAD_ARG, "encoder weights: null");
  GMF_REQUIRE(w->num_layers >= 0 && w->num_layers <= 64, GMF_ERR_BAD_ARG, "encoder weights: bad num_layers");
  GMF_REQUIRE(w->sigma_d > 0.f, GMF_ERR_BAD_ARG, "encoder weights: sigma_d must be positive");
  return GMF_OK;
}

// compute units of the current device (256 on MI355X); queried once per process and device
static int cu_count() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  static int cached[16] = {0};
  if (dev >= 0 && dev < 16 && cached[dev] > 0) return cached[dev];
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  if (dev >= 0 && dev < 16) cached[dev] = n;
  return n;
}

// in-situ profiling: an event pair around the attention launch(es) of a layer, recorded on the caller's stream
static int prof_begin(gmf_handle* h, hipStream_t st, hipEvent_t* ev0, hipEvent_t* ev1) {
  *ev0 = *ev1 = nullptr;
  if (!h->profile) return GMF_OK;
  if (h->prof_used == h->prof_events.size()) {
    hipEvent_t a, b;
    GMF_HIP(hipEventCreate(&a));
    GMF_HIP(hipEventCreate(&b));
    h->prof_events.emplace_back(a, b);
  }
  *ev0 = h->prof_events[h->prof_used].first;
  *ev1 = h->prof_events[h->prof_used].second;
  ++h->prof_used;
  GMF_HIP(hipEventRecord(*ev0, st));
  return GMF_OK;
}

// Everything layer `l` of a forward fixes, from the plan, the layer's view of the weights and the forward's buffers: the guard's words,
// where the attention finds Q' (an image, or the weights to project it from f), the epilogue's fc_message and, under "kv_fold", the
// composed pieces in their place.  The forms that have no such thing (kFp32, kStages: no guard, no fold) leave it empty.
static gmf::LayerRun layer_run(const EncoderPlan& p, const gmf_encoder_weights* w, int l, int B, const float* f, unsigned* fstat,
                               float* c_dense_fb, const float* pts8) {
  gmf::LayerRun r;
  r.w = gmf::layer_weights(w, l);
  r.epi_wst = r.w.tail_wst_h2;
  r.epi_vec = r.w.tail_vec;
  if (p.fused()) { r.epi_next_wst = r.w.next_wst_h2; r.epi_next_bias = r.w.next_bias; }
  // the guard's statistics: f_0's is raised by the front kernel, f_{l+1}'s by the attention epilogue / merge kernels of layer l -
  // always before the kernels that read it
  if (p.guard) r.guard = gmf::PvGuard{fstat + (size_t)l * B * gmf::kPvStatStride, r.w.pv_thr2, fstat + (size_t)(l + 1) * B * gmf::kPvStatStride};
  if (p.q_in_attn) { r.qf_img = f; r.qw_wst = r.w.q_wst_h2; r.qw_bias = r.w.q_bias; }
  if (p.kv_fold) {
    r.qf_img = f;                                  // (beta comes from the f tile with or without a Q' image)
    r.qw_wst = p.q_in_attn ? r.w.kvf_q_wst : nullptr;
    r.qw_bias = p.q_in_attn ? r.w.kvf_q_bias : nullptr;
    r.epi_wst = r.w.kvf_tail_wst;
    r.epi_vec = r.w.kvf_tail_vec;                 // the epilogue's vectors with Wa bv + ba
    r.kvf_vec = r.w.kvf_vec;
  }
  // "compat_16": a pair that trips the guard at this layer for the first time gets its fp32 cache from one more role of the layer's
  // linear launch (fstat[l] is complete: the front kernel / the previous layer's attention and merge raised it)
  if (p.c16_guard) r.lazy = gmf::LazyCompat{c_dense_fb, pts8, fstat, w->pv_guard, l, 1.0f / (w->sigma_d * w->sigma_d)};
  return r;
}

// The attention launch of a layer (bracketed by the in-situ profiling events when enabled): the dense-`attention` drop-in, the
// pipelined kernel, the split-fp16 kernel of the kStages form (c from the cache when there is one, else recomputed), or fp32.
static int run_scattn(gmf_handle* h, const EncoderPlan& p, const gmf::ForwardBuffers& fb, const gmf::LayerRun& lr, float sigma_d,
                      const float* q, const float* k, const float* v, const float* pts8, const float* x2, float* out, int B, int N,
                      hipStream_t st, const float* dense_compat) {
  const int tiles = tiles_of(N);
  const float *wst = lr.w.tail_wst, *vecs = lr.epi_vec;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (int rc = prof_begin(h, st, &ev0, &ev1)) return rc;
  if (dense_compat) GMF_HIP(gmf::launch_scattn_dense(q, k, v, dense_compat, x2, wst, vecs, out, B, N, tiles, st));
  else if (p.pipelined) GMF_HIP(gmf::launch_scattn_h2p(q, k, v, x2, out, B, N, tiles, fb, lr, p.attn_nf, p.attn_ks, st));
  else if (p.form == EncoderPlan::kStages)
    GMF_HIP(gmf::launch_scattn_h2(q, k, v, pts8, x2, wst, vecs, out, B, N, tiles, sigma_d, st, fb.dense));
  else GMF_HIP(gmf::launch_scattn_fp32(q, k, v, pts8, x2, wst, vecs, out, B, N, tiles, sigma_d, st));
  if (ev1) GMF_HIP(hipEventRecord(ev1, st));
  return GMF_OK;
}

// Runs Fusion-2 + the spatial-consistency block of a layer given f,q,k,v (the kFp32 and kStages forms).
static int run_block_tail(gmf_handle* h, const EncoderPlan& p, const gmf::ForwardBuffers& fb, const gmf::LayerRun& lr, float sigma_d,
                          const float* f, const float* q, const float* k, const float* v, const float* pts8, const float* ctx_l,
                          float* x1, float* x2, float* out, int B, int N, int T, hipStream_t st, const float* dense_compat) {
  const int tiles = tiles_of(N), tt = tiles_of(T);
  if (p.form == EncoderPlan::kStages) {
    GMF_HIP(gmf::launch_fusion_attn_h2(true, f, ctx_l, lr.w.attn_wst_h2, lr.w.attn_vec, x1, B, N, tiles, T, tt, st));
    GMF_HIP(gmf::launch_fusion_ff_h2(x1, lr.w.ff_wst_h2, lr.w.ff_vec, x2, B, tiles, st, fb.part_o, p.ff_hs));   // the attention's partial buffer is free here
  } else {
    GMF_HIP(gmf::launch_fusion_attn(true, f, ctx_l, lr.w.attn_wst, lr.w.attn_vec, x1, B, N, tiles, T, tt, st));
    GMF_HIP(gmf::launch_fusion_ff(x1, lr.w.ff_wst, lr.w.ff_vec, x2, B, tiles, st));
  }
  return run_scattn(h, p, fb, lr, sigma_d, q, k, v, pts8, x2, out, B, N, st, dense_compat);
}

static int encoder_forward_impl(gmf_handle* h, const gmf_encoder_weights* w, const float* corr_pos, const float* src_keypts,
                                const float* tgt_keypts, const float* p_tokens, const float* q_tokens, int B, int N, int T,
                                float* logits, float* feat_n, float* feat, gmf_stream_t stream, const int* n_points);

int gmf_encoder_forward(gmf_handle* h, const gmf_encoder_weights* w, const float* corr_pos, const float* src_keypts,
                        const float* tgt_keypts, const float* p_tokens, const float* q_tokens, int B, int N, int T,
                        float* logits, float* feat_n, float* feat, gmf_stream_t stream) {
  GMF_REQUIRE(h, GMF_ERR_BAD_ARG, "encoder_forward: null handle");
  GMF_REQUIRE(B > 0 && N > 0 && T > 0, GMF_ERR_UNSUPPORTED_SHAPE, "encoder_forward: empty input");
  return encoder_forward_impl(h, w, corr_pos, src_keypts, tgt_keypts, p_tokens, q_tokens, B, N, T, logits, feat_n, feat, stream, nullptr);
}

int gmf_encoder_forward_ragged(gmf_handle* h, const gmf_encoder_weights* w, const float* corr_pos, const float* src_keypts,
                               const float* tgt_keypts, const float* p_tokens, const float* q_tokens, const int* n_points, int B,
                               int T, float* logits, float* feat_n, float* feat, gmf_stream_t stream) {
  GMF_REQUIRE(h, GMF_ERR_BAD_ARG, "encoder_forward_ragged: null handle");
  GMF_REQUIRE(n_points, GMF_ERR_BAD_ARG, "encoder_forward_ragged: null n_points");
  GMF_REQUIRE(B > 0 && T > 0, GMF_ERR_UNSUPPORTED_SHAPE, "encoder_forward_ragged: empty input");
  return encoder_forward_impl(h, w, corr_pos, src_keypts, tgt_keypts, p_tokens, q_tokens, B, 0, T, logits, feat_n, feat, stream, n_points);
}

static int encoder_forward_impl(gmf_handle* h, const gmf_encoder_weights* w, const float* corr_pos, const float* src_keypts,
                                const float* tgt_keypts, const float* p_tokens, const float* q_tokens, int B, int N, int T,
                                float* logits, float* feat_n, float* feat, gmf_stream_t stream, const int* n_points) {
  if (int rc = check_weights(h, w)) return rc;
  GMF_REQUIRE(corr_pos && src_keypts && tgt_keypts && p_tokens && q_tokens && logits && feat_n, GMF_ERR_BAD_ARG,
              "encoder_forward: null pointer");
  SetDevice sd(h, stream);
  hipStream_t st = S(stream);
  // ragged batch: per-pair sizes from the host; every image keeps a slot of tiles(max n) tiles per pair
  const bool ragged = n_points != nullptr;
  int min_tiles = 0;
  HostTable tab;
  const HostPart<gmf::PairTab> pairs = tab.add<gmf::PairTab>(ragged ? (size_t)B : 0);
  RingTaken ring;
  if (ragged) {
    long long n_sum = 0;
    if (int rc = check_ragged_sizes(h, n_points, B)) return rc;
    if (int rc = ring_take(h, tab, &ring)) return rc;
    gmf::plan_pair_table(n_points, B, -1.0, 0, pairs.host(ring.host), &N, &n_sum, nullptr);
    min_tiles = tiles_of(*std::min_element(n_points, n_points + B));
  }
  const int L = w->num_layers;
  const int tiles = tiles_of(N), tt = tiles_of(T);
  const EncoderPlan p = plan_encoder(h->tune, w, B, N, T, L, min_tiles, cu_count());
  // checked BEFORE the workspace is reserved and anything is launched
  GMF_REQUIRE(p.fused() || !ragged, GMF_ERR_UNSUPPORTED_SHAPE,
              "encoder_forward_ragged: ragged batches run on the default path only (split-fp16 weight images, at least two layers, the "
              "compat cache, \"fused_linear\" = 1, \"scattn_variant\" = 18)");
  const size_t act = p.act, tok = p.tok;
  char* dtab;
  float *featA, *featB, *f, *q, *k, *v, *x1, *x2, *pts8, *pimg, *qimg, *f1ctx, *x1t, *imgfeat, *ctxall, *c_dense, *c_dense_fb, *ff_part,
      *part_o, *part_ml;
  unsigned *v_scale, *fstat;
  if (int rc = arena_carve(h, {arena_buf(dtab, tab.bytes()), arena_buf(featA, act), arena_buf(featB, act), arena_buf(f, act),
                               arena_buf(q, act), arena_buf(k, act), arena_buf(v, act), arena_buf(x1, act), arena_buf(x2, act),
                               arena_buf(pts8, (size_t)B * tiles * 32 * 8), arena_buf(pimg, tok), arena_buf(qimg, tok),
                               arena_buf(f1ctx, tok), arena_buf(x1t, tok), arena_buf(imgfeat, tok),
                               arena_buf(ctxall, (size_t)(L > 0 ? L : 1) * tok),
                               // scale words of the V and K images' e4m3 planes ("pv_fp8"): per tile [V: 64 | K: 64]
                               arena_buf(v_scale, (size_t)B * tiles * 128),
                               // "pv_fp8" guard: [layer][pair] max row |f_l|^2 (float bits), one 128-byte line per pair
                               arena_buf(fstat, (size_t)(L + 1) * B * gmf::kPvStatStride),
                               arena_buf(c_dense, p.cache_floats),
                               arena_buf(c_dense_fb, p.cache_fb_floats),      // "compat_16": the fp32 cache of the pairs the guard trips
                               // small grids: feed-forward partials beside the attention's
                               arena_buf(ff_part, p.max_splits == 8 ? 8 * act : 0),
                               arena_buf(part_o, p.max_splits * act),
                               arena_buf(part_ml, (size_t)p.max_splits * B * tiles * 64)}))
    return rc;
  if (int rc = ragged ? ring_upload(h, ring, dtab, st) : GMF_OK) return rc;
  const gmf::PairTab* const ptab = ragged ? pairs.dev(dtab) : nullptr;
  gmf::ForwardBuffers fb;
  fb.dense = c_dense;
  fb.fmt = p.fmt;
  fb.half = p.half;
  fb.dense_fb = p.c16_guard ? c_dense_fb : nullptr;
  fb.part_o = part_o;
  fb.part_ml = part_ml;
  fb.ptab = ptab;
  fb.v_scale = p.v_fp8 ? v_scale : nullptr;
  const gmf::LayerWeights w0 = gmf::layer_weights(w, 0);   // layer 0's PointCN runs in front of the loop; the context launch starts from its weights
  unsigned* const zero_words = p.clear_stats ? fstat : nullptr;
  const int n_zero = p.clear_stats ? (L + 1) * B * gmf::kPvStatStride : 0;
  if (p.prologue) {
    GMF_HIP(gmf::launch_pro_ctx_pts(p_tokens, w->f1_ctx_wst_h2, w->f1_ctx_vec, f1ctx, B, T, tt, src_keypts, tgt_keypts, pts8, N, st, ptab,
                                    zero_words, n_zero));
    GMF_HIP(gmf::launch_pro_fattn_compat(q_tokens, f1ctx, w->f1_attn_wst_h2, w->f1_attn_vec, x1t, B, T, tt, pts8, c_dense, N, tiles,
                                         w->sigma_d, st, ptab));
    gmf::PvGuard g0;
    if (p.guard) g0.stat_next = fstat;
    GMF_HIP(gmf::launch_pro_ff_front(x1t, w->f1_ff_wst_h2, w->f1_ff_vec, imgfeat, B, tt, part_o, p.f1_ff_hs, corr_pos, w0.front_wst_h2,
                                     w0.front_vec, f, q, k, v, N, tiles, st, ptab, g0));
    if (p.f1_ff_hs > 1) GMF_HIP(gmf::launch_ff_reduce_h2(part_o, x1t, w->f1_ff_vec, imgfeat, B, tt, p.f1_ff_hs, st));
    GMF_HIP(gmf::launch_ctx_prep_h2(true, imgfeat, w0.ctx_wst_h2, w0.ctx_vec, ctxall, B, T, tt, L, w0.ctx_wst_step, w0.ctx_vec_step, st));
  } else {
    // Fusion-1: image_feat = FusionLayer(p_tok (context), queries = q_tok), pe = False (PointDSC.py:137)
    if (p.f1_h2) {
      // (the two token tensors are read row-major: no packing launches in front of these few-workgroup kernels)
      GMF_HIP(gmf::launch_ctx_prep_h2(false, p_tokens, w->f1_ctx_wst_h2, w->f1_ctx_vec, f1ctx, B, T, tt, 1, 0, 0, st, true));
      GMF_HIP(gmf::launch_fusion_attn_h2(false, q_tokens, f1ctx, w->f1_attn_wst_h2, w->f1_attn_vec, x1t, B, T, tt, T, tt, st, true));
      GMF_HIP(gmf::launch_fusion_ff_h2(x1t, w->f1_ff_wst_h2, w->f1_ff_vec, imgfeat, B, tt, st, part_o, p.f1_ff_hs));
    } else {
      GMF_HIP(gmf::launch_pack_p32(p_tokens, pimg, B, T, kC, (long)T * kC, kC, 1, st));
      GMF_HIP(gmf::launch_pack_p32(q_tokens, qimg, B, T, kC, (long)T * kC, kC, 1, st));
      GMF_HIP(gmf::launch_ctx_prep(false, pimg, w->f1_ctx_wst, w->f1_ctx_vec, f1ctx, B, T, tt, 1, 0, 0, st));
      GMF_HIP(gmf::launch_fusion_attn(false, qimg, f1ctx, w->f1_attn_wst, w->f1_attn_vec, x1t, B, T, tt, T, tt, st));
      GMF_HIP(gmf::launch_fusion_ff(x1t, w->f1_ff_wst, w->f1_ff_vec, imgfeat, B, tt, st));
    }
    // context side of all L Fusion-2 layers in one launch
    if (L > 0) {
      if (p.form != EncoderPlan::kFp32) GMF_HIP(gmf::launch_ctx_prep_h2(true, imgfeat, w0.ctx_wst_h2, w0.ctx_vec, ctxall, B, T, tt, L,
                                                                         w0.ctx_wst_step, w0.ctx_vec_step, st));
      else GMF_HIP(gmf::launch_ctx_prep(true, imgfeat, w0.ctx_wst, w0.ctx_vec, ctxall, B, T, tt, L, w0.ctx_wst_step, w0.ctx_vec_step, st));
    }
    GMF_HIP(gmf::launch_pack_pts8(src_keypts, tgt_keypts, pts8, B, N, st, ptab, zero_words, n_zero));
    if (p.cache) GMF_HIP(gmf::launch_compat_build(pts8, c_dense, B, N, tiles, w->sigma_d, p.fmt, st, ptab));
  }

  float* cur = featA;
  float* nxt = featB;
  // The fused forms (the default): the layer's PointCN runs in the PREVIOUS layer's attention epilogue (layer 0: a small f-only
  // kernel).  kLinear, two launches per layer:
  //   k_linear_h2 : f -> Q', K, V (split-fp16 images) and x2 = Fusion-2(f)
  //   k_scattn_h2p: Q', K, V, c, x2 -> f_{l+1} = ReLU(PointCN_{l+1}(fc_message(attention) + x2))   (last layer: the features)
  if (p.fused()) {
    if (!p.prologue) {                            // (small grids: the prologue's third launch ran it)
      gmf::PvGuard g0;
      if (p.guard) g0.stat_next = fstat;
      GMF_HIP(gmf::launch_front_h2(3, p.front_split, corr_pos, w0.front_wst_h2, w0.front_vec, f, q, k, v, B, N, tiles, ptab, nullptr, g0, st));
    }
    for (int l = 0; l < L; ++l) {
      const gmf::LayerRun lr = layer_run(p, w, l, B, f, fstat, c_dense_fb, pts8);
      const float* ctx_l = ctxall + (size_t)l * tok;
      float* const out = (l + 1 == L) ? cur : f;   // every layer but the last: f_{l+1}, written by the attention epilogue / the merge
      if (p.form == EncoderPlan::kLinear) {
        GMF_HIP(gmf::launch_linear_h2(p.roles, p.one_product, f, ctx_l, p.q_in_attn ? nullptr : q, k, v, x2, B, N, tiles, T, tt, fb, lr, st));
      } else if (p.form == EncoderPlan::kSmall3) {
        // three launches: {Q' | K | V | cross-attention} -> {key-split attention | hidden-split feed-forward} -> merge
        GMF_HIP(gmf::launch_small_front_fattn(h->tune.small_fattn_tile, f, ctx_l, q, k, v, x1, B, N, tiles, T, tt, fb, lr, st));
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (int rc = prof_begin(h, st, &e0, &e1)) return rc;
        GMF_HIP(gmf::launch_small_attn_ff_merge(h->tune.small_merge_tile, q, k, v, x1, ff_part, p.ff_hs, out, B, N, tiles, p.attn_ks, fb, lr, st));
        if (e1) GMF_HIP(hipEventRecord(e1, st));
        continue;
      } else {
        // (projecting Q'/K/V on a side stream beside the Fusion-2 kernels, forked and joined with events, was measured at
        // B = 1: 1.62 vs 1.58 ms at N = 5000, 1.08 vs 1.00 ms at N = 1000 - the event round trips cost more than the overlap gives)
        GMF_HIP(gmf::launch_front_h2(2, p.front_split, f, lr.w.front_wst_h2, lr.w.front_vec, f, q, k, v, B, N, tiles, nullptr, fb.v_scale, lr.guard, st));
        GMF_HIP(gmf::launch_fusion_attn_h2(true, f, ctx_l, lr.w.attn_wst_h2, lr.w.attn_vec, x1, B, N, tiles, T, tt, st));
        GMF_HIP(gmf::launch_fusion_ff_h2(x1, lr.w.ff_wst_h2, lr.w.ff_vec, x2, B, tiles, st, part_o, p.ff_hs));
      }
      if (int rc = run_scattn(h, p, fb, lr, w->sigma_d, q, k, v, pts8, x2, out, B, N, st, nullptr)) return rc;
    }
    GMF_HIP(gmf::launch_head(cur, w->head_wst, w->head_vec, logits, feat_n, feat, B, N, tiles, st, h->status_dev, ptab,
                             p.guard ? fstat : nullptr, p.guard ? w->pv_guard : nullptr, L));
    return GMF_OK;
  }
  if (L == 0) {
    // degenerate: features are layer0(corr_pos) only
    GMF_HIP(gmf::launch_front(1, corr_pos, w0.front_wst, w0.front_vec, cur, q, k, v, B, N, tiles, st));
  }
  for (int l = 0; l < L; ++l) {
    const gmf::LayerRun lr = layer_run(p, w, l, B, f, fstat, c_dense_fb, pts8);
    const float* in = (l == 0) ? corr_pos : cur;
    if (p.form == EncoderPlan::kStages)
      GMF_HIP(gmf::launch_front_h2(l == 0 ? 1 : 0, p.front_split, in, lr.w.front_wst_h2, lr.w.front_vec, f, q, k, v, B, N, tiles, nullptr, nullptr, {}, st));
    else GMF_HIP(gmf::launch_front(l == 0 ? 1 : 0, in, lr.w.front_wst, lr.w.front_vec, f, q, k, v, B, N, tiles, st));
    if (int rc = run_block_tail(h, p, fb, lr, w->sigma_d, f, q, k, v, pts8, ctxall + (size_t)l * tok, x1, x2, nxt, B, N, T, st, nullptr)) return rc;
    float* t = cur; cur = nxt; nxt = t;
  }
  GMF_HIP(gmf::launch_head(cur, w->head_wst, w->head_vec, logits, feat_n, feat, B, N, tiles, st, h->status_dev));
  return GMF_OK;
}

int gmf_nonlocal_block_forward(gmf_handle* h, const gmf_encoder_weights* w, int layer, int apply_pointcn,
                               const float* feat_img, const float* pts8, const float* attention,
                               const float* image_feat_img, float* out_img, int B, int N, int T, gmf_stream_t stream) {
  GMF_REQUIRE(h, GMF_ERR_BAD_ARG, "nonlocal_block_forward: null handle");
  if (int rc = check_weights(h, w)) return rc;
  GMF_REQUIRE(feat_img && image_feat_img && out_img, GMF_ERR_BAD_ARG, "nonlocal_block_forward: null pointer");
  GMF_REQUIRE((pts8 != nullptr) != (attention != nullptr), GMF_ERR_BAD_ARG, "nonlocal_block_forward: pass exactly one of pts8 / attention");
  GMF_REQUIRE(layer >= 0 && layer < w->num_layers, GMF_ERR_BAD_ARG, "nonlocal_block_forward: layer out of range");
  GMF_REQUIRE(B > 0 && N > 0 && T > 0, GMF_ERR_UNSUPPORTED_SHAPE, "nonlocal_block_forward: empty input");
  GMF_REQUIRE(apply_pointcn == 0 || apply_pointcn == 1, GMF_ERR_BAD_ARG, "nonlocal_block_forward: bad flag");
  SetDevice sd(h, stream);
  hipStream_t st = S(stream);
  const int tiles = tiles_of(N), tt = tiles_of(T);
  // one layer: no compat cache, so the kFp32 or kStages form (the dense-compat kernel consumes fp32 images: kFp32)
  const EncoderPlan p = plan_encoder(h->tune, w, B, N, T, 1, 0, cu_count(), attention != nullptr);
  float *f, *q, *k, *v, *x1, *x2, *ctx;
  if (int rc = arena_carve(h, {arena_buf(f, p.act), arena_buf(q, p.act), arena_buf(k, p.act), arena_buf(v, p.act), arena_buf(x1, p.act),
                               arena_buf(x2, p.act), arena_buf(ctx, p.tok)}))
    return rc;
  const gmf::LayerRun lr = layer_run(p, w, layer, B, f, nullptr, nullptr, pts8);   // (those forms: the layer's weights and nothing else)
  // apply_pointcn = 0: the caller's feat is already the block input (NonLocalBlock.forward, PointDSC.py:40-45)
  if (p.form == EncoderPlan::kStages) {
    GMF_HIP(gmf::launch_front_h2(apply_pointcn ? 0 : 2, p.front_split, feat_img, lr.w.front_wst_h2, lr.w.front_vec, f, q, k, v, B, N, tiles, nullptr, nullptr, {}, st));
    GMF_HIP(gmf::launch_ctx_prep_h2(true, image_feat_img, lr.w.ctx_wst_h2, lr.w.ctx_vec, ctx, B, T, tt, 1, 0, 0, st));
  } else {
    GMF_HIP(gmf::launch_front(apply_pointcn ? 0 : 2, feat_img, lr.w.front_wst, lr.w.front_vec, f, q, k, v, B, N, tiles, st));
    GMF_HIP(gmf::launch_ctx_prep(true, image_feat_img, lr.w.ctx_wst, lr.w.ctx_vec, ctx, B, T, tt, 1, 0, 0, st));
  }
  return run_block_tail(h, p, gmf::ForwardBuffers{}, lr, w->sigma_d, f, q, k, v, pts8, ctx, x1, x2, out_img, B, N, T, st, attention);
}

int gmf_fusion_layer_forward(gmf_handle* h, int pe, int latent_dim, int d_head, const float* ctx_wst, const float* ctx_vec,
                             const float* attn_wst, const float* attn_vec, const float* ff_wst, const float* ff_vec,
                             const float* data, const float* queries, long long q_sb, long long q_sr, long long q_sk,
                             float* out, long long o_sb, long long o_sr, long long o_sk, int B, int N, int T,
                             gmf_stream_t stream, const float* ff_wst_h2, const float* ctx_wst_h2, const float* attn_wst_h2) {
  GMF_REQUIRE(h && ctx_wst && ctx_vec && attn_wst && attn_vec && ff_wst && ff_vec && data && queries && out,
              GMF_ERR_BAD_ARG, "fusion_layer_forward: null pointer");
  GMF_REQUIRE((ctx_wst_h2 == nullptr) == (attn_wst_h2 == nullptr), GMF_ERR_BAD_ARG,
              "fusion_layer_forward: ctx_wst_h2 and attn_wst_h2 go together (the attention reads the context image the "
              "context kernel of the same kind writes)");
  GMF_REQUIRE(B > 0 && N > 0 && T > 0, GMF_ERR_UNSUPPORTED_SHAPE, "fusion_layer_forward: empty input");
  const bool narrow = (latent_dim == 128 && d_head == 64), wide = (latent_dim == 256 && d_head == 128);
  GMF_REQUIRE(narrow || wide, GMF_ERR_UNSUPPORTED_SHAPE,
              "fusion_layer_forward: kernels exist for (latent_dim, d_head) = (128, 64) and (256, 128), context dim 128");
  SetDevice sd(h, stream);
  hipStream_t st = S(stream);
  const int tiles = tiles_of(N), tt = tiles_of(T);
  const size_t act = (size_t)B * tiles * 32 * latent_dim;
  const size_t tok = (size_t)B * tt * kTileFloats;
  const size_t ctxsz = wide ? 2 * tok : tok;
  // small grids of the wide layer: the feed-forward's hidden chunks are split over hs workgroups per row block
  const int ff_hs_w = (wide && ff_wst_h2 && h->tune.ff_split != 1) ?
                          (h->tune.ff_split > 1 ? h->tune.ff_split : gmf::plan_ff_split_w(((tiles + 3) / 4) * B)) : 1;
  float *xin, *x1, *x2, *cimg, *ctx, *ff_part_w;
  if (int rc = arena_carve(h, {arena_buf(xin, act), arena_buf(x1, act), arena_buf(x2, act), arena_buf(cimg, tok), arena_buf(ctx, ctxsz),
                               arena_buf(ff_part_w, ff_hs_w > 1 ? (size_t)ff_hs_w * act : 0)}))
    return rc;
  // the split-fp16 kernels of the 256-wide layer read the context tokens row-major and (hidden-split feed-forward) write the
  // output through its strides: on the small grids this layer usually runs on, a packing pass is a launch like any other
  const bool wide_direct = wide && attn_wst_h2 != nullptr;
  if (!wide_direct) GMF_HIP(gmf::launch_pack_p32(data, cimg, B, T, kC, (long)T * kC, kC, 1, st));
  GMF_HIP(gmf::launch_pack_p32(queries, xin, B, N, latent_dim, q_sb, q_sr, q_sk, st));
  if (narrow) {
    if (attn_wst_h2) {
      GMF_HIP(gmf::launch_ctx_prep_h2(pe != 0, cimg, ctx_wst_h2, ctx_vec, ctx, B, T, tt, 1, 0, 0, st));
      GMF_HIP(gmf::launch_fusion_attn_h2(pe != 0, xin, ctx, attn_wst_h2, attn_vec, x1, B, N, tiles, T, tt, st));
    } else {
      GMF_HIP(gmf::launch_ctx_prep(pe != 0, cimg, ctx_wst, ctx_vec, ctx, B, T, tt, 1, 0, 0, st));
      GMF_HIP(gmf::launch_fusion_attn(pe != 0, xin, ctx, attn_wst, attn_vec, x1, B, N, tiles, T, tt, st));
    }
    if (ff_wst_h2) GMF_HIP(gmf::launch_fusion_ff_h2(x1, ff_wst_h2, ff_vec, x2, B, tiles, st));
    else GMF_HIP(gmf::launch_fusion_ff(x1, ff_wst, ff_vec, x2, B, tiles, st));
  } else {
    if (attn_wst_h2) {
      GMF_HIP(gmf::launch_ctx_prep_w_h2(pe != 0, data, ctx_wst_h2, ctx_vec, ctx, B, T, tt, st, true));
      GMF_HIP(gmf::launch_fusion_attn_w_h2(pe != 0, xin, ctx, attn_wst_h2, attn_vec, x1, B, N, tiles, T, tt, st, h->tune.wide_attn_tile));
    } else {
      GMF_HIP(gmf::launch_ctx_prep_w(pe != 0, cimg, ctx_wst, ctx_vec, ctx, B, T, tt, st));
      GMF_HIP(gmf::launch_fusion_attn_w(pe != 0, xin, ctx, attn_wst, attn_vec, x1, B, N, tiles, T, tt, st));
    }
    if (ff_wst_h2 && ff_hs_w > 1) {                 // the partials' reduction writes the caller's tensor
      GMF_HIP(gmf::launch_fusion_ff_w_h2(x1, ff_wst_h2, ff_vec, x2, B, tiles, st, ff_part_w, ff_hs_w, out, o_sb, o_sr, o_sk, N, h->status_dev));
      return GMF_OK;
    }
    if (ff_wst_h2) GMF_HIP(gmf::launch_fusion_ff_w_h2(x1, ff_wst_h2, ff_vec, x2, B, tiles, st, ff_part_w, ff_hs_w));
    else GMF_HIP(gmf::launch_fusion_ff_w(x1, ff_wst, ff_vec, x2, B, tiles, st));
  }
  GMF_HIP(gmf::launch_unpack_p32(x2, out, B, N, latent_dim, o_sb, o_sr, o_sk, st, h->status_dev));
  return GMF_OK;
}

}  // extern "C"
