// One layer of a gmf_encoder_weights block as plain pointers (layer_weights), and the layout of a layer's "kv_fold" block, which the
// packer (gmf_pack.cpp, pack_kv_fold) writes and the forward reads by the same names.  Free of HIP.
#pragma once
#include "encoder_plan.hpp"

namespace gmf {

// A GMF_KV_FOLD_STRIDE block (gmf_encoder_weights::kv_fold): its pieces in order, in floats, and where each starts
constexpr size_t kKvfQWstFloats = 4 * kTileFloats;      // 4 split-fp16 stages of Wk^T Wq' (q~ = (Wk^T Wq') f + Wk^T bq')
constexpr size_t kKvfTailWstFloats = 5 * kTileFloats;   // 5 stages of fc_message, its first layer composed with projection_v: Wa Wv | Wb | Wc
constexpr size_t kKvfQBiasFloats = kC;                  // Wk^T bq'
constexpr size_t kKvfVecFloats = 2 * kC;                // Wq'^T bk [128] | bk . bq' [1, padded to 128]
constexpr size_t kKvfTailVecFloats = 2 * kC;            // the epilogue's vectors: Wa bv + ba [64] | bb [64] | bc [128]
constexpr size_t kKvfQWst = 0;
constexpr size_t kKvfTailWst = kKvfQWst + kKvfQWstFloats;
constexpr size_t kKvfQBias = kKvfTailWst + kKvfTailWstFloats;
constexpr size_t kKvfVec = kKvfQBias + kKvfQBiasFloats;
constexpr size_t kKvfTailVec = kKvfVec + kKvfVecFloats;
static_assert(kKvfTailVec + kKvfTailVecFloats == GMF_KV_FOLD_STRIDE, "the pieces of a kv_fold block add up to its stride");

// Layer l's weights.  *_h2: the split-fp16 image of the same weights (null when the block has none).
struct LayerWeights {
  const float *front_wst, *front_wst_h2, *front_vec;   // PointCN, then Q' | K | V
  const float *q_wst_h2, *q_bias;                      // ... the four Q' stages and bq' inside them
  const float *ctx_wst, *ctx_wst_h2, *ctx_vec;         // Fusion-2: context side,
  int ctx_wst_step, ctx_vec_step;                      // ... floats to the next layer's (one launch prepares every layer's context)
  const float *attn_wst, *attn_wst_h2, *attn_vec;      // cross-attention,
  const float *ff_wst, *ff_wst_h2, *ff_vec;            // feed-forward
  const float *tail_wst, *tail_wst_h2, *tail_vec;      // fc_message
  const float *next_wst_h2, *next_bias;                // the NEXT layer's PointCN (4 split-fp16 stages + bias); null: this is the last layer
  const float* pv_thr2;                                // this layer's entry of pv_guard; null: no thresholds
  // the pieces of this layer's kv_fold block, by the names above; null: the block has none
  const float *kvf_q_wst, *kvf_tail_wst, *kvf_q_bias, *kvf_vec, *kvf_tail_vec;
};

inline LayerWeights layer_weights(const gmf_encoder_weights* w, int l) {
  auto at = [l](const float* base, size_t stride) { return base ? base + (size_t)l * stride : nullptr; };
  LayerWeights r{};
  r.front_wst = at(w->front_wst, w->front_wst_stride);
  r.front_wst_h2 = at(w->front_wst_h2, w->front_wst_stride);
  r.front_vec = at(w->front_vec, w->front_vec_stride);
  r.q_wst_h2 = r.front_wst_h2 ? r.front_wst_h2 + 4 * kTileFloats : nullptr;
  r.q_bias = r.front_vec ? r.front_vec + kC : nullptr;
  r.ctx_wst = at(w->ctx_wst, w->ctx_wst_stride);
  r.ctx_wst_h2 = at(w->ctx_wst_h2, w->ctx_wst_stride);
  r.ctx_vec = at(w->ctx_vec, w->ctx_vec_stride);
  r.ctx_wst_step = w->ctx_wst_stride;
  r.ctx_vec_step = w->ctx_vec_stride;
  r.attn_wst = at(w->attn_wst, w->attn_wst_stride);
  r.attn_wst_h2 = at(w->attn_wst_h2, w->attn_wst_stride);
  r.attn_vec = at(w->attn_vec, w->attn_vec_stride);
  r.ff_wst = at(w->ff_wst, w->ff_wst_stride);
  r.ff_wst_h2 = at(w->ff_wst_h2, w->ff_wst_stride);
  r.ff_vec = at(w->ff_vec, w->ff_vec_stride);
  r.tail_wst = at(w->tail_wst, w->tail_wst_stride);
  r.tail_wst_h2 = at(w->tail_wst_h2, w->tail_wst_stride);
  r.tail_vec = at(w->tail_vec, w->tail_vec_stride);
  if (l + 1 < w->num_layers) {
    r.next_wst_h2 = w->front_wst_h2 ? r.front_wst_h2 + w->front_wst_stride : nullptr;
    r.next_bias = w->front_vec ? r.front_vec + w->front_vec_stride : nullptr;
  }
  r.pv_thr2 = at(w->pv_guard, 1);
  if (const float* kvf = at(w->kv_fold, GMF_KV_FOLD_STRIDE)) {
    r.kvf_q_wst = kvf + kKvfQWst;
    r.kvf_tail_wst = kvf + kKvfTailWst;
    r.kvf_q_bias = kvf + kKvfQBias;
    r.kvf_vec = kvf + kKvfVec;
    r.kvf_tail_vec = kvf + kKvfTailVec;
  }
  return r;
}

}  // namespace gmf
