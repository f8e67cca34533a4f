// The host plan of one encoder forward, free of HIP: the per-handle knobs (struct Tuning), every launch decision of a forward
// (EncoderPlan, plan_encoder) and the work splits behind them.  Pure integer logic over the knobs, the weight images present and
// the shape, so it runs as a program of its own under the host sanitizers (tests/abi_cpp/encoder_plan_host.cpp).
#pragma once
#include "../../include/gmf_hip.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>

constexpr int kC = 128;
constexpr size_t kTileFloats = 32 * kC;

inline int tiles_of(int n) { return (n + 31) / 32; }

namespace gmf {

// Per-handle tuning knobs (gmf_set_tuning).  Every value selects between forms that compute the same result up to
// rounding; there is no process-global state and no environment variable behind any of them.
struct Tuning {
  int scattn_variant = 18;   // 18 = cached, software-pipelined split-fp16 attention; 9 = split-fp16 without the pipelining
                             // (and without the cache when compat_cache = 0); 0 = fp32 MFMA path for every stage
  bool use_cache = true;     // compat cache (built once per batch) for variants 9 / 18
  int key_splits = 0;        // attention key splits: 0 = automatic (small grids, and the tail of large ones), 1 = off, n = forced
  bool tail_split = false;   // large grids: split the last partial round of attention workgroups by keys.  Off by default: a CU
                             // left with one resident workgroup runs it almost twice as fast, so the "half-empty last round" costs
                             // little (32 x 5000: 1.10 ms split vs 1.07 ms whole, measured)
  int ff_split = 0;          // feed-forward hidden splits on small grids: 0 = automatic, 1 = off, 2 / 4 / 8 = forced
  bool front_split = true;   // small grids: one workgroup per output (Q' + f | K | V) of k_front_h2
  bool wide_attn_tile = true;     // 256-wide layer: cross-attention with one workgroup per tile on grids of up to 256 tiles
  bool small_merge_tile = true;   // small grids: the merge step with one workgroup per query tile, its waves splitting the feature blocks
  bool small_fattn_tile = true;   // [r5] small grids: the cross-attention role of the layer's first launch per query tile, context tiles dealt to its waves
  bool small_roles = true;   // small grids: three launches per layer with two kinds of workgroups each (else five or six)
  bool fused_linear = true;  // one kernel per layer for Q'/K/V + Fusion-2 (k_linear_h2) with the next PointCN in the attention epilogue
  int conv_patch = 1;        // stride-1 3x3 convolutions: 1 = LDS patch kernel (automatic form), 2 = never three workgroups per CU, 0 = gather kernel
  bool small_prologue = true;   // [r5] small grids: the prologue's two chains as roles of shared launches
  bool conv_small = true;    // [r5] grids of fewer than 128 workgroups of the 128-pixel convolution kernels (a few images): the K-split kernel
  int nms_binned = 1;        // 1 = grid-binned NMS candidates on large grids, 2 = always, 0 = all pairs
  bool topk_select = true;   // radix select of the S seeds (false = full bitonic sort)
  int mid_grid_roles = 512;  // two-launch form on grids below this many base workgroups (>= 256): the linear kernel runs as two
                             // workgroup roles per row block (Q'/K/V | Fusion-2); 0 = never
  bool kv_fold = true;          // large grids (two-launch plan, parity numerics, fp32 cache): keys = values = the layer input f, the K and V
                                // projections composed into the query side and fc_message's first layer (false: the unfolded form, bit for bit)
  bool q_in_attention = true;   // [r4] large grids: Q' is projected in the attention kernel's prologue, not written by k_linear_h2 (bit-identical)
  int pv_fp8 = 1;            // parity arithmetic of the default path: the two cross products of O += P V on the block-scaled fp8 matrix
                             // pipe (scattn_h2p_body<3, *, true>).  1 = guarded per pair and layer on the device
                             // (PvGuard), 2 = unconditionally, 0 = all three products on the f16 pipe
  int compat_format = 0;     // element format of the compat cache on the cached, pipelined path: 0 = the plan's choice ("compat_16"); 2 =
                             // 16-bit fixed point, rint(65535 c), UNCONDITIONALLY: half the attention's c stream and half the build,
                             // absolute error <= 7.6e-6 on c.  Measured: inside the parity contract on 3DMatch-shape
                             // inputs, 4-8x the reference's own fp32 noise on ill-conditioned KITTI-shape inputs - so it is opt-in
  int compat_16 = 1;         // two-launch plan, parity numerics, the guarded fp8 form: the 16-bit cache under the "pv_fp8" guard - per pair
                             // and layer, 16 bits where the guard lets the fp8 products through, the exact fp32 cache (built on the device
                             // for the pairs that trip, once per forward) where it does not.  1 = on grids of 256 row blocks and more
                             // (default), 2 = on every grid of that plan, 0 = fp32 for everyone
  int precision = 0;         // NOT rounding-equivalent: 0 = parity numerics (fp32-equivalent split-fp16 products, the default);
                             // 1 = throughput numerics: the spatial-consistency attention multiplies plain
                             // fp16 operands (one product, fp32 accumulation) and streams c as fp16 - outside the 1e-4 gate
  int spectral_col_splits = 0;   // spectral matching: column splits of a pair's sweep, 0 = from the pair's N (launchers_spectral.hpp), 1..32 = forced
  int clique_local_rows = 384;   // maximum clique: a root with at most this many candidates is searched in LDS (launchers_clique.hpp), 0..384
};

// The knobs by their public names (include/gmf_hip.h documents each): the one table behind gmf_set_tuning and gmf_get_tuning.  A knob is
// an int or a bool field of Tuning (exactly one of i, b is set; a bool reads and writes as 0 / 1) and accepts a closed range lo..hi or,
// with n_only > 0, a short set.  knob_set marks an unused slot with -1: no knob of a set accepts a negative value.
struct Knob {
  const char* name;
  int Tuning::*i;
  bool Tuning::*b;
  int lo, hi;
  int only[5];
  int n_only;
};
constexpr Knob knob_flag(const char* name, bool Tuning::*f) { return {name, nullptr, f, 0, 0, {0, 1}, 2}; }
constexpr Knob knob_range(const char* name, int Tuning::*f, int lo, int hi) { return {name, f, nullptr, lo, hi, {}, 0}; }
constexpr Knob knob_set(const char* name, int Tuning::*f, int a, int b, int c = -1, int d = -1, int e = -1) {
  return {name, f, nullptr, 0, 0, {a, b, c, d, e}, 2 + (c >= 0) + (d >= 0) + (e >= 0)};
}
constexpr Knob kKnobs[] = {
    knob_set("scattn_variant", &Tuning::scattn_variant, 0, 9, 18),
    knob_flag("front_output_split", &Tuning::front_split),
    knob_set("ff_hidden_splits", &Tuning::ff_split, 0, 1, 2, 4, 8),
    knob_range("attn_key_splits", &Tuning::key_splits, 0, 8),
    knob_flag("attn_tail_split", &Tuning::tail_split),
    knob_flag("small_grid_roles", &Tuning::small_roles),
    knob_flag("fused_linear", &Tuning::fused_linear),
    knob_flag("compat_cache", &Tuning::use_cache),
    knob_range("conv_lds_patch", &Tuning::conv_patch, 0, 2),
    knob_flag("small_fattn_tile", &Tuning::small_fattn_tile),
    knob_flag("small_prologue_roles", &Tuning::small_prologue),
    knob_flag("conv_small_grid", &Tuning::conv_small),
    knob_range("nms_binned", &Tuning::nms_binned, 0, 2),
    knob_flag("topk_select", &Tuning::topk_select),
    knob_flag("wide_attn_tile", &Tuning::wide_attn_tile),
    knob_flag("small_merge_tile", &Tuning::small_merge_tile),
    knob_range("mid_grid_roles", &Tuning::mid_grid_roles, 0, 4096),
    knob_flag("q_in_attention", &Tuning::q_in_attention),
    knob_flag("kv_fold", &Tuning::kv_fold),
    knob_range("pv_fp8", &Tuning::pv_fp8, 0, 2),
    knob_set("compat_format", &Tuning::compat_format, 0, 2),
    knob_range("compat_16", &Tuning::compat_16, 0, 2),
    knob_range("precision", &Tuning::precision, 0, 2),
    knob_range("spectral_col_splits", &Tuning::spectral_col_splits, 0, 32),   // kSmMaxSplits (launchers_spectral.hpp)
    knob_range("clique_local_rows", &Tuning::clique_local_rows, 0, 384),      // kPmcLocal (launchers_clique.hpp)
};

inline const Knob* find_knob(const char* name) {
  for (const Knob& k : kKnobs)
    if (std::strcmp(name, k.name) == 0) return &k;
  return nullptr;
}

inline bool knob_accepts(const Knob& k, int value) {
  if (k.n_only == 0) return value >= k.lo && value <= k.hi;
  return std::find(k.only, k.only + k.n_only, value) != k.only + k.n_only;
}

// false: no such knob, or a value it does not accept (t is then unchanged); *why names the knob and what it accepts
inline bool set_knob(Tuning& t, const char* name, int value, std::string* why) {
  const Knob* k = find_knob(name);
  if (!k) { *why = std::string("unknown knob ") + name; return false; }
  if (!knob_accepts(*k, value)) {
    *why = std::string(name) + " must be ";
    if (k->n_only == 0) *why += "in " + std::to_string(k->lo) + ".." + std::to_string(k->hi);
    for (int j = 0; j < k->n_only; ++j) *why += (j == 0 ? "" : j + 1 == k->n_only ? " or " : ", ") + std::to_string(k->only[j]);
    return false;
  }
  if (k->b) t.*(k->b) = value != 0;
  else t.*(k->i) = value;
  return true;
}

// false: no such knob
inline bool get_knob(const Tuning& t, const char* name, int* value) {
  const Knob* k = find_knob(name);
  if (!k) return false;
  *value = k->b ? (t.*(k->b) ? 1 : 0) : t.*(k->i);
  return true;
}

}  // namespace gmf

// Work split of the attention grid (attn_item): W items on `slots` resident workgroups (2 per CU).  n_full = items per XCD
// that run whole; the rest are split `ksplits` ways by key range (ksplits = 1: none).
inline void plan_attn_split(const gmf::Tuning& tune, int cus, int W, int tiles, int max_splits, bool ragged, int* n_full_out,
                            int* ksplits_out) {
  const int slots = 2 * cus;
  const int per_xcd = (W >> 3) + ((W & 7) ? 1 : 0);
  int n_full = per_xcd, ksplits = 1;                                    // default: every item whole
  if (max_splits > 1 && tiles >= 8) {
    const int cap = std::min(max_splits, std::max(1, tiles / 4));
    if (tune.key_splits > 1) { n_full = 0; ksplits = std::min(tune.key_splits, cap); }             // forced: every item split
    else if (tune.key_splits == 0) {
      // small grid: ONE workgroup per CU - a workgroup alone on its CU runs its tiles almost twice as fast as two
      // co-resident ones (B = 1, N = 5000: 6 splits = 240 workgroups 1.64 ms per forward, 8 splits = 320 workgroups 1.75 ms)
      if (W < slots / 2) { n_full = 0; ksplits = std::min(std::max(2, (slots / 2) / W), cap); }
      else if (W < 3 * slots / 4 && tiles >= 64) { n_full = 0; ksplits = std::min(2, cap); }       // measured break-even
      else if (W > slots && tune.tail_split && !ragged) {
        // large grid: whole rounds run whole; a last partial round of at most half the slots is split to fill them (the split
        // tail assumes items of one length: not for ragged batches)
        const int full = (W / slots) * slots, rest = W - full;
        if (rest > 0 && 2 * rest <= slots && tiles >= 16) { n_full = full / 8; ksplits = std::min(std::min(slots / rest, 4), cap); }
      }
    }
    if (ksplits <= 1) { n_full = per_xcd; ksplits = 1; }
  }
  *n_full_out = n_full;
  *ksplits_out = ksplits;
}

// hidden splits of the feed-forward on a grid of `base` workgroups (tune.ff_split: 0 = automatic, 1 = off, 2 / 4 / 8 = forced)
inline int plan_ff_split(const gmf::Tuning& tune, int base, int max_parts) {
  int hs = 1;
  if (max_parts >= 2) {
    if (tune.ff_split > 0) hs = tune.ff_split;
    else if (base < 256) hs = base <= 32 ? 8 : base <= 64 ? 4 : 2;   // (measured at B = 1 .. 4: the merge reads every partial)
    hs = std::min(hs, max_parts);
    if (hs != 2 && hs != 4 && hs != 8) hs = 1;
  }
  return hs;
}

// How one encoder forward runs: every launch decision, made once (plan_encoder) from the handle's knobs, the weight images
// present and the shape, with the sizes of the buffers that depend on them.  The launchers are told; none reads the knobs.
struct EncoderPlan {
  enum Form {
    kFp32,          // fp32 images and kernels for every stage (split-fp16 weight images missing, "scattn_variant" 0, dense attention)
    kStages,        // split-fp16, one kernel per stage; the attention writes the block output
    kFusedStages,   // the cached, pipelined attention applies the next layer's PointCN in its epilogue; one kernel per other stage
    kLinear,        // ... and k_linear_h2 for Q'/K/V + Fusion-2: two launches per layer (the default)
    kSmall3,        // ... small grids: three launches per layer with two workgroup roles each
  };
  Form form = kFp32;
  bool fused() const { return form >= kFusedStages; }
  bool f1_h2 = false;        // Fusion-1 on split-fp16 images
  bool prologue = false;     // small grids: the prologue's two chains as roles of three shared launches (k_pro_*)
  bool cache = false;        // compat cache, built once per batch
  bool pipelined = false;    // attention: k_scattn_h2p streaming c from the cache (scattn_variant 18)
  int fmt = 0;               // the cache's element format (ForwardBuffers::fmt)
  bool half = false;         // throughput numerics (ForwardBuffers::half) ...
  bool one_product = false;  // ... and the linear stages multiply one product as well ("precision" = 2)
  bool front_split = false;  // k_front_h2 with one workgroup per output
  int max_splits = 0;        // capacity of the key- and hidden-split partials (0: no workspace for them)
  int attn_nf = 0, attn_ks = 1;   // attention items per XCD that run whole, key splits of the rest
  int ff_hs = 1, f1_ff_hs = 1;    // hidden splits of the layers' feed-forward and of Fusion-1's
  bool roles = false;        // k_linear_h2 as two workgroup roles per row block
  bool q_in_attn = false;    // no Q' image: the attention projects its own (LayerRun::qf_img)
  bool kv_fold = false;      // keys = values = f: no K / V projections, composed weights (gmf_encoder_weights::kv_fold)
  bool c16_guard = false;    // "compat_16": fmt = 2 for the pairs and layers the guard lets through, a lazily built fp32 cache for the rest
  bool v_fp8 = false;        // V carries e4m3 cross planes (ForwardBuffers::v_scale) ...
  bool guard = false;        // ... chosen per pair and layer on the device (PvGuard)
  bool clear_stats = false;  // the key-point packing clears the guard's statistics
  size_t act = 0, tok = 0, cache_floats = 0;   // floats of an activation image, a token image, the cache
  size_t cache_fb_floats = 0;                  // ... and of the guarded form's fp32 cache (c16_guard)
};

// min_tiles > 0: a ragged batch whose smallest pair has that many tiles.  dense: the caller passes the attention matrix.
inline EncoderPlan plan_encoder(const gmf::Tuning& t, const gmf_encoder_weights* w, int B, int N, int T, int L, int min_tiles, int cus,
                                bool dense = false) {
  EncoderPlan p;
  const int tiles = tiles_of(N), tt = tiles_of(T);
  const int W = ((tiles + 3) / 4) * B;     // workgroups of 128 query rows
  const bool ragged = min_tiles > 0;
  p.act = (size_t)B * tiles * kTileFloats;
  p.tok = (size_t)B * tt * kTileFloats;
  // split-fp16 path: needs every split-fp16 weight image; the dense-`attention` drop-in and scattn_variant 0 run on fp32 images
  const bool h2 = !dense && t.scattn_variant >= 9 && w->front_wst_h2 && w->ctx_wst_h2 && w->attn_wst_h2 && w->ff_wst_h2 && w->tail_wst_h2;
  const bool fusable = h2 && t.fused_linear && t.scattn_variant == 18;
  // throughput numerics ("precision" = 1, 2): on the two-launch path of large grids the attention multiplies one fp16 product and
  // streams the compat matrix as fp16 (level 2: the layer's linear stages multiply one product as well); every other path keeps the
  // parity numerics
  const bool half = t.precision >= 1 && fusable && W >= 256 && !ragged;
  // the cache's element format: fp16 c in the throughput mode; else the handle's "compat_format" wherever the pipelined kernel
  // (variant 18) is the cache's only reader.  4 KiB per pair of 32-row tiles as fp32, 2 KiB in the 16-bit formats
  const int fmt = half ? 1 : t.scattn_variant == 18 ? t.compat_format : 0;
  const size_t cache_floats = (size_t)B * tiles * tiles * (fmt ? 512 : 1024);
  const size_t cache_cap = (size_t)96 << 30;      // above it the cache is not used
  p.cache = h2 && L > 1 && t.use_cache && cache_floats * 4 <= cache_cap;
  const bool fused = fusable && p.cache;
  if (p.cache) { p.cache_floats = cache_floats; p.fmt = fmt; p.half = half; }
  p.one_product = p.half && t.precision == 2;
  p.pipelined = p.cache && t.scattn_variant == 18;
  p.front_split = t.front_split && W < 128;
  // partials of the key / hidden splits: small grids up to 8 splits of every query block, large grids 2..4 of the last partial round
  p.max_splits = (p.cache && tiles >= 8) ? (W < 384 ? 8 : 4) : 0;
  // ragged batch: planned on the SMALLEST pair's tiles (every pair then has at least four key tiles per split); either every item is
  // split - small grids: a handful of whole items walking all their keys alone left most of the chip idle (4 pairs x 1000: 1.50 ms
  // against 0.74 for the uniform batch) - or none is
  plan_attn_split(t, cus, W, ragged ? min_tiles : tiles, p.max_splits, ragged, &p.attn_nf, &p.attn_ks);
  p.ff_hs = plan_ff_split(t, W, p.max_splits);
  p.f1_ff_hs = tt <= tiles ? plan_ff_split(t, ((tt + 3) / 4) * B, p.max_splits) : 1;   // (into the attention's partials)
  if (!h2) p.form = EncoderPlan::kFp32;
  else if (!fused) p.form = EncoderPlan::kStages;
  // small grids: when both the attention and the feed-forward are split anyway, their workgroups share launches
  else if (W < 256 && t.small_roles && p.attn_nf == 0 && p.attn_ks > 1 && p.ff_hs > 1 && p.max_splits == 8) p.form = EncoderPlan::kSmall3;
  // below 256 row blocks key / hidden / output splits fill the chip better; a ragged batch takes either the three-launch form of
  // small grids or the two-launch form (the one-kernel-per-stage form in between has no pair table)
  else p.form = (W >= 256 || ragged) ? EncoderPlan::kLinear : EncoderPlan::kFusedStages;
  // grids that give a CU about one workgroup: k_linear_h2 as two roles per row block (the Q'/K/V projections | Fusion-2) in one launch
  p.roles = p.form == EncoderPlan::kLinear && t.mid_grid_roles > 0 && W < t.mid_grid_roles;
  // [r4] Q' in the attention kernel's prologue (parity arithmetic of the pipelined kernel; not with the linear kernel as two roles,
  // whose Q'/K/V role writes the image): k_linear_h2 then projects K and V only
  p.q_in_attn = p.form == EncoderPlan::kLinear && t.q_in_attention && !p.half && !p.roles;
  p.f1_h2 = h2 && w->f1_ctx_wst_h2 && w->f1_attn_wst_h2 && w->f1_ff_wst_h2;
  const bool pro_grid = t.small_prologue && fused && p.f1_h2 && W < 256;    // grids whose prologue runs as roles (below; fp32 cache only)
  // "compat_16" (the default): on the two-launch plan with the parity numerics of the pipelined kernel the cache format
  // follows the fp8 decision - uniform or ragged, the linear kernel whole or as two roles, Q' in the attention prologue or as an image,
  // folded or not.  "pv_fp8" = 1 with thresholds: 16 bits where the guard lets a pair's layer through, and a second, fp32 cache that the
  // device fills for the pairs that trip (c16_guard); "pv_fp8" = 2: 16 bits for everyone, as the fp8 products; three products ("pv_fp8"
  // = 0, pv_guard = NULL) keep fp32.  The size cap counts both caches; beyond it the plan is the fp32 one.  Everything else - small
  // grids, "precision" 1 / 2 - keeps what it has: the default asks for 256 row blocks, as the two-launch plan of uniform batches does
  // (a smaller ragged batch on that plan keeps the fp32 cache and the role prologue, whatever its knobs say); "compat_16" = 2 takes
  // every grid of the two-launch plan, with the prologue as kernels of its own (what the tests of small shapes use)
  if ((t.compat_16 == 2 || (t.compat_16 == 1 && W >= 256)) && p.form == EncoderPlan::kLinear && p.pipelined && !p.half && p.fmt == 0 &&
      (t.pv_fp8 == 2 || (t.pv_fp8 == 1 && w->pv_guard))) {
    const size_t fb = t.pv_fp8 == 1 ? cache_floats : 0;
    if ((cache_floats / 2 + fb) * 4 <= cache_cap) {
      p.fmt = 2;
      p.cache_floats = cache_floats / 2;
      p.cache_fb_floats = fb;
      p.c16_guard = fb != 0;
    }
  }
  // "kv_fold": the two-launch plan with the parity numerics of the pipelined kernel - uniform or ragged, the linear kernel whole or as
  // two roles, Q' in the attention prologue or as an image, either cache format (one rule for all of them: the forms that are compared
  // bit for bit fold together).  Everything else - small grids, "precision" 1 / 2, weights without the composed block - runs the
  // unfolded form
  p.kv_fold = t.kv_fold && p.form == EncoderPlan::kLinear && p.pipelined && !p.half && w->kv_fold != nullptr;
  // parity arithmetic: V with e4m3 cross planes for the pv_fp8 form of every attention kernel of the fused forms (a weights block
  // without thresholds, pv_guard = NULL, gets the three-product form under the guarded default, never the unguarded one).  [r5]
  // "pv_fp8" = 1: guarded per pair and layer on the device; the key-point packing clears the statistics (a superset of the readers)
  p.v_fp8 = fused && !p.half && (t.pv_fp8 == 2 || (t.pv_fp8 == 1 && w->pv_guard));
  p.clear_stats = fused && t.pv_fp8 == 1 && w->pv_guard;
  p.guard = p.clear_stats && !p.half;
  // [r5] small grids: the prologue is two independent chains of few-workgroup kernels - image side (Fusion-1 context, cross-attention,
  // feed-forward) and point side (key points, compat cache, layer 0 + first PointCN).  Three launches carry one link of each
  // (k_pro_*, encoder_h2.hip): the point side runs under the image side instead of behind it.  Same bodies: bit-identical.
  p.prologue = pro_grid && p.fmt == 0;
  return p;
}
