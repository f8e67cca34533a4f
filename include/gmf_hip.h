/* gmf_hip.h - C ABI of libgmf_hip.so: the MI355X (gfx950) implementation of GMF's
 * multimodal-fusion hot path.
 *
 * The reference (XiaoshuiHuang/GMF) has NO native plugin ABI: the path sits behind Python
 * nn.Module.forward calls.  This header is therefore the boundary a binding
 * would target; each entry point names the reference interface it replaces (file:line relative to
 * the reference tree).  The Python drop-in modules in gmf_amd/ bind it with ctypes
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - plain C types only; every data pointer is a DEVICE pointer owned by the caller
 *     (e.g. torch.Tensor.data_ptr()); the library never frees caller memory;
 *   - every call is asynchronous on the caller's stream (gmf_stream_t = hipStream_t passed as
 *     void*; NULL = the default stream) and performs no host synchronisation;
 *   - return value: 0 = GMF_OK, negative = error (see enum); gmf_last_error_string(h) has details;
 *     no exception or abort ever crosses this boundary;
 *   - a handle is bound to one device; distinct handles are independent.  Calls on ONE handle are serialised by an
 *     internal lock and every call reuses the handle's workspace, so a handle serves one logical stream of work: a call on a
 *     different stream than the previous call first waits (on the device) for the previous stream's work; the caller's
 *     current device is restored on return;
 *   - all tensors are fp32.  "P32 image" / "T image" are the tiled layouts described in
 *     gmf_amd/csrc/mfma_core.hpp; gmf_pack_rows_p32 / gmf_unpack_rows_p32 convert from and to
 *     arbitrary strided [B, rows, K] views (row-major [B,N,C] or channel-major [B,C,N]).
 */
#ifndef GMF_HIP_H_
#define GMF_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gmf_handle gmf_handle;
typedef void* gmf_stream_t;

enum {
  GMF_OK = 0,
  GMF_ERR_BAD_ARG = -1,
  GMF_ERR_UNSUPPORTED_SHAPE = -2,
  GMF_ERR_HIP = -3,
  GMF_ERR_NO_DEVICE = -4,
  GMF_ERR_OOM = -5,
  GMF_ERR_WORKSPACE = -6   /* the caller-provided workspace (gmf_set_workspace) is too small for this call */
};

#define GMF_ABI_VERSION 5   /* 5: gmf_encoder_weights gained `pv_guard` (a caller that fills the struct itself must be rebuilt; one that uses
                             * gmf_encoder_pack_weights keeps working); "pv_fp8" takes 0 / 1 / 2.  gmf_icp_point_to_point_ex and
                             * gmf_ransac_feature_matching, then gmf_spectral_matching, then gmf_max_clique and gmf_pmc_graph, then gmf_tsdf_allocate, gmf_tsdf_integrate and gmf_tsdf_extract, then gmf_rgbd_pyramids, gmf_rgbd_correspondences and
                             * gmf_rgbd_odometry, then gmf_tsdf_integrate_color and gmf_tsdf_extract_color, then gmf_icp_point_to_plane, then gmf_tsdf_extract_mesh, then gmf_color_gradients,
                             * gmf_icp_colored and gmf_voxel_down_sample_color joined under 5: added entry points, no existing signature or struct changed.  4: + gmf_get_tuning; the
                             * pose head / pick_seeds take any N */

/* ---- lifetime ------------------------------------------------------------------------------ */
int gmf_abi_version(void);
/* Creates a handle on HIP device `device` (fails with GMF_ERR_NO_DEVICE if there is none). */
int gmf_create(int device, gmf_handle** out);
void gmf_destroy(gmf_handle* h);
const char* gmf_last_error_string(gmf_handle* h);
/* Bytes of device workspace currently held by the handle (library-owned or caller-provided). */
long long gmf_workspace_bytes(gmf_handle* h);
/* Workspace ownership.  By default the library owns ONE device block per handle (hipMalloc, grown with a device
 * synchronisation when a larger shape arrives - never grow it inside a stream capture).  gmf_set_workspace hands the
 * library a caller-owned device block instead (e.g. a torch tensor: the memory then belongs to the caller's allocator, and
 * the library frees its own block); a call that needs more than `bytes` returns GMF_ERR_WORKSPACE without launching anything
 * and gmf_workspace_wanted() returns the size that call asked for (with headroom): allocate, set, call again.
 * gmf_set_workspace(h, NULL, 0) returns to the library-owned block.  The block must stay valid until the work of the last
 * call that used it has completed on its stream.  (The reference has no counterpart: its intermediates are torch tensors.) */
int gmf_set_workspace(gmf_handle* h, void* device_ptr, long long bytes);
long long gmf_workspace_wanted(gmf_handle* h);

/* Sticky status word of the handle, kept in host-mapped memory: kernels OR bits into it, the host reads it WITHOUT any
 * device synchronisation (after the caller's own stream / device synchronisation it reflects every finished call).
 *   GMF_STATUS_NONFINITE: an inlier logit, a feature norm (gmf_encoder_forward / gmf_classifier_forward) or an output
 *   element of gmf_fusion_layer_forward was NaN or infinite.  The split-fp16 MFMA operands hold |x| < 65504 (weights are
 *   checked when they are packed; activations cannot be): an activation beyond that range turns into inf / NaN and ends up
 *   here instead of passing silently.  The reference (fp32 throughout) has no such limit.
 * *flags receives the word; clear != 0 resets it. */
#define GMF_STATUS_NONFINITE 1
/* [ABI 5] informational, not an error: under "pv_fp8" = 1 the device-side guard sent at least one (pair, layer) of a finished
 * gmf_encoder_forward(_ragged) to the three-product form of P V (the network's attention scores can exceed the bound of
 * gmf_encoder_weights::pv_guard there).  The results are as valid as any; the bit says why a step took ~3 % longer. */
#define GMF_STATUS_PV_GUARDED 2
/* gmf_sparse_build_plan met a duplicate (batch, coordinates) input row: rows must be unique, they are never merged; the
 * plan and everything computed from it are not valid. */
#define GMF_STATUS_SPARSE_DUPLICATE 4
/* gmf_batchnorm_masked_forward met a level with fewer than 2 valid rows (torch's BatchNorm raises there): its outputs and
 * batch statistics are not valid and the running statistics were left unchanged. */
#define GMF_STATUS_BATCHNORM_ROWS 8
/* gmf_posegraph_optimize met a pivot of H + lambda I that was not finite or not positive (stop code 6 of that graph and pass) */
#define GMF_STATUS_POSEGRAPH_PIVOT 16
/* gmf_hardest_contrastive_forward met a row index outside its tensor (positive_pairs, pos_sel, sel0 or sel1): that index was
 * read as 0 and the loss is not valid. */
#define GMF_STATUS_LOSS_INDEX 32
int gmf_status_read(gmf_handle* h, int* flags, int clear);

/* [ABI 5] PointDSC's learnable scalar `sigma` (PointDSC.py:164) from DEVICE memory.  While `sigma_dev` is non-NULL every entry point
 * that takes sigma by value - gmf_similarity_matrix, gmf_similarity_backward, gmf_spectral_matching_loss_fused / _backward and, through
 * gmf_pose_params::sigma, gmf_pose_head(_ragged) / gmf_pose_head_backward - ignores that value and its kernels read the float at this
 * address when they run (the same correctly rounded 1 / sigma^2 as the host forms: identical bits).  What it is for: a training step
 * whose optimizer updates sigma on the device can be captured in a HIP graph and replayed without the one host read per step the
 * by-value form needs (libs/trainer.py:131-166; gmf_amd.train.GraphedTrainingStep).  NULL (default) restores the by-value form.  The
 * address must stay valid while set. */
int gmf_set_sigma_device(gmf_handle* h, const float* sigma_dev);

/* Per-handle tuning knobs (state lives in the handle; no process globals, no environment variables).  Every setting
 * except "precision" computes the same result up to rounding - there is no timing-only or wrong-result mode in the
 * library; unknown names and out-of-range values are rejected with GMF_ERR_BAD_ARG.
 *   "precision"         : 0 = parity numerics (default): every contraction is fp32-equivalent (split-fp16 operands, three
 *                         partial products, fp32 accumulation), logits and poses within 1e-4 of the reference.
 *                         1 = throughput numerics (the reduced-precision variant of SURVEY.md section 7 step 8): on large
 *                         grids (>= 256 attention workgroups) the spatial-consistency attention multiplies plain fp16
 *                         operands (ONE product, fp32 accumulation) and streams the compat matrix as fp16; softmax
 *                         statistics, LayerNorm, GELU, the linear stages and the pose head are unchanged.  NOT within the
 *                         1e-4 gate: measured against the parity mode at 32 x 5000: max |d logit| 1.6e-4, identical inlier
 *                         labels, 1.46x the throughput (1.50x at 16 x 10000).
 *                         2 = level 1, and the layer's linear stages (Q'/K/V projections, Fusion-2 cross-attention and
 *                         feed-forward; grids of >= 512 base workgroups) multiply only the high fp16 planes of weights and
 *                         activations too: max |d logit| 4e-2 (mean 2e-3), 99.9 % identical logit signs, 98-100 % identical
 *                         final labels, 1.6x the throughput.
 *   "scattn_variant"    : 18 = split-fp16 MFMA attention (2 planes, 3 products), compat matrix streamed from the per-batch
 *                         cache, tile loop software-pipelined inside each wave (default); 9 = the same arithmetic without
 *                         the pipelining; 0 = every encoder stage on the fp32 MFMA with fp32 images.
 *   "compat_cache"      : 1 = build the compat matrix once per batch (default), 0 = recompute c_ij in the attention kernel
 *                         (what the library does by itself when the cache would exceed 96 GB); 0 implies the
 *                         non-pipelined kernel.
 *   "compat_format"     : element format of the compat cache on the pipelined path: 0 = the plan's choice ("compat_16"; default); 2 =
 *                         16-bit fixed point rint(65535 c) UNCONDITIONALLY - half the cache, half its stream, |dc| <= 7.6e-6.  Opt-in:
 *                         measured inside the 1e-4 gate on 3DMatch-shape inputs, but 4-8x the reference's own fp32 noise on
 *                         ill-conditioned KITTI-shape inputs (profiles/r03_compat_formats.txt).
 *   "compat_16"         : 1 = on the two-launch plan of large grids (parity numerics) the compat cache is 16-bit fixed point under the
 *                         "pv_fp8" guard (default): per pair and layer the attention streams 16 bits where the guard lets the fp8
 *                         products through, and an exact fp32 cache - built on the device for the pairs that trip, once per forward -
 *                         where it does not ("pv_fp8" = 2: 16 bits for everyone; "pv_fp8" = 0 or pv_guard = NULL: fp32).  The
 *                         workspace holds both caches.  1 applies to grids of 256 row blocks and more, 2 to every grid of the
 *                         two-launch plan; 0 = the fp32 cache for everyone: the earlier results, bit for bit.
 *   "pv_fp8"            : parity arithmetic of the default path (scattn_variant 18, fused_linear 1): the two CROSS products of the
 *                         attention's O += P V (P_hi V_lo + P_lo V_hi) on the block-scaled fp8 matrix pipe - one
 *                         v_mfma_scale_f32_32x32x64_f8f6f4 per feature block and key tile, e4m3 operands, one scale per (feature,
 *                         tile), the softmax row sum taken over exactly the probabilities the pipe multiplies - and likewise the two
 *                         cross products of S = K Q'^T (one scale per (key, 32 channels) and per (query, 32 channels)); only
 *                         P_hi V_hi and K_hi Q'_hi stay on the f16 pipe.  With "kv_fold" the two high planes are the same numbers
 *                         and are stored once.  1 (default) = GUARDED [ABI 5]: per pair and layer, on the
 *                         device, from the largest row norm of the layer's input features against gmf_encoder_weights::pv_guard
 *                         (a bound on the attention scores the layer can form): layers whose softmax can collapse onto single keys
 *                         - where the e4m3 rounding of one key's V reaches the output whole - take the three-product form, every
 *                         other layer the fp8 form.  No host synchronisation, no dependence on the other pairs of the batch.
 *                         2 = the fp8 form unconditionally, 0 = all three products of P V on the f16 pipe (the strict form).
 *                         Logits of the two forms differ by <= 3e-5 (mean 2e-6) at 32 x 5000 (profiles/r03_pv_fp8.txt).
 *   "attn_tail_split"   : 1 = large grids: the last partial round of attention workgroups is split by keys, 0 = whole (default).
 *   "small_grid_roles"  : 1 = small grids run three launches per layer with mixed workgroup roles (default), 0 = one per stage.
 *   "attn_key_splits"   : 0 = automatic (small grids only), 1 = off, 2..8 = forced number of key splits.
 *   "ff_hidden_splits"  : 0 = automatic (small grids only), 1 = off, 2 / 4 / 8 = forced.
 *   "front_output_split": 1 = small grids use one workgroup per output of the front kernel (default), 0 = never.
 *   "fused_linear"      : 1 = one kernel per layer for Q'/K/V + Fusion-2 (default), 0 = the three-kernel sequence.
 *   "wide_attn_tile"    : 1 = the cross-attention of the (256, 128) FusionLayer runs one workgroup per 32-row tile on grids of up
 *                         to 256 tiles, its waves splitting the feature blocks and the context tiles (default), 0 = one
 *                         workgroup per four tiles.
 *   "small_merge_tile"  : 1 = the merge step of the small-grid layer runs one workgroup per query tile whose four waves split
 *                         the feature blocks (default; bit-identical results), 0 = one workgroup per four tiles.
 *   "mid_grid_roles"    : W (default 512): on grids of 256 .. W - 1 base workgroups that kernel runs as two workgroup roles per
 *                         row block (Q'/K/V | Fusion-2; bit-identical results); 0 = never.
 *   "conv_lds_patch"    : 1 = stride-1 3x3 convolutions stage activations through LDS (default), 2 = same without the
 *                         three-workgroup form, 0 = gather form.
 *   "small_fattn_tile"  : [ABI 5] 1 = on small grids (B = 1, the reference's evaluation mode) the cross-attention role of a layer's first
 *                         launch runs one workgroup per query tile whose four waves deal the context tiles among themselves (default;
 *                         fusion_layer.py:84-94), 0 = one workgroup per four query tiles, each wave walking all context tiles.
 *                         Same products, another order of the softmax's partial sums.
 *   "conv_small_grid"   : [ABI 5] 1 = grids of fewer than 128 workgroups of those kernels - a few images, e.g. the two of one scene pair - run
 *                         the K-split kernel: 32 pixels x 32 channels per workgroup, its four waves a quarter of the k range each
 *                         (default), and the stem kernel 4 x 4 instead of 8 x 8 pooled pixels per workgroup (bit-identical);
 *                         0 = the 128-pixel kernels at every size.  Same products, another accumulation order.
 *   "small_prologue_roles": [ABI 5] 1 = on small grids the forward's prologue - two independent chains of few-workgroup kernels, image
 *                         side (Fusion-1 context / cross-attention / feed-forward, fusion_layer.py:172-201) and point side (key points,
 *                         compat cache PointDSC.py:216-221, layer 0 + first PointCN) - runs as three launches that carry one link of
 *                         each chain as two workgroup roles (default; the kernels' own bodies: bit-identical results), 0 = six kernels.
 *   "nms_binned"        : 1 = grid-binned NMS candidates on large grids (default), 2 = always, 0 = all pairs.
 *   "topk_select"       : 1 = radix select of the S seeds (default), 0 = full bitonic sort.
 *   "q_in_attention"    : [ABI 4] 1 = on large grids every attention workgroup projects its own Q' in its prologue (default; PointDSC.py:56),
 *                         0 = the linear kernel writes a Q' image.  Bit-identical results.
 *   "kv_fold"           : 1 = on the two-launch plan of large grids (parity numerics, either compat cache format) the attention's key and value
 *                         tiles are the layer input f itself: projection_k is composed into the query side, projection_v into
 *                         fc_message's first layer (gmf_encoder_weights::kv_fold; PointDSC.py:56-64; default).  Same guard rule as
 *                         "pv_fp8".  0 = the K and V projections are computed: the unfolded code, bit for bit.  The staged entry
 *                         points never fold.  Rounding-equivalent (logits within 4e-5 of the unfolded form, inside the parity gate).
 *   "spectral_col_splits": gmf_spectral_matching: 0 = the columns of a pair's sweep are split over workgroups by a rule of its own
 *                         N (default), 1..32 = that many splits at most (another order of a row's partial sums).
 *   "clique_local_rows" : gmf_max_clique: a root of the search with at most this many candidates is searched in LDS with
 *                         one candidate set per level; wider roots keep no sets and read the bit matrix.  0..384, default 384.
 *                         Both have the same search tree and return the same clique. */
int gmf_set_tuning(gmf_handle* h, const char* name, int value);
/* [ABI 4] The current value of a knob, so that a caller that changes one for a single call can put back what it found
 * (the Python PointDSC module does this for its module-local numerics mode).  Both calls take the handle's lock. */
int gmf_get_tuning(gmf_handle* h, const char* name, int* value);

/* In-situ timing of the dominant kernel (the spatial-consistency attention): while enabled, every
 * k_scattn launch made through gmf_encoder_forward / gmf_nonlocal_block_forward is bracketed by HIP events
 * recorded on the caller's stream.  gmf_profile_read synchronises those events (host sync - call it outside
 * timed regions), returns their summed duration and count, and resets the list.  Used by bench.py. */
int gmf_profile_enable(gmf_handle* h, int on);
int gmf_profile_read(gmf_handle* h, double* scattn_ms_total, int* scattn_launches);

/* ---- layout conversion ----------------------------------------------------------------------
 * src element (b, r, k) lives at src[b*sb + r*sr + k*sk]; dst is the P32 image
 * [B, ceil(n_rows/32), 32*K] (rows >= n_rows are zero).  K must be a multiple of 8.
 * Replaces the .permute()/.view() glue around the reference modules (PointDSC.py:70,130-135,223). */
int gmf_pack_rows_p32(gmf_handle* h, const float* src, long long sb, long long sr, long long sk, int B, int n_rows,
                      int K, float* dst, gmf_stream_t stream);
int gmf_unpack_rows_p32(gmf_handle* h, const float* src_img, int B, int n_rows, int K, float* dst, long long sb,
                        long long sr, long long sk, gmf_stream_t stream);
/* src_keypts, tgt_keypts [B,N,3] -> pts8 [B, Npad, 8] = (sx,sy,sz,0,tx,ty,tz,0). */
int gmf_pack_pts8(gmf_handle* h, const float* src, const float* tgt, int B, int N, float* dst, gmf_stream_t stream);

/* ---- encoder stages (operate on images; weights are packed blobs, layouts in gmf_amd/packing.py) */
/* Images of a stage hold Npad = 32 ceil(N/32) rows per pair, [B, Npad/32 tiles, 32*128] floats:
 *   P32 image of X[rows, K]: float (((b*tiles + tile)*(K/8) + g)*64 + lane)*4 + e = X[b][32 tile + i][8 g + 4 h + e];
 *   T   image of V[rows, D]: float ((((b*tiles + tile)*(D/32) + db)*4 + q)*64 + lane)*4 + e = V[b][32 tile + 8 q + 4 h + e][32 db + i];
 *   lane = 32 h + i, e = 0..3 (gmf_amd/packing.py: rows_p32 / timg and their inverses).
 * Padding rows (>= N): every stage writes them (finite whenever its inputs' padding rows are finite), and an input's padding rows
 * reach only the same padding rows of the outputs - except V, whose padding rows are multiplied by P = 0 for every query:
 * they must be finite (NaN * 0 = NaN).  A chain that starts from gmf_pack_rows_p32 (zero padding) keeps this by itself.
 * layer0 (if first) + PointCN_i + projection_{q,k,v} of NonLocalBlock i.
 * Replaces GMF_PointDSC/models/PointDSC.py:88,104-109 (NonLocalNet) and :56-58 (NonLocalBlock).
 * in: corr_pos [B,N,6] row-major if first, else feat P32 image.  Outputs f, q, k: P32 images; v: T image (D = 128).
 * q = (Wq f + bq) log2(e)/sqrt(128) (the softmax scale folded in, gmf_scattn_forward takes exp2). */
int gmf_front_forward(gmf_handle* h, int first, const float* in, const float* wst, const float* vecs, float* f,
                      float* q, float* k, float* v, int B, int N, gmf_stream_t stream);
/* Spatial-consistency self-attention + fc_message + (message + fusion2_out).
 * Replaces PointDSC.py:216-221 (compat matrix, recomputed in-kernel from pts8, never stored),
 * :60-65 and :73. */
int gmf_scattn_forward(gmf_handle* h, const float* q, const float* k, const float* v, const float* pts8,
                       const float* fusion2_out, const float* wst, const float* vecs, float* out, int B, int N,
                       float sigma_d, gmf_stream_t stream);
/* Same, but with the caller's dense compatibility matrix `attention` [B,N,N] (row-major) as
 * NonLocalBlock.forward receives it (PointDSC.py:40-45,62) instead of recomputing it from key points. */
int gmf_scattn_forward_dense(gmf_handle* h, const float* q, const float* k, const float* v, const float* attention,
                             const float* fusion2_out, const float* wst, const float* vecs, float* out, int B, int N,
                             gmf_stream_t stream);
/* Context side of FusionLayer: [LCPE] + LayerNorm_context + to_kv, for `sets` weight sets at once.
 * Replaces GMF_PointDSC/models/fusion_layer.py:124-126,46-49,86-87 (DGR twin: model/perceiver_io.py:126-128,89-91).
 * ctx: P32 image [B, Tt, 32*128], Tt = ceil(T/32); out: [sets, B, Tt, 4096]: per 32-token tile the first 2048 floats are Kc
 * [32, 64] as a P32 image (K = 64), the next 2048 Vc [32, 64] as a T image (D = 64) (packing.py ctx_image / split_ctx_image).
 * Set s reads wst + s*wst_stride, vecs + s*vec_stride and writes out + s*B*Tt*4096. */
int gmf_fusion_ctx_prepare(gmf_handle* h, int pe, const float* ctx, const float* wst, const float* vecs, float* out,
                           int B, int T, int sets, int wst_stride, int vec_stride, gmf_stream_t stream);
/* Query side up to the first residual: [LCPE] + LayerNorm + to_q + softmax(QK^T)V + to_out + x.
 * Replaces fusion_layer.py:119-121,44,84-94,190. */
int gmf_fusion_attn_forward(gmf_handle* h, int pe, const float* x, const float* ctx_img, const float* wst,
                            const float* vecs, float* x1, int B, int N, int T, gmf_stream_t stream);
/* LayerNorm + Linear(128,1024) + GEGLU + Linear(512,128) + residual.  Replaces fusion_layer.py:54-69,191. */
int gmf_fusion_ff_forward(gmf_handle* h, const float* x1, const float* wst, const float* vecs, float* x2, int B,
                          int N, gmf_stream_t stream);
/* classification head + F.normalize.  Replaces PointDSC.py:175-181,229,241.
 * Outputs are row-major: logits [B,N], feat_n [B,N,128], feat [B,N,128] (feat may be NULL).  A valid row whose features are
 * not finite sets GMF_STATUS_NONFINITE and gets zeros in feat_n; its logit is not meaningful (the head's ReLUs map NaN to 0,
 * so it may be finite).  Rows >= N of feat_img affect nothing. */
int gmf_classifier_forward(gmf_handle* h, const float* feat_img, const float* wst, const float* vecs, float* logits,
                           float* feat_n, float* feat, int B, int N, gmf_stream_t stream);

/* ---- whole encoder ---------------------------------------------------------------------------
 * Packed weights of PointDSC's NonLocalNet (minus the ResNet image encoder, which is upstream of the
 * hot path) + classifier.  All pointers are device pointers; *_stride are in floats between layers. */
typedef struct gmf_encoder_weights {
  int num_layers;
  const float* f1_ctx_wst;  const float* f1_ctx_vec;      /* Fusion-1 context side (pe = 0)  */
  const float* f1_attn_wst; const float* f1_attn_vec;     /* Fusion-1 query side             */
  const float* f1_ff_wst;   const float* f1_ff_vec;
  const float* ctx_wst;     const float* ctx_vec;   int ctx_wst_stride,   ctx_vec_stride;   /* Fusion-2, per layer */
  const float* attn_wst;    const float* attn_vec;  int attn_wst_stride,  attn_vec_stride;
  const float* ff_wst;      const float* ff_vec;    int ff_wst_stride,    ff_vec_stride;
  const float* front_wst;   const float* front_vec; int front_wst_stride, front_vec_stride;
  const float* tail_wst;    const float* tail_vec;  int tail_wst_stride,  tail_vec_stride;  /* fc_message */
  const float* head_wst;    const float* head_vec;
  float sigma_d;
  /* optional split-fp16 (fp16x2) images of every dense weight of the linear stages, same sizes and strides as the
   * fp32 blobs.  When all are non-NULL (tail_wst_h2 included) and the attention variant is 9 / 18 (the default),
   * [layer0]+PointCN+QKV, the context prepare, the cross-attention, the feed-forward and the attention run on the f16
   * MFMA with split-fp16 operands (fp32-equivalent accuracy); otherwise every stage runs on the fp32 MFMA. */
  const float* front_wst_h2; const float* ctx_wst_h2; const float* attn_wst_h2; const float* ff_wst_h2;
  const float* f1_ctx_wst_h2; const float* f1_attn_wst_h2; const float* f1_ff_wst_h2;
  /* optional split-fp16 image of the fc_message weights (same size and stride as tail_wst): the epilogue of the cached,
   * software-pipelined attention kernel then runs on the f16 MFMA too. */
  const float* tail_wst_h2;
  /* [ABI 5] optional, [num_layers]: the "pv_fp8" guard.  Entry l is the largest SQUARED row norm of layer l's input features
   * f = ReLU(PointCN_l(.)) up to which that layer's attention may run its P V cross products on the fp8 pipe (written by
   * gmf_encoder_pack_weights from the spectral norms of projection_q / projection_k, PointDSC.py:23-25,56-64); NULL = no thresholds:
   * the guarded default ("pv_fp8" = 1) then runs the three-product form (as "pv_fp8" = 0), never the unguarded one. */
  const float* pv_guard;
  /* optional (appended; NULL in a zero-initialised struct), per layer GMF_KV_FOLD_STRIDE floats: the weights of the "kv_fold" form of the
   * large-grid attention (keys = values = the layer input f; written by gmf_encoder_pack_weights, composed in fp64 and rounded once) -
   *   4 split-fp16 stages of Wk^T Wq' | 5 stages of fc_message with its first layer composed with projection_v (Wa Wv | Wb | Wc) |
   *   Wk^T bq' [128] | Wq'^T bk [128] | bk . bq' [1, padded to 128] | Wa bv + ba [64] | bb [64] | bc [128].
   * NULL (or a composed weight outside the fp16 range): every plan runs the unfolded form. */
  const float* kv_fold;
} gmf_encoder_weights;
#define GMF_KV_FOLD_STRIDE 37504

/* ---- weight packing ---------------------------------------------------------------------------
 * The reference keeps its weights as a PyTorch state_dict (588 non-image tensors under the names of SURVEY.md section 8b) and
 * has no packed form; the kernels stream blobs (P32 images, BatchNorm folded, softmax scales folded, split-fp16 planes).
 * These entry points build the blobs from the state_dict tensors themselves, so that a host in any language can go from a
 * checkpoint to gmf_encoder_forward: list the tensors by their reference names, pack once, run.
 * Tensors are contiguous fp32; shapes as torch stores them (conv1x1 weights [out, in, 1], depthwise taps [C, 1, 3]). */
typedef struct gmf_tensor {
  const char* name;          /* state_dict key, e.g. "encoder.blocks.NonLocal_layer_3.projection_q.weight" */
  const float* data;         /* host pointer (default) or device pointer (GMF_PACK_DEVICE_TENSORS) */
  int ndim;                  /* 0 .. 4 */
  long long shape[4];
} gmf_tensor;
#define GMF_PACK_DEVICE_TENSORS 1     /* `data` pointers are device pointers (copied to the host first) */
#define GMF_PACK_STANDALONE_BLOCK 2   /* NonLocalBlock on its own (PointDSC.py:40-74): no PointCN in front (identity) */
#define GMF_PACK_HOST_BLOCK 4         /* [ABI 4] keep the packed block in host memory although h is given (errors then still land in
                                       * gmf_last_error_string(h)); gmf_packed_*_place moves it to caller-owned device memory */
typedef struct gmf_packed_encoder gmf_packed_encoder;
/* Packs NonLocalNet (Fusion-1 if present, layer0, num_layers x {PointCN, NonLocalBlock with its Fusion-2}) + classifier
 * (PointDSC.py:77-181) into ONE library-owned device block on h's device and fills a gmf_encoder_weights that points into it.
 * Tensors the list does not need are ignored (the image encoder, num_batches_tracked); a missing one is GMF_ERR_BAD_ARG with
 * its name in gmf_last_error_string.  h may be NULL: the blobs then stay in host memory (inspection / tests; not for kernels).
 * A weight outside the fp16 range of the split operands (|256 w| > 65504, e.g. a BatchNorm with a tiny running_var) leaves the
 * *_h2 pointers NULL: every stage then runs on the fp32 MFMA; gmf_packed_encoder_info reports it. */
int gmf_encoder_pack_weights(gmf_handle* h, const gmf_tensor* tensors, int n_tensors, int num_layers, int flags,
                             gmf_packed_encoder** out);
const struct gmf_encoder_weights* gmf_packed_encoder_weights(const gmf_packed_encoder* p);
/* sigma (PointDSC.py:164, for gmf_pose_params), sigma_d (= sigma_spat, :165), whether the split-fp16 images were built, and
 * the largest |value| met while splitting (inf: a weight was not finite).  Any output pointer may be NULL. */
int gmf_packed_encoder_info(const gmf_packed_encoder* p, float* sigma, float* sigma_d, int* split_fp16, float* max_abs_scaled);
void gmf_packed_encoder_free(gmf_packed_encoder* p);
/* [ABI 4] The packed block in CALLER-OWNED device memory (a host that has its own allocator - PyTorch's caching allocator,
 * an arena - should not get a hipMalloc per pack and a device-wide hipFree per release).  Pack with h = NULL (the blobs stay in host
 * memory), ask for the size, then place: the block is copied to `device_dst` (256-byte aligned, >= gmf_packed_encoder_bytes, on h's
 * device) asynchronously on `stream`, and the object's gmf_encoder_weights is re-based to point into it.  The library never frees
 * `device_dst`; it must outlive every call that uses the weights.  May be called again to move the weights. */
long long gmf_packed_encoder_bytes(const gmf_packed_encoder* p);
int gmf_packed_encoder_place(gmf_handle* h, gmf_packed_encoder* p, void* device_dst, long long bytes, gmf_stream_t stream);

/* One FusionLayer / PerceiverIO with depth = 0 (fusion_layer.py:131-201, perceiver_io.py:139-221; widths (128, 64) and
 * (256, 128)): the arguments of gmf_fusion_layer_forward.  `prefix` is prepended to the module's own key names
 * ("cross_attend_blocks.0.fn.to_q.weight", "cpe.proj_q.weight", ...); pe = whether the layer has a `cpe`. */
typedef struct gmf_fusion_weights {
  int latent_dim, d_head, pe, split_fp16;
  float max_abs_scaled;
  const float *ctx_wst, *ctx_vec, *attn_wst, *attn_vec, *ff_wst, *ff_vec;
  const float *ctx_wst_h2, *attn_wst_h2, *ff_wst_h2;      /* NULL when a weight is outside the fp16 range */
} gmf_fusion_weights;
typedef struct gmf_packed_fusion gmf_packed_fusion;
int gmf_fusion_pack_weights(gmf_handle* h, const gmf_tensor* tensors, int n_tensors, const char* prefix, int pe, int flags,
                            gmf_packed_fusion** out);
const gmf_fusion_weights* gmf_packed_fusion_weights(const gmf_packed_fusion* p);
void gmf_packed_fusion_free(gmf_packed_fusion* p);
long long gmf_packed_fusion_bytes(const gmf_packed_fusion* p);                          /* [ABI 4] as gmf_packed_encoder_bytes / _place */
int gmf_packed_fusion_place(gmf_handle* h, gmf_packed_fusion* p, void* device_dst, long long bytes, gmf_stream_t stream);

/* PointDSC.forward up to the logits (PointDSC.py:216-241) with image TOKENS as input:
 * corr_pos [B,N,6], src/tgt_keypts [B,N,3], p_tokens/q_tokens [B,T,128] (row-major)
 * -> logits [B,N], feat_n [B,N,128] (unit rows), feat [B,N,128] (may be NULL). */
int gmf_encoder_forward(gmf_handle* h, const gmf_encoder_weights* w, const float* corr_pos, const float* src_keypts,
                        const float* tgt_keypts, const float* p_tokens, const float* q_tokens, int B, int N, int T,
                        float* logits, float* feat_n, float* feat, gmf_stream_t stream);

/* The same for a RAGGED batch: B pairs, each with its OWN number of correspondences, in one launch.  The reference feeds its
 * evaluation loop one pair at a time, each with its own N (evaluation/test_3DMatch.py:24-119, PointDSC.py:279,504 assert
 * B == 1); its collate function clips a training batch to the smallest N (datasets/dataloader.py:6-23).  Here the row-major
 * tensors are PACKED: pair b owns rows [n_0 + .. + n_{b-1}, + n_b) of corr_pos [sum n, 6], src/tgt_keypts [sum n, 3], logits
 * [sum n], feat_n / feat [sum n, 128]; the tokens stay [B, T, 128].  n_points: HOST array [B] (the caller knows its tensor
 * shapes; the library sizes its grids from it).  The result equals B calls with B = 1, pair by pair, whatever the order of the pairs
 * (the library deals them to the chip's eight dies by work; small batches run the same small-grid kernels as uniform ones).  Default path only (split-
 * fp16 weight images, num_layers >= 2, "fused_linear" = 1, "scattn_variant" = 18): otherwise GMF_ERR_UNSUPPORTED_SHAPE. */
int gmf_encoder_forward_ragged(gmf_handle* h, const gmf_encoder_weights* w, const float* corr_pos, const float* src_keypts,
                               const float* tgt_keypts, const float* p_tokens, const float* q_tokens, const int* n_points, int B,
                               int T, float* logits, float* feat_n, float* feat, gmf_stream_t stream);

/* One NonLocalBlock on P32 images (PointDSC.py:40-74): feat_img -> out_img given the fused image tokens
 * (P32 image [B,Tt,..]) and EITHER pts8 (compat recomputed in-kernel) OR the dense `attention` [B,N,N]
 * (exactly one of the two non-NULL).  layer selects the weight set inside `w`. */
int gmf_nonlocal_block_forward(gmf_handle* h, const gmf_encoder_weights* w, int layer, int apply_pointcn,
                               const float* feat_img, const float* pts8, const float* attention,
                               const float* image_feat_img, float* out_img, int B, int N, int T, gmf_stream_t stream);

/* FusionLayer.forward / PerceiverIO.forward with depth=0 (fusion_layer.py:172-201; DGR twin
 * model/perceiver_io.py:187-221): data [B,T,128] (context, row-major), queries [B,N,latent_dim] (any strides)
 * -> out [B,N,latent_dim].  (latent_dim, d_head) = (128, 64) is GMF-PointDSC's Fusion-1/2 and DGR's
 * image_fusion (resunet_new.py:618-626); (256, 128) is the DGR bottleneck instance (resunet_new.py:516-525)
 * whose to_out maps the head back to the 256-wide query.  Weight blobs: gmf_amd/packing.py.
 * ff_wst_h2 (may be NULL): the feed-forward weights as split-fp16 images (packing.p32_h2, same size as ff_wst); when
 * given, the GEGLU feed-forward - 96 % of this layer's FLOPs - runs on the f16 MFMA with fp32-equivalent accuracy.
 * ctx_wst_h2 / attn_wst_h2 (both or neither): the context and attention weights as
 * split-fp16 images (packing.p32_h2s, same sizes) - context preparation and cross-attention on the f16 MFMA as well. */
int gmf_fusion_layer_forward(gmf_handle* h, int pe, int latent_dim, int d_head, const float* ctx_wst, const float* ctx_vec,
                             const float* attn_wst, const float* attn_vec, const float* ff_wst, const float* ff_vec,
                             const float* data, const float* queries, long long q_sb, long long q_sr, long long q_sk,
                             float* out, long long o_sb, long long o_sr, long long o_sk, int B, int N, int T,
                             gmf_stream_t stream, const float* ff_wst_h2, const float* ctx_wst_h2, const float* attn_wst_h2);

/* ---- pose head ------------------------------------------------------------------------------- */
typedef struct gmf_pose_params {
  int num_seeds;        /* S = int(N * ratio)                        PointDSC.py:244 */
  int k;                /* neighbours per seed (<= 64, <= N-1)        PointDSC.py:324 */
  int num_iterations;   /* power iterations                          PointDSC.py:437 */
  int use_nms;          /* 1: pick_seeds (test mode) ; 0: plain top-S (train mode)  PointDSC.py:243-246 */
  int refine_iters;     /* 20 in test mode, 0 to skip post_refinement PointDSC.py:256-257,505-508 */
  float sigma;          /* learned feature bandwidth                 PointDSC.py:164 */
  float sigma_d;        /* spatial bandwidth                         PointDSC.py:165 */
  float inlier_threshold;
  float nms_radius;
  float refine_threshold; /* 0.10 if inlier_threshold == 0.10 else 1.2 PointDSC.py:505-508 */
} gmf_pose_params;

/* seeds -> kNN -> seed compatibility + power iteration -> weighted Kabsch -> hypothesis scoring ->
 * argmax -> labels -> post refinement, per pair, all on device.
 * Replaces PointDSC.py:243-257 (pick_seeds :268-286, cal_seed_trans :303-427, cal_leading_eigenvector
 * :429-448, post_refinement :493-528) and models/common.py:10-75.
 * seeds_in may be NULL (seeds are computed from logits) or caller-provided [B,S].
 * Outputs: final_trans [B,16], final_labels [B,N], and optionally (may be NULL) seeds_out [B,S] int32,
 * knn_out [B,S,k] int32, seed_trans [B,S,16], fitness [B,S]. */
int gmf_pose_head(gmf_handle* h, const gmf_pose_params* p, const float* feat_n, const float* src_keypts,
                  const float* tgt_keypts, const float* logits, const int* seeds_in, int B, int N, float* final_trans,
                  float* final_labels, int* seeds_out, int* knn_out, float* seed_trans, float* fitness,
                  gmf_stream_t stream);

/* gmf_pose_head for a ragged batch (packing as gmf_encoder_forward_ragged; n_points: HOST array [B]): pair b uses
 * S_b = int(n_b * ratio) seeds (PointDSC.py:244; p->num_seeds is ignored) and is solved exactly as a B = 1 call - the power
 * iteration's allclose exit (PointDSC.py:444) is resolved per pair.  Every pair needs more than p->k correspondences.
 * final_trans [B,16]; final_labels [sum n]; the optional per-seed outputs are [B, S_max, ...] with S_max = max S_b, the slots
 * behind a pair's own seeds zero. */
int gmf_pose_head_ragged(gmf_handle* h, const gmf_pose_params* p, double ratio, const float* feat_n, const float* src_keypts,
                         const float* tgt_keypts, const float* logits, const int* n_points, int B, float* final_trans,
                         float* final_labels, int* seeds_out, int* knn_out, float* seed_trans, float* fitness,
                         gmf_stream_t stream);

/* pick_seeds / plain top-S only (PointDSC.py:268-286 / :246). */
int gmf_pick_seeds(gmf_handle* h, const float* src_keypts, const float* scores, int B, int N, float nms_radius,
                   int use_nms, int num_seeds, int* seeds_out, gmf_stream_t stream);

/* knn(x, k, ignore_self=True, normalized=True) restricted to the rows listed in `rows` [B,S]
 * (models/common.py:53-75 followed by the gather at PointDSC.py:327-329): feat_n [B,N,128] unit rows
 * -> knn_out [B,S,k] int32, nearest first, the row itself (rank 0) dropped.  Any N for k <= 63 (the rows' distances come from the
 * matrix pipe, in slices of at most 4 GiB; workspace: the handle's arena); k > 63 keeps the in-LDS form (N <= 38400). */
int gmf_knn_rows(gmf_handle* h, const float* feat_n, const int* rows, int B, int N, int S, int k, int* knn_out,
                 gmf_stream_t stream);

/* gmf_knn_rows with the listed row itself as rank 0 WHATEVER ties with it: the k nearest OTHER rows under (distance, index), so a
 * bitwise duplicate of the row at a lower index is a neighbour like any other (gmf_knn_rows drops it as rank 0 and returns the
 * row itself instead).  knn(x, k, ignore_self=False) of models/common.py:70-71 = the row followed by the k - 1 rows this returns.
 * Same distance rows as gmf_knn_rows, the row's own entry set to -inf before the selection; k > 63: the in-LDS selection on
 * those rows (N <= 38400). */
int gmf_knn_rows_self_first(gmf_handle* h, const float* feat_n, const int* rows, int B, int N, int S, int k, int* knn_out,
                            gmf_stream_t stream);

/* [ABI 5] The selection step alone: the k smallest entries behind rank 0 of every given DISTANCE row, under the order (distance,
 * index) - `topk(k + 1, largest=False)[1][..., 1:]` of models/common.py:71-74 for rows the caller has formed itself (gmf_amd.knn with
 * `normalized=False` or a feature width other than 128: distances xx_i - 2 x_i.x_j + xx_j from gmf_gemm_f32, common.py:64-69).
 * dist [B, S, ld] with ld = 32 * ceil(N / 32) floats per row (columns N .. ld - 1 are not read) -> knn_out [B, S, k] int32,
 * nearest first.  0 < k <= 63, k <= N - 1; any N. */
int gmf_knn_from_distances(gmf_handle* h, const float* dist, int B, int N, int S, int k, int* knn_out, gmf_stream_t stream);

/* Descriptor-space nearest neighbour: for every row of F0 [N0,d] the closest row of F1 [N1,d] (row-major, d <= 128),
 * ties to the lower index, fused distance GEMM + row argmin (no N0 x N1 matrix).
 *   mode 0: PointDSC matching (datasets/ThreeDMatch.py:164-166, demo_registration.py:101-103), unit descriptors:
 *           dist = sqrt(2 - 2 <a,b> + 1e-6);
 *   mode 1: DGR find_knn_gpu with nn_max_n > 1 (core/knn.py:50-64): dist = sqrt(||a-b||^2 + 1e-7) (pdist 'L2');
 *   mode 2: DGR find_knn_gpu with nn_max_n <= 1 (core/knn.py:66-70): dist = ||a-b||^2 (pdist 'SquareL2').
 * idx_out [N0] int32, dist_out [N0]. */
int gmf_nn_match(gmf_handle* h, const float* F0, const float* F1, int N0, int N1, int d, int mode, int* idx_out,
                 float* dist_out, gmf_stream_t stream);

/* gmf_nn_match for B ragged pairs in three launches, whatever B (DGR find_knn_gpu_batch, core/knn.py:106-140).  off0 / off1: HOST
 * arrays of B + 1 ascending row offsets from 0 - pair b matches rows [off0[b], off0[b+1]) of F0 against rows [off1[b], off1[b+1])
 * of F1.  idx_out [off0[B]] int32 is local to the pair, or, with global_index != 0, a row of F1 (+ off1[b], the reference's
 * concat_results); dist_out [off0[B]].  Indices and distances are bit for bit those of B gmf_nn_match calls on the slices (first
 * index among equal scores; a NaN query row gives local index 0 and distance NaN).  A pair without query rows contributes
 * nothing; a pair with query rows and no key rows is GMF_ERR_UNSUPPORTED_SHAPE, as are B = 0 and d > 128; offsets that do not
 * ascend are GMF_ERR_BAD_ARG.  No host synchronisation. */
int gmf_nn_match_batched(gmf_handle* h, const float* F0, const float* F1, const int* off0, const int* off1, int B, int d, int mode,
                         int global_index, int* idx_out, float* dist_out, gmf_stream_t stream);

/* PointDSC matching of B ragged pairs with the mutual-nearest-neighbour flag (datasets/ThreeDMatch.py:164-170, KITTI.py:94-101):
 * gmf_nn_match_batched in mode 0 without global_index - idx_out [off0[B]] int32 local to the pair and dist_out [off0[B]], bit for
 * bit - plus mutual_out [off0[B]], one byte per source row: 1 where the row is the best source row of its own winner
 * (target_idx[source_idx[i]] == i).  Every score is formed once and folded along its row and along its column; among equal scores
 * the smaller index wins on both sides (numpy's first argmin).  A row without a winner (all scores NaN) is not mutual.  off0 / off1
 * and the argument errors are those of gmf_nn_match_batched.  No host synchronisation and nothing read back: the call can be
 * captured into a graph. */
int gmf_nn_match_mutual_batched(gmf_handle* h, const float* F0, const float* F1, const int* off0, const int* off1, int B, int d,
                                int* idx_out, float* dist_out, unsigned char* mutual_out, gmf_stream_t stream);

/* The correspondence set of B ragged pairs from descriptors and keypoints, the body of PointDSC's loaders
 * (datasets/ThreeDMatch.py:163-210, KITTI.py:94-129, demo_registration.py:101-107), in five launches whatever B: the matching above,
 * the rows kept (use_mutual != 0: the mutual ones; 0: every row with a winner) compacted in source order, per pair.
 * F0 [off0[B], d], F1 [off1[B], d] unit descriptors; src_keypts [off0[B], 3], tgt_keypts [off1[B], 3]; off0 / off1 HOST arrays as
 * in gmf_nn_match_batched.  Outputs, all on the device, of capacity off0[B] rows, pair b owning rows [out_offsets[b],
 * out_offsets[b + 1]) (out_offsets [B + 1] int32, written on the device):
 *   corr_out [., 2] int64 (source row, target row), local to the pair; src_out / tgt_out [., 3] the gathered keypoints;
 *   corr_pos_out [., in_dim]: in_dim 6 = (src, tgt) minus the pair's means over its kept rows, in_dim 3 = src - tgt;
 *   src_desc_out / tgt_desc_out [., d] the gathered descriptor rows (both or neither; NULL: none);
 *   labels_out [.] fp32 0 / 1 = |R x_src + t - x_tgt| < inlier_threshold with gt_trans [B, 4, 4] fp32 row-major on the device
 *   (both or neither; NULL: none).
 * Rows behind out_offsets[B] are left as they were.  A pair's results do not depend on the other pairs of the batch.  Errors as
 * gmf_nn_match_batched; in_dim other than 3 or 6 is GMF_ERR_UNSUPPORTED_SHAPE.  No host synchronisation and nothing read back. */
int gmf_build_correspondences(gmf_handle* h, const float* F0, const float* F1, const float* src_keypts, const float* tgt_keypts,
                              const int* off0, const int* off1, int B, int d, int use_mutual, int in_dim, const float* gt_trans,
                              float inlier_threshold, int* out_offsets, long long* corr_out, float* src_out, float* tgt_out,
                              float* corr_pos_out, float* src_desc_out, float* tgt_desc_out, float* labels_out, gmf_stream_t stream);

/* The ground-truth pairs of B registration problems (DGR get_matching_indices, util/pointcloud.py:83-96, by brute force): every
 * (i, j), local to pair b, with |R_b x0_i + t_b - x1_j|^2 < radius^2, ordered by i, then j.  xyz0 [total0, 3], xyz1 [total1, 3] fp32;
 * off0 / off1 [B + 1] int32 DEVICE offsets (ascending from 0 to the totals); T [B, 4, 4] fp64 row-major (device).  In fp64:
 * p = ((T00 x + T01 y) + T02 z) + T03 (rows 1, 2 likewise), d2 = ((px - qx)^2 + (py - qy)^2) + (pz - qz)^2, every operation
 * rounded on its own; a pair at exactly `radius` is outside.
 * _count: row_start [total0 + 1] int64 (the first pair of each source row; the caller keeps it for _fill), pair_offsets [B + 1]
 * int64, *num_pairs (host) = K.  Synchronises the stream once (K).  _fill: pairs [K, 2] int64.  One launch per pass for the batch. */
int gmf_matching_indices_count(gmf_handle* h, const float* xyz0, const int* off0, const float* xyz1, const int* off1, int B,
                               long long total0, long long total1, const double* T, double radius, long long* row_start,
                               long long* pair_offsets, long long* num_pairs, gmf_stream_t stream);
int gmf_matching_indices_fill(gmf_handle* h, const float* xyz0, const int* off0, const float* xyz1, const int* off1, int B,
                              long long total0, long long total1, const double* T, double radius, const long long* row_start,
                              long long* pairs, gmf_stream_t stream);

/* The batched input of DGR's inlier network in one launch (core/trainer.py:616-678, core/correspondence.py:29-53), M predicted
 * pairs in all, pair b owning rows [off0[b], off0[b+1]) of them (off0 / off1 [B + 1] int32, device).  The pairs come as `nn` [M]
 * int32 - row m is source row m of the packed source tensors, its match nn[m] local to the pair's target rows (gmf_nn_match_batched
 * without global_index); pred_out [M, 2] int64 then receives (m - off0[b], nn[m]) - or as `pred` [M, 2] int64 (labels only).
 * Rows (coords_out non-NULL, needs `nn`): coords_out [M, 7] int32 = (coords0[m], coords1[off1[b] + nn[m], 1:]) from coords0 /
 * coords1 [*, 4] int32, and feats_out by feat_type: 0 ones [M, 1]; 1 [M, 2 c] = (a0[m], a1[off1[b] + nn[m]]), a0 / a1 [*, c]
 * descriptors, c <= 64; 2 [M, 6] = the cos of the two points, a0 / a1 [*, 3], computed in fp64 and rounded to fp32.
 * Labels (labels_out non-NULL): labels_out [M] 0 / 1 = whether i + j seeds[b] (int64, wrapping) is among pos_keys[pos_off[b] ..
 * pos_off[b+1]), which must be sorted inside each pair's range (pos_off [B + 1], seeds [B] int64, device).  No workspace, no host
 * synchronisation. */
int gmf_inlier_input(gmf_handle* h, const int* nn, const long long* pred, const int* off0, const int* off1, int B, long long M,
                     long long* pred_out, const int* coords0, const int* coords1, int* coords_out, int feat_type, const float* a0,
                     const float* a1, int c, float* feats_out, const long long* pos_keys, const long long* pos_off,
                     const long long* seeds, unsigned char* labels_out, gmf_stream_t stream);

/* rigid_transform_3d(A, B, weights, weight_threshold) (models/common.py:10-50):
 * A,B [n,k,3], weights [n,k] or NULL -> T [n,4,4].  The 3x3 SVD runs on the device. */
int gmf_procrustes_batched(gmf_handle* h, const float* A, const float* B, const float* weights, int n, int k,
                           float weight_threshold, float* T44, gmf_stream_t stream);

/* post_refinement (PointDSC.py:493-528) for B pairs independently: T_in/out [B,16]. */
int gmf_post_refinement(gmf_handle* h, const float* T_in, const float* src_keypts, const float* tgt_keypts, int B, int N,
                        float refine_threshold, int iters, float* T_out, gmf_stream_t stream);

/* DGR weighted_procrustes(X, Y, w, eps) (GMF_DeepGlobalRegistration/.../core/registration.py:91-113),
 * batched over B pairs with ragged sizes: offsets [B+1] (device int32) delimit rows of X,Y [sum N,3], w [sum N].
 * R [B,9], t [B,3].  fp64 SVD on device, no host transfer. */
int gmf_weighted_procrustes(gmf_handle* h, const float* X, const float* Y, const float* w, const int* offsets, int B,
                            float eps, float* R, float* t, gmf_stream_t stream);

/* DGR GlobalRegistration(points, trans_points, weights, max_iter, ..., max_break_count, break_threshold_ratio, ...,
 * quantization_size) (GMF_DeepGlobalRegistration/.../core/registration.py:135-194; loss core/loss.py:42-61;
 * caller core/deep_global_registration.py:334-340): weighted-Procrustes initialisation + robust Adam refinement of a 6-D
 * rotation and a translation, batched over B ragged pairs like gmf_weighted_procrustes (offsets [B+1] device int32;
 * X,Y [sum N,3]; w [sum N] or NULL for the unweighted form).  eps = the loss's eps (float32 machine epsilon in the
 * reference).  R [B,9], t [B,3], stats [B,3] = {iterations, loss, break_count}.  max_points: the largest per-pair point
 * count if the host knows it (sizes the workgroup: 16 register-resident points per thread), 0 otherwise.  One persistent
 * kernel, no host sync. */
int gmf_global_registration(gmf_handle* h, const float* X, const float* Y, const float* w, const int* offsets, int B,
                            float eps, float quantization_size, int max_iter, int max_break_count,
                            double break_threshold_ratio, float* R, float* t, float* stats, int max_points,
                            gmf_stream_t stream);

/* ---- evaluation solvers: correspondence RANSAC and point-to-point ICP (open3d's, as the reference's evaluation calls them) -- */

/* registration_ransac_based_on_correspondence (GMF_PointDSC/evaluation/test_3DMatch.py:76-94; GMF_DeepGlobalRegistration/
 * .../core/deep_global_registration.py:57-85) over B ragged pairs: row i of src [total_rows,3] corresponds to row i of
 * tgt; offsets [B+1] (device int32) delimit the pairs; mask [total_rows] (uint8, NULL = every row) picks the rows that take part.
 * H hypotheses per pair of ransac_n (3..8) distinct rows (the sampler of gmf_amd/csrc/ransac_sampler.hpp, pair index
 * first_pair + b), each an unweighted fp64 Kabsch fit scored over all participating rows: inlier when |R s + t - q|^2 < tau^2.
 * The winner has the most inliers, then the smaller sum of their d^2, then the smaller h.  max_rows: the largest pair if known
 * (sizes the row split; any value is correct).  Out: T_out [B,16], inliers [total_rows] uint8 (the winner's), fitness [B],
 * inlier_rmse [B], hypothesis [B] int64 (-1: no valid hypothesis, T = identity), sample [B, ransac_n] int64 (rows within
 * the pair).  No host synchronisation; graph-capturable. */
int gmf_ransac_correspondence(gmf_handle* h, const float* src, const float* tgt, const int* offsets, const unsigned char* mask,
                              int B, long long total_rows, int max_rows, int ransac_n, int num_hypotheses, float tau,
                              unsigned long long seed, int first_pair, float* T_out, unsigned char* inliers, float* fitness,
                              float* inlier_rmse, long long* hypothesis, long long* sample, gmf_stream_t stream);

/* registration_icp with TransformationEstimationPointToPoint (GMF_PointDSC/evaluation/benchmark_utils.py:40-56;
 * GMF_DeepGlobalRegistration/.../core/deep_global_registration.py:385-405) over B ragged pairs: src [total_src,3] with
 * src_offsets [B+1], tgt [sum Nt,3] with tgt_offsets [B+1] (device int32), init [B,16].  C = the exact nearest target row of
 * each transformed source row with d^2 < tau^2; up to max_iter passes of T <- Umeyama(C) T, stopping when both
 * |d fitness| < rel_fitness and |d rmse| < rel_rmse.  max_src / max_tgt: the largest pair sizes if known (size the grid; any
 * value >= 1 is correct).  Out: T_out [B,16], fitness [B], inlier_rmse [B], iterations [B] int32, nn [total_src] int64
 * (target row within the pair, -1 outside C).  2 max_iter + 4 launches; convergence is decided on the device. */
int gmf_icp_point_to_point(gmf_handle* h, const float* src, const int* src_offsets, const float* tgt, const int* tgt_offsets,
                           int B, long long total_src, int max_src, int max_tgt, const float* init, float tau, int max_iter,
                           double rel_fitness, double rel_rmse, float* T_out, float* fitness, float* inlier_rmse,
                           int* iterations, long long* nn, gmf_stream_t stream);

/* gmf_icp_point_to_point with a choice of nearest-neighbour search.  total_tgt: all target rows of the batch
 * (tgt_offsets[B], in 1..2^31 - 1).  search 0: the brute-force search, exactly gmf_icp_point_to_point's launches.  search 1: a
 * hashed uniform grid of cell edge tau (1 + 2^-10) over the targets, built once per call (four more launches, scratch for
 * total_tgt rows from the workspace), then each pass looks only at the 27 cells around a transformed source row.  The d^2
 * expression and the (d^2, row) order are the brute-force search's, so every output is bit-identical to search 0; the work
 * per pass falls from Ns Nt distance tests to the rows of 27 cells per source row (no gain when tau is comparable to the
 * cloud's extent).  search 1 takes total_tgt < 2^29 (the table's slots are int32).  No host synchronisation;
 * graph-capturable. */
int gmf_icp_point_to_point_ex(gmf_handle* h, const float* src, const int* src_offsets, const float* tgt, const int* tgt_offsets,
                              int B, long long total_src, int max_src, int max_tgt, const float* init, float tau, int max_iter,
                              double rel_fitness, double rel_rmse, float* T_out, float* fitness, float* inlier_rmse,
                              int* iterations, long long* nn, long long total_tgt, int search, gmf_stream_t stream);

/* registration_icp with TransformationEstimationPointToPlane (open3d 0.9) over B ragged pairs [joined under ABI 5: an added
 * entry point].  The arguments, the correspondence set C, nn, fitness, inlier_rmse (Euclidean), the loop and its stopping rule
 * are gmf_icp_point_to_point_ex's; tgt_normals [total_tgt,3] fp32 holds one normal per target row, used as given (not
 * renormalised, any sign: negating normals changes no output bit).  Only the update differs: over the rows of C whose normal is
 * finite, with p the transformed source row, q its target and n the target's normal, r = (p - q) . n and J = [p x n ; n] in
 * fp64, A = sum J J^T, b = sum J r; A x = -b is solved by LDL^T without pivoting, a pivot d_k being accepted when it is finite
 * and d_k > 2^-40 A_kk (the original diagonal entry); T <- [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)] T in fp64.  A rejected pivot
 * or an empty C leaves T as it is for that pass (the loop then normally stops at the next comparison).  max_src: an upper bound
 * of every pair's source rows (<= 0: total_src is taken); here it sizes the grid of the split step, and a pair with more rows
 * than it comes back with NaN in T_out and iterations -1.  The sums are taken per 512 source rows of a pair in a fixed tree, then
 * in ascending order: no float atomics, and a pair's bits do not depend on the batch, on max_src or on the search.
 * 3 max_iter + 5 launches (search 1: four more); no host synchronisation; graph-capturable. */
int gmf_icp_point_to_plane(gmf_handle* h, const float* src, const int* src_offsets, const float* tgt, const float* tgt_normals,
                           const int* tgt_offsets, int B, long long total_src, int max_src, int max_tgt, const float* init,
                           float tau, int max_iter, double rel_fitness, double rel_rmse, float* T_out, float* fitness,
                           float* inlier_rmse, int* iterations, long long* nn, long long total_tgt, int search,
                           gmf_stream_t stream);

/* registration_colored_icp (open3d 0.9; Park, Zhou, Koltun, ICCV 2017) over B ragged pairs [joined under ABI 5: an added entry
 * point].  gmf_icp_point_to_plane's arguments, then src_intensity [total_src] and tgt_intensity [total_tgt] (float32, one per
 * row), tgt_gradients [total_tgt,3] (float32: gmf_color_gradients of the targets) and lambda_geometric in [0, 1].  C, nn,
 * fitness, inlier_rmse (Euclidean), the loop, its stopping rule, the solve and the sum tree are gmf_icp_point_to_plane's.  The
 * sums of A and b run over the rows of C whose normal, gradient and two intensities are finite: with p the transformed source
 * row, q its target, n and g the target's normal and gradient, r_G = (p - q) . n, J_G = [p x n ; n], u = (p - q) - r_G n,
 * r_I = I_s - (g . u + I_t), m = -(g - (g . n) n), J_I = [p x m ; m] in fp64,
 * A = sum lambda J_G J_G^T + (1 - lambda) J_I J_I^T, b = sum lambda J_G r_G + (1 - lambda) J_I r_I (each term scaled by the
 * square root of its weight, taken on the host in double).  Negating normals changes no output bit; a pair's bits do not
 * depend on the batch, on max_src or on the search.  3 max_iter + 5 launches (search 1: four more); no host synchronisation;
 * graph-capturable. */
int gmf_icp_colored(gmf_handle* h, const float* src, const int* src_offsets, const float* tgt, const float* tgt_normals,
                    const int* tgt_offsets, int B, long long total_src, int max_src, int max_tgt, const float* init, float tau,
                    int max_iter, double rel_fitness, double rel_rmse, float* T_out, float* fitness, float* inlier_rmse,
                    int* iterations, long long* nn, long long total_tgt, int search, const float* src_intensity,
                    const float* tgt_intensity, const float* tgt_gradients, double lambda_geometric, gmf_stream_t stream);

/* registration_ransac_based_on_feature_matching (GMF_DeepGlobalRegistration/.../core/deep_global_registration.py:26-54) over B
 * ragged pairs: src [total_src,3] with src_offsets [B+1], tgt [total_tgt,3] with tgt_offsets [B+1] (device int32; a pair may have
 * no targets), nn [total_src] int64: the feature-space nearest target row of every source row, numbered within the pair.
 * Hypothesis h in 0 .. max_iteration - 1 (1..2^24) of pair first_pair + b draws ransac_n (3..8) distinct source rows (the
 * sampler of gmf_amd/csrc/ransac_sampler.hpp over the pair's Ns rows) and pairs each with its nn.  It passes when every nn is a
 * row of the pair's targets; when, with edge_length_threshold r in (0, 1] (<= 0: off), for every two sampled pairs
 * |s_i - s_j|^2 >= r^2 |q_i - q_j|^2 and the reverse (fp64); when the unweighted fp64 Kabsch fit succeeds; and when, with
 * checker_distance >= 0 (negative: off), every sampled pair has fp32 |R s + t - q|^2 <= checker_distance^2 under the fit
 * rounded to fp32.  The first max_validation (1..65536) passing h in increasing order are evaluated on the whole clouds: C =
 * the source rows whose exact nearest target (smallest fp32 d^2, then smallest row) has d^2 < tau^2.  The winner has the
 * largest |C| (at least 1), then the smaller sum over C of rz(d^2 2^24 / tau^2) capped at 2^24 - 1, then the smaller h; no refit.
 * search 0 tests every target of the pair; search 1 (total_tgt < 2^29) builds a hashed grid of cell edge tau (1 + 2^-10) over
 * the targets and tests the 27 cells around a transformed row: the same bits.  max_src: the largest pair's source rows if
 * known (any value >= 1 is correct).  Out: T_out [B,16], fitness [B] (|C| / Ns), inlier_rmse [B], hypothesis [B] int64 (-1:
 * no winner, T = identity, fitness = rmse = 0), sample [B, ransac_n] int64 (source rows within the pair, -1 without a winner),
 * nn_out [total_src] int64 (the winner's nearest target row within the pair, -1 outside C), validated [B] int32 (hypotheses
 * evaluated); optional (NULL: not returned) hyp [B, max_validation] int32 (the evaluated h in order, -1 padded), count
 * [B, max_validation] int32 and sum [B, max_validation] int64 (their |C| and fixed-point sums, 0 padded).  No host
 * synchronisation; graph-capturable. */
int gmf_ransac_feature_matching(gmf_handle* h, const float* src, const int* src_offsets, const float* tgt, const int* tgt_offsets,
                                const long long* nn, int B, long long total_src, long long total_tgt, int max_src, int ransac_n,
                                int max_iteration, int max_validation, float tau, float checker_distance,
                                float edge_length_threshold, unsigned long long seed, int first_pair, int search, float* T_out,
                                float* fitness, float* inlier_rmse, long long* hypothesis, long long* sample, long long* nn_out,
                                int* validated, int* hyp, int* count, long long* sum, gmf_stream_t stream);

/* ---- multiway registration (GMF_PointDSC/multiway/test_multi_ate.py) ------------------------------------

 * open3d 0.9's get_information_matrix_from_point_clouds for E edges over F shared clouds.  points [sum N, 3] (device) holds the
 * clouds packed once; cloud_offsets [F + 1], edge_source and edge_target [E] are HOST arrays (the call plans its chunks from
 * them; cloud offsets increase strictly from 0).  transformation [E, 16] fp64 (device) maps the source cloud's rows into the
 * target's frame.  C_e: the source rows whose transformed row has its exact nearest target row within tau, found as
 * gmf_icp_point_to_point_ex(search = 1, max_iter = 0) finds it, bit for bit.  info [E, 36] fp64 = the sum over C_e of G^T G with
 * G = [-[q]x | I] at the matched target row q, count [E] = |C_e|, nn (may be null) [the sum of the edges' source rows] the
 * matched target row within its cloud or -1, edge after edge.  A transformation that is not finite gives zeros.  No floating-point
 * atomics: an edge's numbers do not depend on the other edges of the call.  E == 0 is legal and does nothing. */
int gmf_information_matrix(gmf_handle* h, const float* points, const int* cloud_offsets, int F, const int* edge_source,
                           const int* edge_target, int E, const double* transformation, float tau, double* info, int* count,
                           long long* nn, gmf_stream_t stream);

/* open3d's GlobalOptimizationConvergenceCriteria and GlobalOptimizationOption */
typedef struct gmf_posegraph_options {
  int max_iteration, max_iteration_lm, reference_node;      /* open3d: 100, 20, -1 */
  double min_relative_increment, min_relative_residual_increment, min_right_term, min_residual;   /* open3d: 1e-6 each */
  double edge_prune_threshold, preference_loop_closure;     /* open3d: 0.25, 1.0 */
} gmf_posegraph_options;

/* open3d's global_optimization (Levenberg-Marquardt with a line process per uncertain edge, two passes with the pruning in
 * between) for G ragged pose graphs, one workgroup each; the algorithm is written out in DESIGN.md section 4m.  node_offsets,
 * edge_offsets [G + 1], edge_source, edge_target [m] (node indices within the graph) are HOST arrays.  Device: poses [n, 16] fp64
 * in and out, edge_transformation [m, 16], edge_information [m, 36], edge_uncertain [m], edge_mask [m] or null (0: the edge is
 * treated as absent), line_process [m] (0 for an edge that is masked or pruned), kept [m], stats [G, 2, 4] int32 (per pass: outer
 * iterations, rejected steps, stop code, edges that took part), residual [G, 2], trace [G, 2, max_iteration + 1, 2] (residual and
 * lambda after each outer iteration, NaN padded) or null.  Stop codes: 0 max_iteration, 1 min_right_term, 2 min_relative_increment,
 * 3 min_relative_residual_increment, 4 min_residual, 5 max_iteration_lm, 6 a pivot was not positive (GMF_STATUS_POSEGRAPH_PIVOT is set).
 * At most 256 nodes and 65536 edges per graph (GMF_ERR_UNSUPPORTED_SHAPE beyond). */
int gmf_posegraph_optimize(gmf_handle* h, double* poses, const int* node_offsets, const int* edge_offsets, int G,
                           const int* edge_source, const int* edge_target, const double* edge_transformation,
                           const double* edge_information, const unsigned char* edge_uncertain, const unsigned char* edge_mask,
                           const gmf_posegraph_options* opt, double* line_process, unsigned char* kept, int* stats, double* residual,
                           double* trace, gmf_stream_t stream);

/* The spectral-matching baseline SM(corr, src_keypts, tgt_keypts, args, top_ratio) of the reference's evaluation
 * (GMF_PointDSC/baseline_scripts/baseline_3DMatch.py:19-53; baseline_KITTI.py:51) over B ragged pairs, matrix-free: corr
 * [sum N,6], src / tgt [sum N,3] (float32), offsets [B+1] (device int32; a pair may be empty), topk [B] (device int32: the k
 * rows to label, int(N top_ratio) in the reference).  Per pair, in fp32:
 *   d_ij = |c_i[0:3] - c_j[0:3]| - |c_i[3:6] - c_j[3:6]| (coordinate differences, then the root of the sum of squares),
 *   m_ij = max(0, 4.5 - d_ij^2 / (2 sigma^2)), sigma = inlier_threshold / 3, m_ii = 0;
 *   v = ones, `iterations` (1..1000; the reference: 10) times v <- M v, v <- v / (|v|_2 + 1e-6);
 *   labels = 1 on the k rows of largest v, equal values to the smaller row (the reference's argsort leaves ties open);
 *   T = rigid_transform_3d(src, tgt, v * labels) (GMF_PointDSC/models/common.py:10-50): weights not normalised, centroids over
 *   sum w + 1e-6, R = V diag(1, 1, det) U^T by the fp64 Kabsch; k = 0, an all-zero v or an empty pair give the identity.
 * M is never formed: each product recomputes its entries, rows on lanes, the columns streamed through LDS and split over
 * workgroups by a rule of the pair's own N; the partial sums are added in split order (no floating-point atomics), so a pair has
 * the same bits alone, in any batch and on every run.  max_n: an upper bound of the largest pair's rows (0: every pair is empty);
 * it sizes the grid and the workspace (up to 32 B max_n floats: give the largest pair itself where it is known).  B <= 65535,
 * B max_n < 2^31.  Out: eig_out [sum N] (v), labels_out [sum N] (float 0 / 1), T_out [B,16].  gmf_set_tuning:
 * "spectral_col_splits" (0 = by the rule, 1..32 = forced).  The two square roots of a matrix entry are v_sqrt_f32 as it comes (1
 * ulp).  A pair with more than max_n rows, or whose rows end past B max_n, is not computed: its T_out is the identity and its
 * eig_out and labels_out rows are zeros; no status is raised.  2 iterations + 2 launches, no host synchronisation;
 * graph-capturable. */
int gmf_spectral_matching(gmf_handle* h, const float* corr, const float* src, const float* tgt, const int* offsets, int B, int max_n,
                          float inlier_threshold, const int* topk, int iterations, float* eig_out, float* labels_out, float* T_out,
                          gmf_stream_t stream);

/* The maximum-clique baseline PMC(corr, src_keypts, tgt_keypts, args) of the reference's evaluation
 * (GMF_PointDSC/baseline_scripts/baseline_3DMatch.py:56-77) over B ragged pairs, exact [joined under ABI 5: added entry points]:
 * corr [total_rows,6], src / tgt [total_rows,3] (float32), offsets [B+1] (device int32; a pair may be empty).  Per pair of N rows:
 *   graph   in fp32, every operation rounded on its own: a = ((dx^2 + dy^2) + dz^2) on the differences of columns 0..2, b alike
 *           on columns 3..5; metric 0: edge iff |a - b| < inlier_threshold (the reference's rule: squared lengths); metric 1:
 *           edge iff |sqrt(a) - sqrt(b)| < inlier_threshold (correctly rounded roots).  No diagonal.
 *   clique  a maximum clique of that graph: a pure function of the pair's rows whenever exact_out is 1 - the same alone, in any
 *           batch and on every run.  A graph without edges gives the smallest row alone.
 *   pose    rigid_transform_3d(src, tgt, labels) (GMF_PointDSC/models/common.py:10-50) with 0 / 1 weights: centroids over
 *           sum w + 1e-6, the fp64 Kabsch of gmf_spectral_matching.  An empty pair gives the identity.
 * max_steps (>= 1) bounds the branch-and-bound nodes expanded per pair; the count can pass it by 256 at most (one per search
 * wave).  Where it ends a search exact_out is 0 and the labels are the largest clique found.  max_n: an upper bound of the largest
 * pair's rows, at most 8192 (GMF_ERR_UNSUPPORTED_SHAPE above); total_rows: the rows of corr.  They size the grid and the
 * workspace (2 total_rows ceil(max_n / 64) words of bit rows and 512 B max_n bytes of clique lists).  A pair with more than
 * max_n rows, or whose rows end past total_rows, is not computed: identity, zeros, size 0, exact 0.  B <= 65535.
 * Out: labels_out [total_rows] (float 0 / 1), T_out [B,16], size_out [B], exact_out [B], steps_out [B], degree_out [total_rows]
 * (the graph's row sums).  7 launches, no host synchronisation; graph-capturable. */
int gmf_max_clique(gmf_handle* h, const float* corr, const float* src, const float* tgt, const int* offsets, int B,
                   long long total_rows, int max_n, float inlier_threshold, int metric, long long max_steps, float* labels_out,
                   float* T_out, int* size_out, int* exact_out, long long* steps_out, int* degree_out, gmf_stream_t stream);

/* The graph of gmf_max_clique alone: bits_out [total_rows, ceil(max_n / 64)] 64-bit words, bit j % 64 of word j / 64 of row
 * offsets[b] + i = edge (i, j) of pair b; bits past a pair's last column are zero, words past its last word are not written.
 * degree_out [total_rows].  One launch. */
int gmf_pmc_graph(gmf_handle* h, const float* corr, const int* offsets, int B, long long total_rows, int max_n,
                  float inlier_threshold, int metric, unsigned long long* bits_out, int* degree_out, gmf_stream_t stream);

/* ---- fragments from depth frames: TSDF fusion (open3d's ScalableTSDFVolume, as the reference's make_fragments.py drives it) ---- */

/* G ragged fragments of posed depth frames -> the vertices of each fragment's marching-cubes mesh, in three calls [joined under
 * ABI 5: added entry points].  The arithmetic, step by step, is DESIGN.md section 4o (tests/tsdf_reference.py restates it and the
 * kernels equal it bit for bit); a volume unit is 16^3 voxels, unit_length = 16 voxel_length.
 *
 * Shared inputs: depth [F,H,W] on the device, uint16 sensor values (depth_is_u16 != 0: d = float(v) / float(depth_scale)) or
 * float32 metres (a negative or non-finite value is 0); d >= float(depth_trunc) is 0; 0 is "no measurement".  frame_offsets [G+1]
 * (device int32, not decreasing, from 0 to F: fragment g owns frames frame_offsets[g] .. frame_offsets[g+1] - 1, possibly none).
 * One pinhole camera (fx, fy, cx, cy) per call.  G <= 65535, F H W < 2^31.
 *
 * gmf_tsdf_allocate: poses [F,16] camera-to-world, fp64 row-major, on the device.  Every stride-th pixel of every stride-th row
 * with d > 0 is back-projected in fp64 and every unit of the box floor((p -+ sdf_trunc) / unit_length) exists.  Out (device):
 * unit_keys_out [max_units,3] int32 and birth_out [max_units] int32, of which the first *num_units rows are written - the units of
 * fragment 0 in ascending (x, y, z) order, then fragment 1's, ...; birth = the first frame (counted within the fragment) that
 * touches the unit; unit_offsets_out [G+1] int32.  *num_units (host).  Synchronises the stream once.  GMF_ERR_UNSUPPORTED_SHAPE
 * when the frames touch more than max_units (1..2^22) units, or a unit index leaves +-32767; the outputs are then not valid.
 * Workspace: 12 bytes per table slot (a power of two >= 2 max_units, at least 1024), 16 per max_units and the radix sort's. */
int gmf_tsdf_allocate(gmf_handle* h, const void* depth, int depth_is_u16, const double* poses, const int* frame_offsets, int G, int F,
                      int H, int W, double fx, double fy, double cx, double cy, double voxel_length, double sdf_trunc,
                      double depth_scale, double depth_trunc, int stride, int max_units, int* unit_keys_out, int* birth_out,
                      int* unit_offsets_out, long long* num_units, gmf_stream_t stream);

/* gmf_tsdf_integrate: poses_inv [F,16] world-to-camera, fp64 (the caller inverts; the kernel rounds them to float32).  unit_keys
 * [num_units,3], unit_offsets [G+1], birth [num_units] as gmf_tsdf_allocate wrote them.  Every unit takes the frames >= its birth
 * of its fragment, in order: projective update with weight 1, tsdf = (tsdf w + min(1, sdf / sdf_trunc)) / (w + 1), in fp32.
 * Out: tsdf_out, weight_out [num_units,16,16,16] float32, voxel (x, y, z) of a unit at x 256 + y 16 + z; every voxel is written
 * (0 / 0 where no frame reached it).  Workspace: 4 (F + 1) H W bytes.  2 launches, no host synchronisation. */
int gmf_tsdf_integrate(gmf_handle* h, const void* depth, int depth_is_u16, const double* poses_inv, const int* frame_offsets, int G,
                       int F, int H, int W, double fx, double fy, double cx, double cy, double voxel_length, double sdf_trunc,
                       double depth_scale, double depth_trunc, const int* unit_keys, const int* unit_offsets, const int* birth,
                       int num_units, float* tsdf_out, float* weight_out, gmf_stream_t stream);

/* gmf_tsdf_extract: the vertex set of the marching-cubes mesh of the volume.  An edge between two voxels adjacent along an axis
 * yields a vertex when both have weight > 0, their tsdf differ in sign (< 0 against >= 0) and one of the four 2x2x2 cubes around
 * the edge has eight voxels of weight > 0 (neighbouring units of the same fragment included); it lies on the edge at
 * |tsdf_a| / (|tsdf_a| + |tsdf_b|), computed in fp64.  Order: fragment, unit, voxel index, axis.
 * points_out NULL: counts - point_offsets_out [G+1] (device int32) is written and *num_points (host) after synchronising the
 * stream once.  points_out [max_points,3] float32: the vertices are written as well (any past max_points are dropped: give what
 * the counting call reported), nothing is read back and num_points is not touched.  Fewer than 2^31 vertices per call. */
int gmf_tsdf_extract(gmf_handle* h, const int* unit_keys, const int* unit_offsets, int G, int num_units, const float* tsdf,
                     const float* weight, double voxel_length, float* points_out, long long max_points, int* point_offsets_out,
                     long long* num_points, gmf_stream_t stream);

/* The RGB8 forms (open3d's color_type = RGB8; tests/tsdf_color_reference.py restates them)
 * [joined under ABI 5: added entry points].  They compute what the two entries above compute, with the same bits, and colours
 * beside it.
 *
 * gmf_tsdf_integrate_color: color [F,H,W,3] uint8 on the device, channels R, G, B, the frames of `depth`.  A voxel's colour starts
 * at (0, 0, 0) and changes exactly when its tsdf does, from the same pixel: c_k = (c_k w + float(color_k)) / (w + 1) in fp32 with w
 * the weight before the update; the colour of a pixel without a depth measurement is never read.  color_out [num_units,16,16,16,3]
 * float32 in 0..255, every voxel written (exactly 0 where the weight is 0).  Workspace: 4 (2 F + 1) H W bytes. */
int gmf_tsdf_integrate_color(gmf_handle* h, const void* depth, int depth_is_u16, const unsigned char* color, const double* poses_inv,
                             const int* frame_offsets, int G, int F, int H, int W, double fx, double fy, double cx, double cy,
                             double voxel_length, double sdf_trunc, double depth_scale, double depth_trunc, const int* unit_keys,
                             const int* unit_offsets, const int* birth, int num_units, float* tsdf_out, float* weight_out,
                             float* color_out, gmf_stream_t stream);

/* gmf_tsdf_extract_color: color [num_units,16,16,16,3] as gmf_tsdf_integrate_color wrote it.  points_out NULL: the counting call
 * of gmf_tsdf_extract; neither output is touched.  Otherwise points_out and colors_out [max_points,3] float32 are both written,
 * under the same max_points guard: row i of colors_out is the colour of vertex i, in 0..1 - with ta = |tsdf_a|, tb = |tsdf_b|,
 * ((tb c_a + ta c_b) / (ta + tb)) / 255 in fp64, rounded once (the vertex lies ta / (ta + tb) of the way from a to b). */
int gmf_tsdf_extract_color(gmf_handle* h, const int* unit_keys, const int* unit_offsets, int G, int num_units, const float* tsdf,
                           const float* weight, const float* color, double voxel_length, float* points_out, float* colors_out,
                           long long max_points, int* point_offsets_out, long long* num_points, gmf_stream_t stream);

/* gmf_tsdf_extract_mesh [joined under ABI 5: an added entry point]: the marching-cubes mesh of the volume, DESIGN.md section 4o
 * steps 4 to 6 (tests/tsdf_mesh_reference.py restates 5 and 6).  The vertices, their order and their bits are gmf_tsdf_extract's
 * (with `color` [num_units,16,16,16,3], or NULL: gmf_tsdf_extract_color's colours as well).  A cube of 2x2x2 voxels that all have
 * weight > 0 and do not all lie on one side yields the triangles of the classic case table (corner i of the cube sets bit i of
 * the case when its tsdf < 0); a triangle is three vertex indices counted from its fragment's first vertex, wound so that the
 * normals point from negative to positive tsdf.  Order: fragment, unit, voxel index of the cube's origin, table row.  A vertex
 * normal is the normalised sum, in fp64 and in ascending triangle order, of (p_j - p_i) x (p_l - p_i) over its triangles (i, j, l),
 * p the float32 positions that are returned; (0, 0, 1) where the sum has no finite positive length.
 * The volume is looked at only through weight > 0; unit_keys must be ascending in (x, y, z) and distinct within each fragment.
 * Every output NULL: counts - point_offsets_out and triangle_offsets_out [G+1] (device int32) are written, and *num_points and
 * *num_triangles (host) after synchronising the stream once.  Otherwise points_out, normals_out [max_points,3] float32,
 * colors_out [max_points,3] (exactly when color is given) and triangles_out [max_triangles,3] int32 are written as well (a row
 * past its cap is dropped: give what the counting call reported), nothing is read back and the two counts are not touched.
 * Workspace: about 5.2 KB per unit.  Fewer than 2^31 vertices and triangles per call. */
int gmf_tsdf_extract_mesh(gmf_handle* h, const int* unit_keys, const int* unit_offsets, int G, int num_units, const float* tsdf,
                          const float* weight, const float* color, double voxel_length, float* points_out, float* normals_out,
                          float* colors_out, long long max_points, int* triangles_out, long long max_triangles, int* point_offsets_out,
                          int* triangle_offsets_out, long long* num_points, long long* num_triangles, gmf_stream_t stream);

/* ---- RGB-D odometry (open3d 0.9's compute_rgbd_odometry with the hybrid Jacobian, as make_fragments.py calls it) -------------- */

/* The contract is DESIGN.md section 4p.  The pyramid of F frames of H x W is ONE float32 buffer: level l (0 .. levels-1) is
 * [F,6,h_l,w_l] with h_l = H >> l, w_l = W >> l and the planes I, D, Idx, Idy, Ddx, Ddy, and starts where level l-1 ends
 * (6 F (h_0 w_0 + ... + h_l-1 w_l-1) floats in).  6 F H W must stay below 2^31; levels in 1..8.
 *
 * gmf_rgbd_pyramids: color [F,H,W] uint8 (color_kind 0: I = v / 255), [F,H,W,3] uint8 (1: I = ((0.2990 R + 0.5870 G) + 0.1140 B) / 255
 * in float32) or [F,H,W] float32 (2: as it is); depth [F,H,W] uint16 (d = v / depth_scale) or float32 (metres; negative and
 * non-finite are none); d >= depth_trunc, d < min_depth, d > max_depth and d <= 0 become NaN.  Level 0 is the 3 x 3 Gaussian of
 * both, level l+1 the 2 x 2 mean of the Gaussian of I_l and of D_l, the gradients are 3 x 3 Sobel filters; every filter is two
 * 3-tap passes (rows, then columns; indices clamped; fp64 accumulator, float32 result).  planes_out: every level.  No host
 * synchronisation. */
int gmf_rgbd_pyramids(gmf_handle* h, const void* color, int color_kind, const void* depth, int depth_is_u16, int F, int H, int W,
                      double depth_scale, double depth_trunc, double min_depth, double max_depth, int levels, float* planes_out,
                      gmf_stream_t stream);

/* gmf_rgbd_correspondences: for E pairs (pair_source[e], pair_target[e]; device int32, frames of `planes`) and poses
 * transformation [E,16] (fp64, source camera to target camera), at `level` with the intrinsics (fx, fy, cx, cy) * 2^-level: every
 * source pixel with depth d_s goes to p = d_s (K R K^-1 (u, v, 1)) + K t, (u_t, v_t) = trunc(p_xy / p_z + 0.5), and is a candidate
 * of that target pixel when it is inside, has depth d_t and |p_z - d_t| <= max_depth_diff; the candidate of smallest d_s, then of
 * smallest source index, wins.  map_out [E,h,w] int32: the winning source pixel v_s w + u_s, or -1.  A pair that names a frame
 * outside 0..F-1 gets -1 everywhere.  No host synchronisation. */
int gmf_rgbd_correspondences(gmf_handle* h, const float* planes, int F, int H, int W, int levels, int level, const int* pair_source,
                             const int* pair_target, int E, const double* transformation, double fx, double fy, double cx, double cy,
                             double max_depth_diff, int* map_out, gmf_stream_t stream);

/* gmf_rgbd_odometry: E pairs from odo_init [E,16] (fp64, its last row taken as 0 0 0 1; NULL: identity).  iterations [levels] (HOST ints): iterations[0] runs
 * at the coarsest level.  Out (device): success_out [E] bytes (1 / 0), transformation_out [E,16] and information_out [E,36] fp64
 * (both the identity for a failed pair).  Optional (NULL: not written): scales_out [E,2] (s_src, s_tgt; not written for a pair
 * without level-0 correspondences), and, together, trace_n_out [E,N] int32 and trace_out [E,N,65] fp64 with N = sum of
 * iterations, per iteration the count, then A (36), b (6), r2, x (6) and the pose after the update (16); an iteration that fails
 * writes its count, A, b and r2 only, the iterations after a failure write nothing.  3 launches per iteration for all pairs; the
 * sums are a function of the pair alone (no floating-point atomics, a block partition fixed by the level).  No host
 * synchronisation. */
int gmf_rgbd_odometry(gmf_handle* h, const float* planes, int F, int H, int W, int levels, const int* pair_source, const int* pair_target,
                      int E, const double* odo_init, double fx, double fy, double cx, double cy, double max_depth_diff,
                      const int* iterations, unsigned char* success_out, double* transformation_out, double* information_out,
                      double* scales_out, int* trace_n_out, double* trace_out, gmf_stream_t stream);

/* ---- point-cloud descriptors: radius kNN, normals, FPFH, voxel grids (open3d's, as the reference's feature scripts call them) -- */

/* Radius-bounded k nearest (open3d KDTreeFlann::SearchHybrid) over B ragged clouds: pts [total_rows,3] (float32), offsets
 * [B+1] (device int32).  For every row, up to max_nn (1..256) rows of the same cloud with d^2 < radius^2, the row itself
 * included, the smallest in the total order of (d^2, row).  d^2 = (dx dx + dy dy) + dz dz in fp64 from the fp32 coordinates,
 * each operation rounded on its own.  Out, sorted by that key: idx [total_rows, max_nn] int32 (row within the cloud, -1
 * padding), d2 [total_rows, max_nn] float64 (0 padding; may be NULL), count [total_rows] int32.  Hashed uniform grid sized
 * from total_rows alone; no host synchronisation, graph-capturable. */
int gmf_radius_knn(gmf_handle* h, const float* pts, const int* offsets, int B, long long total_rows, double radius, int max_nn,
                   int* idx, double* d2, int* count, gmf_stream_t stream);

/* open3d estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) without prior normals: the neighbour set of gmf_radius_knn;
 * with >= 3 neighbours the fp64 covariance E[x x^T] - mu mu^T and the eigenvector of its smallest eigenvalue by open3d's
 * FastEigen3x3 (sign as that algorithm yields it), else (0, 0, 1).  normals [total_rows,3] float32.  No host synchronisation. */
int gmf_estimate_normals(gmf_handle* h, const float* pts, const int* offsets, int B, long long total_rows, double radius,
                         int max_nn, float* normals, gmf_stream_t stream);

/* open3d 0.9's InitializePointCloudForColoredICP(KDTreeSearchParamHybrid(radius, max_nn)) [joined under ABI 5: an added entry
 * point]: the colour gradient of every row over the neighbour list of gmf_radius_knn.  normals [total_rows,3] float32, used as
 * given (negating any of them changes no output bit); intensity [total_rows] float32, one per row.  A row with fewer than 4
 * list entries gets 0.  Otherwise the first entry is skipped (the query row, unless an earlier row coincides with it) and over
 * the others in list order, in fp64 from the fp32 inputs: e = v_a - v, d = e - (e . n) n, A = sum d d^T + (count - 1)^2 n n^T,
 * b = sum d (I_a - I); A g = b by 3 x 3 LDL^T without pivoting, a pivot d_k being accepted when it is finite and
 * d_k > 2^-40 A_kk.  A rejected pivot or a non-finite component of g gives g = 0 (open3d applies whatever ldlt() returns).
 * gradients [total_rows,3] float32.  Fixed summation order; no host synchronisation. */
int gmf_color_gradients(gmf_handle* h, const float* pts, const float* normals, const float* intensity, const int* offsets, int B,
                        long long total_rows, double radius, int max_nn, float* gradients, gmf_stream_t stream);

/* open3d compute_fpfh_feature(KDTreeSearchParamHybrid(radius, max_nn)): the neighbour set of gmf_radius_knn, the query excluded
 * by index; SPFH from the fp64 pair features (11 bins per angle), FPFH = the SPFH of the neighbours weighted by 1 / d^2, each
 * 11-bin block renormalised to 100, plus the row's own SPFH.  features [total_rows,33] float32 (row-major; open3d's is
 * [33,N]).  Fixed summation order: bitwise repeatable.  No host synchronisation. */
int gmf_compute_fpfh(gmf_handle* h, const float* pts, const float* normals, const int* offsets, int B, long long total_rows,
                     double radius, int max_nn, float* features, gmf_stream_t stream);

/* open3d voxel_down_sample(voxel): per cloud the grid origin min(pts) - voxel/2, the voxel of a row floor((p - origin) /
 * voxel), out_pts [<= total_rows,3] the fp64 mean of each voxel's rows (summed in ascending row order) stored as float32, the
 * voxels of a cloud in first-occurrence order (by their smallest row).  out_offsets [B+1] (device int32), *num_out (host) the
 * number of voxels.  Synchronises the stream once (the count); GMF_ERR_UNSUPPORTED_SHAPE when a voxel index leaves int32 or
 * a coordinate is not finite. */
int gmf_voxel_down_sample(gmf_handle* h, const float* pts, const int* offsets, int B, long long total_rows, double voxel,
                          float* out_pts, int* out_offsets, long long* num_out, gmf_stream_t stream);

/* gmf_voxel_down_sample for a cloud with colours [joined under ABI 5: an added entry point]: colors [total_rows,3] float32.
 * out_pts, their order, out_offsets, *num_out and the errors are gmf_voxel_down_sample's, bit for bit; out_colors
 * [<= total_rows,3] is the fp64 mean of each voxel's colours over the same rows in ascending row order, stored as float32
 * (open3d's AccumulatedPoint). */
int gmf_voxel_down_sample_color(gmf_handle* h, const float* pts, const float* colors, const int* offsets, int B,
                                long long total_rows, double voxel, float* out_pts, float* out_colors, int* out_offsets,
                                long long* num_out, gmf_stream_t stream);

/* MinkowskiEngine sparse_quantize(pts / voxel, return_index=True) as DGR's preprocess calls it: the voxel floor(p / voxel),
 * out_idx [<= total_rows] int32 the smallest row (within its cloud) of each voxel, ascending per cloud.  out_offsets, num_out
 * and the errors as gmf_voxel_down_sample. */
int gmf_voxel_select(gmf_handle* h, const float* pts, const int* offsets, int B, long long total_rows, double voxel,
                     int* out_idx, int* out_offsets, long long* num_out, gmf_stream_t stream);

/* ---- sparse convolution over up to 6-D coordinates (MinkowskiEngine's, as DGR's inlier network ResUNetBN2C uses it) ------- */

/* Sizes the device block of a sparse plan: M input rows of D (1..6) spatial coordinates, `levels` (1..8) tensor strides 1, 2,
 * 4, ... and num_maps (0..16) kernel maps, maps [num_maps][3] = (k, out level, in level): an odd hypercube edge k with
 * k^D <= 1024 and |out - in| <= 1.  Same level: output o reads input o + d t (t the level's stride); out = in + 1: o + d t (t the
 * input stride); out = in - 1 (transposed): o - d t (t the output stride), so fine output p reads coarse input o when
 * p = o + d t.  Offset index d has the first spatial axis varying fastest.  Every buffer is sized from M and k^D. */
int gmf_sparse_plan_bytes(gmf_handle* h, long long M, int D, int levels, int num_maps, const int* maps, long long* bytes);

/* Builds the plan into `plan` (device, >= gmf_sparse_plan_bytes) from coords [M, 1 + D] int32 (device; the batch index in
 * column 0, rows unique).  Level 0 is the input rows in input order; level l + 1 holds the unique (batch, floor(c / 2^(l+1)) *
 * 2^(l+1)) of level l, ascending in (batch, c_1 .. c_D).  Each kernel map is CSR over its output rows: row_ptr [M + 1] int32 and
 * pairs [M * k^D] of (offset index, input row) int32 pairs, ascending offset per row; rows beyond a level's count have none.  Its
 * offset-major form: by_off [M * k^D] int32, the CSR pair indices sorted by offset (ascending row within one offset), and
 * off_start [k^D + 1] int32, offset d's pairs being by_off[off_start[d] .. off_start[d + 1]).
 * offsets (host, 1 + levels + 4 num_maps) receives byte offsets into `plan`: the int32 row counts of the levels ([16]), the
 * coordinates of each level ([M][8] int32: batch, c_1 .. c_D, zeros), then (row_ptr, pairs, by_off, off_start) of each map.  A
 * duplicate input row sets GMF_STATUS_SPARSE_DUPLICATE.  No host synchronisation: graph-capturable. */
int gmf_sparse_build_plan(gmf_handle* h, const int* coords, long long M, int D, int levels, int num_maps, const int* maps,
                          void* plan, long long plan_bytes, long long* offsets, gmf_stream_t stream);

/* Sparse convolution, fp32 throughout: y[o] = epilogue(sum over the map's pairs (d, i) of row o of [xa | xb][i] W[d]), W [K, ca + cb,
 * cout] (MinkowskiEngine's `kernel` layout), xa [*, ca], xb [*, cb] (cb may be 0: one source) row-major.  row_ptr / pairs /
 * by_off / off_start: a map of gmf_sparse_build_plan, or all NULL for the identity map (K = 1, nsplit = 1).  n_out: device
 * pointer to the output row count (a plan's level count); rows >= *n_out are not written.  epilogue: v * scale[c] + shift[c]
 * (one fma; NULL scale = 1, NULL shift = 0: a folded eval BatchNorm or a bias), + residual [*, cout] (may be NULL), then
 * max(v, 0) if relu.  y must not overlap any input.  The offsets are cut into nsplit (1..K) fixed slices, slice(d) = d nsplit /
 * K.  The workgroups of a slice walk the offset-major pair lists, so each weight block W[d] is read once per 64 pairs of d (per
 * output-row group when W is at most 16 MiB), and write per-slice partial sums (workspace nsplit x cap_out x cout floats); a
 * second pass adds a row's slices in order.  Each output element sums its offsets in ascending order, its input channels as
 * 16-channel chains in order.  No float atomics: bitwise repeatable and independent of the input row order. */
int gmf_sparse_conv(gmf_handle* h, const int* row_ptr, const int* pairs, const int* by_off, const int* off_start, int K,
                    const int* n_out, long long cap_out, const float* xa, int ca, const float* xb, int cb, const float* W, int cout,
                    const float* scale, const float* shift, const float* residual, int relu, int nsplit, float* y,
                    gmf_stream_t stream);

/* Narrow-input sparse convolution (FCGF's conv1: Cin = 1, k = 7), fp32: y[o] = epilogue(sum over the CSR pairs (d, i) of row o of
 * x[i] W[d]), W [K, cin, cout] (K 1..1024, cin 1..8, cout 1..64), x [*, cin] row-major.  row_ptr / pairs: the CSR form of a map
 * of gmf_sparse_build_plan (the offset-major lists are not read).  n_out, cap_out, the epilogue (scale, shift, residual, relu)
 * and the rule that y must not overlap an input are gmf_sparse_conv's; rows >= *n_out are not written.  Each output element is
 * ONE fma chain over its row's pairs in ascending offset, its input channels in order inside a pair; W is held in LDS when
 * K cin cout x 4 B <= 64 KiB, else read from global memory.  No workspace, no float atomics: bitwise repeatable and independent
 * of the input row order and of which other rows or batches share the plan.  No host synchronisation. */
int gmf_sparse_conv_narrow(gmf_handle* h, const int* row_ptr, const int* pairs, int K, const int* n_out, long long cap_out,
                           const float* x, int cin, const float* W, int cout, const float* scale, const float* shift,
                           const float* residual, int relu, float* y, gmf_stream_t stream);

/* FCGF's head (model/resunet.py:641-648), fp32, per row o < *n_out (device count, rows >= it are not written):
 * h = max([xa | xb][o] W1, 0) with W1 [ca + cb, hid] (conv1_tr, 1x1, no bias, then MEF.relu), y = h W2 + bias with W2 [hid, cout]
 * and bias [cout] (may be NULL: 0) (final), then, if normalize, y / (sqrt(sum_j y_j^2) + 1e-8).  ca, hid, cout 1..64, cb 0..64
 * (xa [*, ca], xb [*, cb] row-major; xb may be NULL when cb = 0).  Each hidden and output element is one fma chain over its
 * inputs in order (xa's, then xb's); the squared norm is one fma chain over the outputs in order.  y must not overlap an input.
 * Both weight blocks are held in LDS; no workspace, no host synchronisation.  An all-zero y gives zeros. */
int gmf_sparse_head_l2(gmf_handle* h, const int* n_out, long long cap_out, const float* xa, int ca, const float* xb, int cb,
                       const float* W1, int hid, const float* W2, int cout, const float* bias, int normalize, float* y,
                       gmf_stream_t stream);

/* Packs a ResUNetBN2C state_dict (host tensors) for gmf_sparse_conv: DGR's inlier network (resunet_new.py) or the FCGF feature
 * network (resunet.py), whose 23 convolutions have the same names.  For each of its GMF_SPARSE_RESUNET_LAYERS convolutions in
 * forward order (conv1, block1.conv1, block1.conv2, conv2, ..., conv2_tr, block2_tr.conv1, block2_tr.conv2, conv1_tr, final) the
 * kernel ([K, Cin, Cout], or [Cin, Cout] when K = 1), the eval BatchNorm (eps 1e-5) folded in fp64 into scale / shift, and
 * final.bias ([1, Cout]) as its shift.  layout [GMF_SPARSE_RESUNET_LAYERS][6] receives (kernel, scale, shift offsets in floats
 * into `dev`, -1 where absent; K, Cin, Cout); need_floats the size of the block.  dev == NULL: layout only; else the block is
 * copied to `dev` (dev_floats >= *need_floats; synchronous). */
#define GMF_SPARSE_RESUNET_LAYERS 23
int gmf_sparse_pack_resunet(gmf_handle* h, const gmf_tensor* tensors, int n_tensors, float* dev, long long dev_floats,
                            long long* layout, long long* need_floats);

/* ---- training of the sparse network: sparse-convolution weight gradient, BatchNorm over a level's device-counted rows ---- */

/* Weight gradient of gmf_sparse_conv, fp32: dW[d] = sum over the pairs (d, i) of output rows o < *n_out of [xa | xb][i]^T dy[o],
 * dW [K, ca + cb, cout] (every offset written; 0 for an offset without pairs).  The map arguments are gmf_sparse_conv's (all NULL:
 * the identity map, K = 1, pair j = row j).  dy [*, cout] holds the output level's rows.  The data gradient needs no entry point
 * of its own: it is gmf_sparse_conv over the transposed map with W'[d] = W[s(d)]^T (gmf_amd/sparse.py: sparse_conv_backward).
 * Sum order: each offset's pair list (by_off, ascending output row) is cut into chunks of P = max(64, ceil(nnz / (S - K))) pairs,
 * nnz the map's pair count and S = K + max(K, 256) the chunk slots; inside a chunk 16-pair fma chains are added in pair order, and
 * an offset's chunks are added in chunk order by a second pass.  The order depends only on the map and K: bitwise repeatable, no
 * float atomics.  Workspace: S x (ca + cb) x cout + K + 2 floats.  No host synchronisation. */
int gmf_sparse_conv_wgrad(gmf_handle* h, const int* row_ptr, const int* pairs, const int* by_off, const int* off_start, int K,
                          const int* n_out, const float* xa, int ca, const float* xb, int cb, const float* dy, int cout, float* dW,
                          gmf_stream_t stream);

/* Weight gradient of gmf_sparse_conv_narrow (FCGF's conv1), fp32: dW [K, cin, cout] as gmf_sparse_conv_wgrad defines it, for
 * cin 1..8 and cout 1..64 over a map of gmf_sparse_build_plan (all four map arrays; the identity map has no narrow form).  One
 * wave per chunk walks the offset-major list with lane = output channel, cin accumulators per lane, dy rows read coalesced and
 * the input values broadcast.  Sum order: each offset's pair list is cut into chunks of P = max(64, ceil(nnz / 2048)) pairs over
 * S = K + 2048 slots; inside a chunk, with G = 1, 2, 4 lane groups for cout > 32, > 16, <= 16, group g adds pairs g, g + G, .. as
 * one fma chain in pair order and the groups are added in group order; an offset's chunks are added in chunk order by a second
 * pass.  The order depends only on the map, K and cout: bitwise repeatable, no float atomics; 0 for an offset without pairs.
 * Workspace: S x cin x cout + K + 2 floats.  No host synchronisation. */
int gmf_sparse_conv_narrow_wgrad(gmf_handle* h, const int* row_ptr, const int* pairs, const int* by_off, const int* off_start, int K,
                                 const int* n_out, const float* x, int cin, const float* dy, int cout, float* dW,
                                 gmf_stream_t stream);

/* FCGF's row normalisation (model/resunet.py:647-648) and its backward on x [rows, C], fp32, C 1..4096.  backward == 0: nrm[r] =
 * sqrt(sum_c x_c^2), out[r] = x[r] / (nrm[r] + 1e-8).  backward != 0: out = dx = dy / s - x <x, dy> / (nrm s^2), s = nrm + 1e-8,
 * from the forward's x and nrm.  A row with nrm == 0 gets a zero row in either direction.  (gmf_normalize_rows is F.normalize's
 * x / max(||x||, 1e-12): another function.)  One wave per row; no workspace, no host synchronisation. */
int gmf_rownorm_eps(gmf_handle* h, int backward, const float* x, const float* dy, float* nrm, float* out, long long rows, int C,
                    gmf_stream_t stream);

/* FCGF's hardest-contrastive loss with the random draws as arguments.  F0 [N0, C], F1 [N1, C] fp32 (C 1..64); pairs [K, 2] int64
 * rows (i, j) into F0 / F1; keys [K] int64: i + j max(N0, N1) of all K pairs, sorted ascending; pos_sel [P] int64 indices into
 * pairs (NULL: all pairs, P = K); sel0 [H0], sel1 [H1] int64 candidate-negative rows of F0 / F1.  For every sampled pair k = (i, j):
 *   h01[k] = the row s of sel1 with the smallest sum_c (F0[i] - F1[s])^2 (one fp32 fma chain over c; equal scores: the first
 *   position in sel1), D01[k] = sqrt(that sum + 1e-7), keep0[k] = (i, h01[k]) is not among the K pairs (binary search in keys);
 *   h10 / D10 / keep1 likewise over sel0 against F1[j], the pair tested being (h10[k], j).
 *   terms [3, P] = relu(sum_c (F0[i] - F1[j])^2 - pos_thresh), keep0 relu(neg_thresh - D01)^2, keep1 relu(neg_thresh - D10)^2.
 * out [4] = (pos_loss = mean of terms[0], neg_loss = (mean over keep0 of terms[1] + mean over keep1 of terms[2]) / 2 with a mean
 * over no rows 0, the count of keep0, the count of keep1).  Sums: thread-strided over k, then a fixed tree - bitwise repeatable.
 * An index outside its tensor sets GMF_STATUS_LOSS_INDEX and is read as 0.  No workspace, no host synchronisation. */
int gmf_hardest_contrastive_forward(gmf_handle* h, const float* F0, long long N0, const float* F1, long long N1, int C,
                                    const long long* pairs, long long K, const long long* keys, const long long* pos_sel, long long P,
                                    const long long* sel0, long long H0, const long long* sel1, long long H1, float pos_thresh,
                                    float neg_thresh, long long* h01, long long* h10, unsigned char* keep0, unsigned char* keep1,
                                    float* D01, float* D10, float* terms, float* out, gmf_stream_t stream);
/* Backward of gmf_hardest_contrastive_forward from its outputs, first half: g_pos / g_neg (device scalars) are the gradients of
 * pos_loss / neg_loss.  rows0 [3P, C] with dest0 [3P] int64 are the gradient rows into F0 and their rows: 3k the positive term
 * -> i_k, 3k + 1 the negative term of side 0 -> i_k, 3k + 2 the negative term of side 1 -> h10[k]; rows1 / dest1 into F1 (-> j_k,
 * j_k, h01[k]).  An inactive hinge or a dropped row writes zeros.  gmf_rows_sum_by_dest adds them per destination row. */
int gmf_hardest_contrastive_backward(gmf_handle* h, const float* F0, long long N0, const float* F1, long long N1, int C,
                                     const long long* pairs, long long K, const long long* pos_sel, long long P, const long long* h01,
                                     const long long* h10, const unsigned char* keep0, const unsigned char* keep1, const float* D01,
                                     const float* D10, const float* terms, const float* out, float neg_thresh, const float* g_pos,
                                     const float* g_neg, float* rows0, long long* dest0, float* rows1, long long* dest1,
                                     gmf_stream_t stream);
/* out [N, C] (C 1..64): out[r] = sum over e in [row_start[r], row_start[r + 1]) of rows[order[e]], added in that order; rows
 * [E, C], order [E] and row_start [N + 1] int64 - a CSR by destination row (a stable sort of the destinations gives a fixed order:
 * bitwise repeatable, no float atomics).  A row without entries gets zeros. */
int gmf_rows_sum_by_dest(gmf_handle* h, const float* rows, long long E, const long long* order, const long long* row_start,
                         long long N, int C, float* out, gmf_stream_t stream);

/* MinkowskiBatchNorm in TRAINING mode (nn.BatchNorm1d over the valid rows of all batches) on a sparse level: x [cap, C] row-major,
 * *n_rows (device pointer, a plan's level count) valid rows first.  y = gamma (x - mean) rstd + beta, + residual [cap, C] (may be
 * NULL), then max(., 0) if relu - plain bn, relu(bn) and the residual block's tail relu(bn(x) + residual); rows >= *n_rows of y are
 * written as 0.  mean / rstd [C] (biased variance) are returned for the backward; running_mean / running_var (both or neither)
 * are updated as torch does: r = (1 - momentum) r + momentum v, the variance unbiased over the valid count.  Fewer than 2 valid
 * rows sets GMF_STATUS_BATCHNORM_ROWS and leaves the running statistics alone.  Column sums run over min(64, ceil(cap / 256))
 * fixed row chunks of the cap slots (4 row lanes per column added in order, chunks added in order), the variance as a second
 * pass over the centred rows.  Workspace 2 x chunks x C floats.  No host synchronisation. */
int gmf_batchnorm_masked_forward(gmf_handle* h, const float* x, const float* residual, const float* gamma, const float* beta,
                                 const int* n_rows, long long cap, int C, float eps, float momentum, int relu, float* y, float* mean,
                                 float* rstd, float* running_mean, float* running_var, gmf_stream_t stream);
/* Backward of gmf_batchnorm_masked_forward: g = dy on valid rows (and where y_relu > 0 when the forward applied the ReLU; y_relu
 * is then its output, else NULL), 0 elsewhere, written for all cap rows - the upstream gradient of the residual branch; dbeta =
 * sum g, dgamma = sum g xhat (the forward's chunk order); dx = gamma rstd (g - dbeta / n - xhat dgamma / n) on valid rows, 0
 * beyond. */
int gmf_batchnorm_masked_backward(gmf_handle* h, const float* dy, const float* x, const float* y_relu, const float* mean,
                                  const float* rstd, const float* gamma, const int* n_rows, long long cap, int C, float* g, float* dx,
                                  float* dgamma, float* dbeta, gmf_stream_t stream);

/* ---- validation step: the non-test forward's similarity matrix and the metrics of libs/trainer.py:194-262 ---------- */

/* M = clamp(1 - (1 - Fn Fn^T) / sigma^2, 0, 1) with a zero diagonal (GMF_PointDSC/models/PointDSC.py:231-234):
 * feat_n [B,N,128] unit rows -> M [B,N,N] with row stride ldm >= N floats (element (b,i,j) at M[(b*N + i)*ldm + j];
 * the padding columns are not written).  Split-fp16 MFMA product, fp32 accumulate; writing M is the bound, and a row
 * stride that is a multiple of 32 floats (whole 128-byte lines per row piece) nearly doubles the store rate. */
int gmf_similarity_matrix(gmf_handle* h, const float* feat_n, int B, int N, float sigma, float* M, int ldm,
                          gmf_stream_t stream);

/* SpectralMatchingLoss.forward(M, gt_labels) (GMF_PointDSC/libs/loss.py:116-140): M [B,N,N] with row stride ldm,
 * gt_labels [B,N] float 0/1 -> loss_out [1] (device).  balanced != 0 is the reference's default form. */
int gmf_spectral_matching_loss(gmf_handle* h, const float* M, int ldm, const float* gt_labels, int B, int N, int balanced,
                               float* loss_out, gmf_stream_t stream);

/* The same loss straight from the features: gmf_similarity_matrix followed by gmf_spectral_matching_loss without M
 * ever reaching memory (upper triangle of tiles only, reduced on the fly). */
int gmf_spectral_matching_loss_fused(gmf_handle* h, const float* feat_n, const float* gt_labels, int B, int N, float sigma,
                                     int balanced, float* loss_out, gmf_stream_t stream);

/* Backward of gmf_spectral_matching_loss_fused (first slice of the training path, libs/trainer.py:158): the gradient of
 * SpectralMatchingLoss(M(feat_n, sigma), gt_labels) (PointDSC.py:231-234, libs/loss.py:116-140) for an upstream gradient
 * of 1, with respect to feat_n -> d_feat_n [B,N,128] and to the bandwidth sigma -> d_sigma [1] (both device, fp32).  M and
 * dL/dM are never written: S = Fn Fn^T tile by tile, dL/dFn = 2 G Fn with G = dL/dM * [0 <= u <= 1] / sigma^2 (clamp's
 * gradient mask), split-fp16 MFMA products with fp32 accumulation, dsigma summed in fp64 in a fixed order. */
int gmf_spectral_matching_backward(gmf_handle* h, const float* feat_n, const float* gt_labels, int B, int N, float sigma,
                                   int balanced, float* d_feat_n, float* d_sigma, gmf_stream_t stream);

/* ClassificationLoss.forward(pred, gt, weight) (GMF_PointDSC/libs/loss.py:67-113): pred [B,N] logits, gt [B,N] float
 * 0/1, weight [B,N] or NULL -> out [6] (device) = loss, precision, recall, f1 (pair 0, as loss.py:99-101), mean logit of
 * the inliers, mean logit of the outliers. */
int gmf_classification_loss(gmf_handle* h, const float* pred, const float* gt, const float* weight, int B, int N,
                            int balanced, float* out6, gmf_stream_t stream);

/* TransformationLoss.forward(trans, gt_trans, src_keypts, tgt_keypts, probs) (GMF_PointDSC/libs/loss.py:12-64):
 * trans, gt_trans [B,4,4]; src_keypts, tgt_keypts [B,N,3]; probs [B,N] -> out [5] (device) = loss, recall (%), RE (deg),
 * TE (cm), RMSE.  As the reference, pair i's warped source points are compared with the target points of every pair of
 * the batch (loss.py:47-48,61 broadcast [N,3] against [bs,N,3]). */
int gmf_transformation_loss(gmf_handle* h, const float* trans, const float* gt_trans, const float* src_keypts,
                            const float* tgt_keypts, const float* probs, int B, int N, float re_thre, float te_thre,
                            float* out5, gmf_stream_t stream);

/* ---- training primitives (row f-4) -----------------------------------------------------------------------------------
 * What the training forward + backward of the encoder are made of (FusionLayer / PerceiverIO fusion_layer.py:32-128,172-201;
 * PointCN, NonLocalBlock and classifier PointDSC.py:10-74,104-109,175-181 with TRAIN-mode BatchNorm; the two losses the
 * reference trains with by default, libs/loss.py:67-140, config_3DMatch.py:50-52), on plain row-major fp32 tensors;
 * gmf_amd/train.py composes them into torch.autograd.Functions.  Contractions run on the fp32 MFMA (exact
 * fp32 products; gradients of magnitude 1e-8 need no operand scaling), every cross-row sum is taken in a fixed order. */

/* C[b] = alpha * op(A[b]) op(B[b]) (+ bias[col]) (+ residual[b]) (-> ReLU if relu != 0) for b < batch; op(X) = X^T when trans_x != 0.  op(A) is
 * M x K, op(B) is K x N; lda / ldb / ldc are row strides and stride_* batch strides, in floats (residual shares C's layout).
 * Few output tiles with a long contraction (weight gradients: K = every row of the batch) are split over K into partials
 * that are added in index order. */
int gmf_gemm_f32(gmf_handle* h, int trans_a, int trans_b, const float* A, const float* B, float* C, const float* bias,
                 const float* residual, int M, int N, int K, long long lda, long long ldb, long long ldc, long long stride_a,
                 long long stride_b, long long stride_c, int batch, float alpha, int relu, gmf_stream_t stream);
/* LCPE (fusion_layer.py:118-128) on x [rows, C] = sequences of L rows: forward y = x + bias + depthwise conv3(x) with taps
 * w [C,1,3]; backward (x := dy, y := dx, bias unused) the transposed taps: dx[l] = dy[l] (1 + w1) + w0 dy[l+1] + w2 dy[l-1]. */
int gmf_lcpe(gmf_handle* h, int backward, const float* x, const float* w, const float* bias, float* y, int rows, int L, int C,
             gmf_stream_t stream);
/* nn.LayerNorm over the last dim (eps 1e-5): y, and mean / rstd [rows] for the backward.  Backward: dx = the input gradient
 * (+ dx_add when non-NULL: the residual branch's gradient). */
int gmf_layernorm_forward(gmf_handle* h, const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                          long long rows, int C, gmf_stream_t stream);
int gmf_layernorm_backward(gmf_handle* h, const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                           const float* dx_add, float* dx, long long rows, int C, gmf_stream_t stream);
/* forward: out = softmax(mul * scale * a) per row of length T (mul: optional element-wise multiplier of the logits, the
 * compat matrix of the spatial-consistency attention, PointDSC.py:60-62); backward: a = P, b = dP -> out = dS =
 * scale * mul * P * (dP - <dP, P>). */
int gmf_softmax_rows(gmf_handle* h, int backward, const float* a, const float* b, const float* mul, float* out, long long rows, int T,
                     float scale, gmf_stream_t stream);
/* GEGLU (fusion_layer.py:54-57): hdn [rows, 2H] -> out [rows, H] = x * gelu_erf(gates); backward: dg [rows, H] -> out = dhdn [rows, 2H]. */
int gmf_geglu(gmf_handle* h, int backward, const float* hdn, const float* dg, float* out, long long rows, int H,
              gmf_stream_t stream);
/* out[c] = sum over rows r of x'[r][c] * y'[r + shift][c] with y' = 1 (y NULL), y, (y - mean[r]) * rstd[r] (LayerNorm's xhat)
 * or (y - cmean[c]) * crstd[c] (BatchNorm's; crstd NULL = 1), x' = x or x - cmean[c] (center_x); rows r + shift outside r's
 * sequence of L rows contribute 0.  Bias, LayerNorm / BatchNorm parameter and LCPE-tap gradients, BatchNorm statistics.
 * relu_y (optional): x is first masked by the saved output of a ReLU (x where relu_y > 0, else 0).  dual != 0 (needs y): out
 * holds 2C values, [sum x' y' | sum x'] - a normalisation's dgamma and dbeta, or an LCPE tap and its bias, in one pass. */
int gmf_colsum(gmf_handle* h, const float* x, const float* y, const float* mean, const float* rstd, const float* cmean,
               const float* crstd, int center_x, int shift, int L, long long rows, int C, const float* relu_y, int dual, float* out,
               gmf_stream_t stream);
/* nn.BatchNorm1d in TRAINING mode over the rows of x [rows, C] (= BatchNorm1d on [B, C, N]): batch statistics (mean / rstd [C]
 * returned for the backward), running statistics updated as torch does (momentum, unbiased variance; may be NULL), optional
 * fused ReLU.  Backward: dx, dgamma, dbeta; y_relu (the saved output) masks dy when the forward applied the ReLU, else NULL. */
int gmf_batchnorm_train_forward(gmf_handle* h, const float* x, const float* gamma, const float* beta, float* y, float* mean,
                                float* rstd, float* running_mean, float* running_var, long long rows, int C, float eps,
                                float momentum, int relu, gmf_stream_t stream);
int gmf_batchnorm_train_backward(gmf_handle* h, const float* dy, const float* x, const float* y_relu, const float* mean,
                                 const float* rstd, const float* gamma, float* dx, float* dgamma, float* dbeta, long long rows, int C,
                                 gmf_stream_t stream);
/* F.normalize(x, p=2, dim=-1) (PointDSC.py:229) on rows [rows, C]: forward a = x -> out = y, nrm [rows] = max(||x||, 1e-12);
 * backward a = y (the saved output), dy, nrm -> out = dx = (dy - y <dy, y>) / nrm. */
int gmf_normalize_rows(gmf_handle* h, int backward, const float* a, const float* dy, float* nrm, float* out, long long rows, int C,
                       gmf_stream_t stream);
/* out = y > 0 ? dy : 0 (ReLU backward from the saved output). */
int gmf_relu_backward(gmf_handle* h, const float* dy, const float* y, float* out, long long total, gmf_stream_t stream);
/* d loss / d pred of ClassificationLoss (libs/loss.py:67-93) for an upstream gradient of 1: mean BCE-with-logits, balanced
 * (pos_weight = num_neg / num_pos over the batch) or not, or weighted per element (weight non-NULL). */
int gmf_classification_backward(gmf_handle* h, const float* pred, const float* gt, const float* weight, int B, int N, int balanced,
                                float* d_pred, gmf_stream_t stream);
/* dL/dM [B,N,N] (dense) of SpectralMatchingLoss(M, gt_labels) (libs/loss.py:116-140), M with row stride ldm. */
int gmf_spectral_matching_dense_backward(gmf_handle* h, const float* M, int ldm, const float* gt_labels, int B, int N, int balanced,
                                         float* dM, gmf_stream_t stream);
/* Backward of gmf_similarity_matrix for an arbitrary upstream dM [B,N,N] (dense): d_feat_n [B,N,128] and d_sigma [1]
 * (PointDSC.py:231-234: matmul, clamp with its gradient mask, zero diagonal).  S and G are materialised in the workspace
 * (training sizes: N ~ 1000); the loss-specific fused form without them is gmf_spectral_matching_backward. */
int gmf_similarity_backward(gmf_handle* h, const float* feat_n, const float* dM, int B, int N, float sigma, float* d_feat_n,
                            float* d_sigma, gmf_stream_t stream);
/* Dense compat matrix [B,N,N] row-major, c_ij = clamp(1 - (|p_i-p_j| - |q_i-q_j|)^2 / sigma_d^2, min=0) (PointDSC.py:216-221;
 * the trainable path materialises it as the reference does; the inference path streams it in kernel order instead). */
int gmf_compat_dense(gmf_handle* h, const float* src_keypts, const float* tgt_keypts, int B, int N, float sigma_d, float* out,
                     gmf_stream_t stream);
/* d loss / d trans [B,4,4] of TransformationLoss (libs/loss.py:35-64) for an upstream gradient of 1:
 * loss = (1/B) sum_i [any(probs_i > 0)] mean_{b,n} |R_i p_in + t_i - q_bn|^2 (the reference's broadcast over the batch). */
int gmf_transformation_loss_backward(gmf_handle* h, const float* trans, const float* src_keypts, const float* tgt_keypts,
                                     const float* probs, int B, int N, float* d_trans, gmf_stream_t stream);
/* Backward of gmf_pose_head in train mode (use_nms = 0, refine_iters = 0; PointDSC.py:246,252,330-425): final_trans is the
 * hypothesis of the best seed of each pair, so d_final_trans [B,4,4] flows through that seed's weighted Kabsch solve
 * (closed-form derivative of the 3x3 SVD), its weights, the power iterations in reverse and the feature compatibility
 * matrix to the k neighbour rows of feat_n and to sigma.  knn_idx [B,S,k] and fitness [B,S] are gmf_pose_head's outputs for
 * the same inputs.  d_feat_n [B,N,128] is written whole (zero outside the neighbour rows), d_sigma [B] per pair. */
int gmf_pose_head_backward(gmf_handle* h, const gmf_pose_params* p, const float* feat_n, const float* src_keypts,
                           const float* tgt_keypts, const int* knn_idx, const float* fitness, const float* d_final_trans, int B,
                           int N, float* d_feat_n, float* d_sigma, gmf_stream_t stream);
/* Backward of gmf_weighted_procrustes with respect to the weights (DGR trains its inlier network through this solve,
 * core/trainer.py:594-614; X and Y carry no gradient there): d_R [B,3,3], d_t [B,3] -> d_w (ragged like w). */
int gmf_weighted_procrustes_backward(gmf_handle* h, const float* X, const float* Y, const float* w, const int* offsets, int B,
                                     float eps, const float* d_R, const float* d_t, float* d_w, gmf_stream_t stream);

/* ---- training of the image encoder (ResNet-34 -> layer2 in train(), GMF_PointDSC/models/resnet.py:36-75,195-216) -------
 * Dense NHWC fp32 activations [B,H,W,C] (= rows x channels matrices: BatchNorm, ReLU and the column sums above apply as they
 * are), weights as the nn.Conv2d parameter [cout,cin,ksize,ksize] fp32, pad = ksize / 2, no bias.  Supported
 * (cin, cout, ksize, stride): (3,64,7,2) the stem, (64,64,3,1), (128,128,3,1), (64,128,3,2), (64,128,1,2).  All three passes
 * contract on the fp32 MFMA; every sum has a fixed order (no float atomics): equal inputs give equal bits. */

/* y [B,Ho,Wo,cout] = conv(x, w), Ho = (H + 2 pad - ksize) / stride + 1.  x is read through its element strides (sb, sc, sh, sw):
 * dense NHWC for the four layer shapes; any non-negative strides (NCHW as the reference passes images) for the stem. */
int gmf_conv2d_forward_f32(gmf_handle* h, const float* x, long long sb, long long sc, long long sh, long long sw, const float* w,
                           float* y, int B, int H, int W, int cin, int cout, int ksize, int stride, gmf_stream_t stream);
/* dx [B,H,W,cin] = the input gradient of that convolution for dy [B,Ho,Wo,cout] (+ dx_add when non-NULL: the residual
 * branch's gradient); a gather, every entry written (0 where no output pixel reads the input pixel).  Not for the stem. */
int gmf_conv2d_dgrad(gmf_handle* h, const float* dy, const float* w, const float* dx_add, float* dx, int B, int H, int W, int cin,
                     int cout, int ksize, int stride, gmf_stream_t stream);
/* dw [cout,cin,ksize,ksize] = sum over output pixels of dy[p][co] x[p stride + k - pad][ci]; the pixel range is split over
 * workgroups into workspace slabs that are added in index order.  x strides as in the forward. */
int gmf_conv2d_wgrad(gmf_handle* h, const float* x, long long sb, long long sc, long long sh, long long sw, const float* dy, float* dw,
                     int B, int H, int W, int cin, int cout, int ksize, int stride, gmf_stream_t stream);
/* nn.MaxPool2d(3, 2, 1) on NHWC (C % 4 == 0): y [B,Hp,Wp,C], Hp = (H - 1) / 2 + 1.  Backward: dx [B,H,W,C] from the saved input
 * x and dy; each window's gradient goes to its first maximum in row-major window order (torch's rule). */
int gmf_maxpool3x3s2_forward(gmf_handle* h, const float* x, float* y, int B, int H, int W, int C, gmf_stream_t stream);
int gmf_maxpool3x3s2_backward(gmf_handle* h, const float* x, const float* dy, float* dx, int B, int H, int W, int C,
                              gmf_stream_t stream);
/* gmf_batchnorm_train_forward with the BasicBlock's identity branch: y = relu?(bn(x) + residual), residual [rows, C].  The
 * backward is gmf_batchnorm_train_backward (y_relu = this y) for x and gmf_relu_backward(dy, y) for the residual. */
int gmf_batchnorm_residual_forward(gmf_handle* h, const float* x, const float* residual, const float* gamma, const float* beta,
                                   float* y, float* mean, float* rstd, float* running_mean, float* running_var, long long rows, int C,
                                   float eps, float momentum, int relu, gmf_stream_t stream);

/* ---- image encoder epilogue (ResNet BasicBlock, GMF_PointDSC/models/resnet.py:59-75) ------------------------------- */

/* y = max(y + bias[c] (+ residual), 0) in place on an NHWC fp32 tensor of n_pixels x C (C % 4 == 0): the folded
 * BatchNorm bias, the residual add and the ReLU that follow each MIOpen convolution, in one pass.  residual may be NULL. */
int gmf_bias_relu_nhwc(gmf_handle* h, float* y, const float* bias, const float* residual, long long n_pixels, int C,
                       gmf_stream_t stream);

/* The ResNet stem in one kernel (GMF_PointDSC/models/resnet.py:198-204): conv1 7x7 stride 2 pad 3 (3 -> 64 channels) with
 * the BatchNorm folded in, ReLU and max-pool 3x3 stride 2 pad 1.  x [B,3,H,W] fp32 with element strides (sb, sc, sh, sw) -
 * NCHW as the reference passes it, or any view; y [B,Hp,Wp,64] NHWC fp32 with Hc = (H-1)/2+1, Hp = (Hc-1)/2+1 (same for W).
 * wimg: the folded weights as a split-fp16 image of 256 W (gmf_amd/packing.py: stem_image), bias [64].  Implicit GEMM on the
 * f16 MFMA with split-fp16 operands, fp32 accumulate; the pooled tile is written once. */
int gmf_stem_forward(gmf_handle* h, const float* x, long long sb, long long sc, long long sh, long long sw, const float* wimg,
                     const float* bias, float* y, int B, int H, int W, gmf_stream_t stream);

/* Convolution of the ResNet-34 layer1 / layer2 shapes (GMF_PointDSC/models/resnet.py:36-75, 144-170) as an implicit GEMM on
 * the f16 MFMA with split-fp16 operands: x [B,H,W,cin] NHWC fp32 -> y [B,Ho,Wo,cout] NHWC fp32 (pad = ksize / 2),
 *   y = conv(x, W) + bias (+ residual [B,Ho,Wo,cout]) -> ReLU if relu != 0.
 * wimg: the BatchNorm-folded weights as a split-fp16 image of 256 W (gmf_amd/packing.py: conv_image(W, stride); k order
 * (channel block, tap) for the stride-1 3x3 shapes, (tap, channel block) for the others).  Supported:
 * (cin, cout, ksize, stride) = (64,64,3,1), (64,128,3,2), (128,128,3,1), (64,128,1,2). */
int gmf_conv_nhwc(gmf_handle* h, const float* x, const float* wimg, const float* bias, const float* residual, float* y,
                  int B, int H, int W, int cin, int cout, int ksize, int stride, int relu, gmf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GMF_HIP_H_ */
