// C ABI, training primitives (include/gmf_hip.h, section "training primitives"): argument checks and the split-K / column-sum
// workspaces around the kernels of train_kernels.hip.  Kept apart from gmf_api.cpp so that the inference launch sequences
// (and the source hash bench.py ties its profile to) do not move when the training path grows.
#include "api_common.hpp"
#include "launchers_pose.hpp"
#include "launchers_sparse.hpp"
#include "launchers_sparse_train.hpp"
#include "launchers_image_train.hpp"

extern "C" {

int gmf_gemm_f32(gmf_handle* h, int trans_a, int trans_b, const float* A, const float* B, float* C, const float* bias,
                 const float* residual, int M, int N, int K, long long lda, long long ldb, long long ldc, long long stride_a,
                 long long stride_b, long long stride_c, int batch, float alpha, int relu, gmf_stream_t stream) {
  GMF_REQUIRE(h && A && B && C, GMF_ERR_BAD_ARG, "gemm_f32: null pointer");
  GMF_REQUIRE(M > 0 && N > 0 && K > 0 && batch > 0, GMF_ERR_UNSUPPORTED_SHAPE, "gemm_f32: empty problem");
  // leading dimensions: a row of op(X) as it is stored must fit its stride (a smaller one reads or writes out of bounds on the device)
  GMF_REQUIRE(lda >= (trans_a ? M : K) && ldb >= (trans_b ? K : N) && ldc >= N, GMF_ERR_BAD_ARG,
              "gemm_f32: need lda >= (trans_a ? M : K), ldb >= (trans_b ? K : N), ldc >= N (row strides in floats)");
  GMF_REQUIRE(batch == 1 || (stride_a >= 0 && stride_b >= 0 && stride_c >= N), GMF_ERR_BAD_ARG,
              "gemm_f32: batched outputs overlap (stride_c < N) or a batch stride is negative");
  // grid limits: blockIdx.y = ceil(M / 64) at most, blockIdx.z = batch * ksplits (ksplits <= 128)
  GMF_REQUIRE((M + 63) / 64 <= 65535, GMF_ERR_UNSUPPORTED_SHAPE, "gemm_f32: M too large for one launch (ceil(M / 64) > 65535)");
  SetDevice sd(h, stream);
  const int ksplits = gmf::gemm_ksplits(trans_a != 0, trans_b != 0, A, B, M, N, K, (long)lda, (long)ldb, (long)stride_a, (long)stride_b, batch);
  GMF_REQUIRE((long long)batch * ksplits <= 65535, GMF_ERR_UNSUPPORTED_SHAPE, "gemm_f32: batch * k-splits exceeds 65535 workgroups in z: split the batch");
  float* part;          // split-K partials
  if (int rc = arena_carve(h, {arena_buf(part, ksplits > 1 ? (size_t)batch * ksplits * M * N : 0)})) return rc;
  GMF_HIP(gmf::launch_gemm_f32(trans_a != 0, trans_b != 0, A, B, C, bias, residual, M, N, K, (long)lda, (long)ldb, (long)ldc,
                               (long)stride_a, (long)stride_b, (long)stride_c, batch, alpha, part, ksplits, relu ? 1 : 0, S(stream)));
  return GMF_OK;
}

int gmf_lcpe(gmf_handle* h, int backward, const float* x, const float* w, const float* bias, float* y, int rows, int L, int C,
             gmf_stream_t stream) {
  GMF_REQUIRE(h && x && w && y && (backward || bias), GMF_ERR_BAD_ARG, "lcpe: null pointer");
  GMF_REQUIRE(rows > 0 && L > 0 && C > 0 && rows % L == 0, GMF_ERR_UNSUPPORTED_SHAPE, "lcpe: rows must be a positive multiple of L");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_lcpe(backward != 0, x, w, bias, y, rows, L, C, S(stream)));
  return GMF_OK;
}

int gmf_layernorm_forward(gmf_handle* h, const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                          long long rows, int C, gmf_stream_t stream) {
  GMF_REQUIRE(h && x && gamma && beta && y && mean && rstd, GMF_ERR_BAD_ARG, "layernorm_forward: null pointer");
  GMF_REQUIRE(rows > 0 && C > 0, GMF_ERR_UNSUPPORTED_SHAPE, "layernorm_forward: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_ln_fwd(x, gamma, beta, y, mean, rstd, (long)rows, C, S(stream)));
  return GMF_OK;
}

int gmf_layernorm_backward(gmf_handle* h, const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                           const float* dx_add, float* dx, long long rows, int C, gmf_stream_t stream) {
  GMF_REQUIRE(h && dy && x && gamma && mean && rstd && dx, GMF_ERR_BAD_ARG, "layernorm_backward: null pointer");
  GMF_REQUIRE(rows > 0 && C > 0, GMF_ERR_UNSUPPORTED_SHAPE, "layernorm_backward: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_ln_bwd(dy, x, gamma, mean, rstd, dx_add, dx, (long)rows, C, S(stream)));
  return GMF_OK;
}

int gmf_softmax_rows(gmf_handle* h, int backward, const float* a, const float* b, const float* mul, float* out, long long rows, int T,
                     float scale, gmf_stream_t stream) {
  GMF_REQUIRE(h && a && out && (!backward || b), GMF_ERR_BAD_ARG, "softmax_rows: null pointer");
  GMF_REQUIRE(rows > 0 && T > 0, GMF_ERR_UNSUPPORTED_SHAPE, "softmax_rows: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_softmax(backward != 0, a, b, mul, out, (long)rows, T, scale, S(stream)));
  return GMF_OK;
}

int gmf_geglu(gmf_handle* h, int backward, const float* hdn, const float* dg, float* out, long long rows, int H,
              gmf_stream_t stream) {
  GMF_REQUIRE(h && hdn && out && (!backward || dg), GMF_ERR_BAD_ARG, "geglu: null pointer");
  GMF_REQUIRE(rows > 0 && H > 0, GMF_ERR_UNSUPPORTED_SHAPE, "geglu: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_geglu(backward != 0, hdn, dg, out, (long)rows, H, S(stream)));
  return GMF_OK;
}

int gmf_colsum(gmf_handle* h, const float* x, const float* y, const float* mean, const float* rstd, const float* cmean,
               const float* crstd, int center_x, int shift, int L, long long rows, int C, const float* relu_y, int dual, float* out,
               gmf_stream_t stream) {
  GMF_REQUIRE(h && x && out, GMF_ERR_BAD_ARG, "colsum: null pointer");
  GMF_REQUIRE((mean == nullptr) == (rstd == nullptr) && (!mean || y), GMF_ERR_BAD_ARG, "colsum: mean and rstd come together, with y");
  GMF_REQUIRE(rows > 0 && C > 0 && L > 0 && rows % L == 0, GMF_ERR_UNSUPPORTED_SHAPE, "colsum: rows must be a positive multiple of L");
  GMF_REQUIRE(shift >= -1 && shift <= 1, GMF_ERR_BAD_ARG, "colsum: shift must be -1, 0 or 1");
  SetDevice sd(h, stream);
  GMF_REQUIRE(!dual || y, GMF_ERR_BAD_ARG, "colsum: dual needs y (without y both sums are the same)");
  const size_t n_part = (size_t)gmf::colsum_chunks((long)rows) * C * (dual ? 2 : 1);
  float* part;
  if (int rc = arena_carve(h, {arena_buf(part, n_part)})) return rc;
  GMF_REQUIRE(!center_x || cmean, GMF_ERR_BAD_ARG, "colsum: center_x needs cmean");
  GMF_HIP(gmf::launch_colsum(x, y, mean, rstd, cmean, crstd, center_x ? 1 : 0, shift, L, (long)rows, C, part, out, S(stream), relu_y,
                             dual != 0));
  return GMF_OK;
}

// Dense train-mode BatchNorm, both exported forms: y = relu?(bn(x) (+ residual)); `who` prefixes the messages.
static int bn_dense_forward(gmf_handle* h, const char* who, const float* x, const float* residual, const float* gamma, const float* beta,
                            float* y, float* mean, float* rstd, float* running_mean, float* running_var, long long rows, int C,
                            float eps, float momentum, int relu, gmf_stream_t stream) {
  GMF_REQUIRE(h && x && gamma && beta && y && mean && rstd, GMF_ERR_BAD_ARG, std::string(who) + ": null pointer");
  GMF_REQUIRE((running_mean == nullptr) == (running_var == nullptr), GMF_ERR_BAD_ARG, std::string(who) + ": running stats come together");
  GMF_REQUIRE(rows > 1 && C > 0, GMF_ERR_UNSUPPORTED_SHAPE, std::string(who) + ": need more than one row");
  SetDevice sd(h, stream);
  const size_t n_part = (size_t)gmf::colsum_chunks((long)rows) * C;
  float *part, *sum, *sumsq;
  if (int rc = arena_carve(h, {arena_buf(part, n_part), arena_buf(sum, (size_t)C), arena_buf(sumsq, (size_t)C)})) return rc;
  hipStream_t st = S(stream);
  GMF_HIP(gmf::launch_colsum(x, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, (int)rows, (long)rows, C, part, sum, st));
  GMF_HIP(gmf::launch_bn_finish(sum, nullptr, mean, rstd, nullptr, nullptr, C, (long)rows, eps, momentum, st));
  // sum of squared deviations: x' = x - mean (centred), y' = (x - mean) * 1
  GMF_HIP(gmf::launch_colsum(x, x, nullptr, nullptr, mean, nullptr, 1, 0, (int)rows, (long)rows, C, part, sumsq, st));
  GMF_HIP(gmf::launch_bn_finish(sum, sumsq, mean, rstd, running_mean, running_var, C, (long)rows, eps, momentum, st));
  GMF_HIP(gmf::launch_bn_apply(x, mean, rstd, gamma, beta, y, (long)rows, C, relu ? 1 : 0, residual, st));
  return GMF_OK;
}

int gmf_batchnorm_train_forward(gmf_handle* h, const float* x, const float* gamma, const float* beta, float* y, float* mean,
                                float* rstd, float* running_mean, float* running_var, long long rows, int C, float eps,
                                float momentum, int relu, gmf_stream_t stream) {
  return bn_dense_forward(h, "batchnorm_train_forward", x, nullptr, gamma, beta, y, mean, rstd, running_mean, running_var, rows, C, eps,
                          momentum, relu, stream);
}

int gmf_batchnorm_train_backward(gmf_handle* h, const float* dy, const float* x, const float* y_relu, const float* mean,
                                 const float* rstd, const float* gamma, float* dx, float* dgamma, float* dbeta, long long rows, int C,
                                 gmf_stream_t stream) {
  GMF_REQUIRE(h && dy && x && mean && rstd && gamma && dx && dgamma && dbeta, GMF_ERR_BAD_ARG, "batchnorm_train_backward: null pointer");
  GMF_REQUIRE(rows > 1 && C > 0, GMF_ERR_UNSUPPORTED_SHAPE, "batchnorm_train_backward: need more than one row");
  SetDevice sd(h, stream);
  const size_t n_part = (size_t)gmf::colsum_chunks((long)rows) * C * 2;
  float* part;
  if (int rc = arena_carve(h, {arena_buf(part, n_part)})) return rc;
  hipStream_t st = S(stream);
  // ONE pass over dy: dgamma = sum g xhat, dbeta = sum g, with g = dy masked by the output of the ReLU that followed
  GMF_HIP(gmf::launch_colsum(dy, x, nullptr, nullptr, mean, rstd, 0, 0, (int)rows, (long)rows, C, part, dgamma, st, y_relu, true, dbeta));
  GMF_HIP(gmf::launch_bn_bwd(dy, x, mean, rstd, gamma, dbeta, dgamma, dx, (long)rows, C, st, y_relu));
  return GMF_OK;
}

int gmf_normalize_rows(gmf_handle* h, int backward, const float* a, const float* dy, float* nrm, float* out, long long rows, int C,
                       gmf_stream_t stream) {
  GMF_REQUIRE(h && a && nrm && out && (!backward || dy), GMF_ERR_BAD_ARG, "normalize_rows: null pointer");
  GMF_REQUIRE(rows > 0 && C > 0, GMF_ERR_UNSUPPORTED_SHAPE, "normalize_rows: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_normalize(backward != 0, a, dy, nrm, out, (long)rows, C, S(stream)));
  return GMF_OK;
}

int gmf_relu_backward(gmf_handle* h, const float* dy, const float* y, float* out, long long total, gmf_stream_t stream) {
  GMF_REQUIRE(h && dy && y && out, GMF_ERR_BAD_ARG, "relu_backward: null pointer");
  GMF_REQUIRE(total > 0, GMF_ERR_UNSUPPORTED_SHAPE, "relu_backward: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_relu_bwd(dy, y, out, (long)total, S(stream)));
  return GMF_OK;
}

int gmf_classification_backward(gmf_handle* h, const float* pred, const float* gt, const float* weight, int B, int N, int balanced,
                                float* d_pred, gmf_stream_t stream) {
  GMF_REQUIRE(h && pred && gt && d_pred, GMF_ERR_BAD_ARG, "classification_backward: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "classification_backward: empty input");
  SetDevice sd(h, stream);
  float* pw;
  if (int rc = arena_carve(h, {arena_buf(pw, 1)})) return rc;
  GMF_HIP(gmf::launch_bce_bwd(pred, gt, weight, d_pred, pw, balanced, (long)B * N, S(stream)));
  return GMF_OK;
}

int gmf_spectral_matching_dense_backward(gmf_handle* h, const float* M, int ldm, const float* gt_labels, int B, int N, int balanced,
                                         float* dM, gmf_stream_t stream) {
  GMF_REQUIRE(h && M && gt_labels && dM, GMF_ERR_BAD_ARG, "spectral_matching_dense_backward: null pointer");
  GMF_REQUIRE(B > 0 && N > 0 && ldm >= N, GMF_ERR_UNSUPPORTED_SHAPE, "spectral_matching_dense_backward: need ldm >= N > 0");
  SetDevice sd(h, stream);
  float* consts;
  if (int rc = arena_carve(h, {arena_buf(consts, (size_t)4 * B)})) return rc;
  GMF_HIP(gmf::launch_sm_dense_bwd(M, ldm, gt_labels, consts, dM, B, N, balanced, S(stream)));
  return GMF_OK;
}

int gmf_similarity_backward(gmf_handle* h, const float* feat_n, const float* dM, int B, int N, float sigma, float* d_feat_n,
                            float* d_sigma, gmf_stream_t stream) {
  GMF_REQUIRE(h && feat_n && dM && d_feat_n && d_sigma, GMF_ERR_BAD_ARG, "similarity_backward: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "similarity_backward: empty input");
  GMF_REQUIRE(sigma != 0.f || h->sigma_dev, GMF_ERR_BAD_ARG, "similarity_backward: sigma must be non-zero");
  SetDevice sd(h, stream);
  const size_t nn = (size_t)B * N * N, rows = (size_t)B * N;
  const size_t n_part = (size_t)gmf::colsum_chunks((long)rows);
  float *Sm, *G, *rowdsig, *part;
  if (int rc = arena_carve(h, {arena_buf(Sm, nn), arena_buf(G, nn), arena_buf(rowdsig, rows), arena_buf(part, n_part)})) return rc;
  hipStream_t st = S(stream);
  const long ld = 128, sF = (long)N * 128, sN = (long)N * N;
  // S = Fn Fn^T per pair, G = dM * [0 <= u <= 1] / sigma^2, dFn = G Fn + G^T Fn, dsigma = sum of the row partials
  GMF_HIP(gmf::launch_gemm_f32(false, true, feat_n, feat_n, Sm, nullptr, nullptr, N, N, 128, ld, ld, N, sF, sF, sN, B, 1.0f, nullptr, 1, 0, st));
  GMF_HIP(gmf::launch_sim_bwd_G(Sm, dM, G, rowdsig, B, N, sigma, st, h->sigma_dev));
  GMF_HIP(gmf::launch_gemm_f32(false, false, G, feat_n, d_feat_n, nullptr, nullptr, N, 128, N, N, ld, ld, sN, sF, sF, B, 1.0f, nullptr, 1, 0, st));
  GMF_HIP(gmf::launch_gemm_f32(true, false, G, feat_n, d_feat_n, nullptr, d_feat_n, N, 128, N, N, ld, ld, sN, sF, sF, B, 1.0f, nullptr, 1, 0, st));
  GMF_HIP(gmf::launch_colsum(rowdsig, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, (int)rows, (long)rows, 1, part, d_sigma, st));
  return GMF_OK;
}

int gmf_compat_dense(gmf_handle* h, const float* src_keypts, const float* tgt_keypts, int B, int N, float sigma_d, float* out,
                     gmf_stream_t stream) {
  GMF_REQUIRE(h && src_keypts && tgt_keypts && out, GMF_ERR_BAD_ARG, "compat_dense: null pointer");
  GMF_REQUIRE(B > 0 && N > 0 && N <= 65535 && B <= 65535, GMF_ERR_UNSUPPORTED_SHAPE, "compat_dense: need 0 < B, N <= 65535");
  GMF_REQUIRE(sigma_d > 0.f, GMF_ERR_BAD_ARG, "compat_dense: sigma_d must be positive");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_compat_dense(src_keypts, tgt_keypts, out, B, N, sigma_d, S(stream)));
  return GMF_OK;
}

int gmf_transformation_loss_backward(gmf_handle* h, const float* trans, const float* src_keypts, const float* tgt_keypts,
                                     const float* probs, int B, int N, float* d_trans, gmf_stream_t stream) {
  GMF_REQUIRE(h && trans && src_keypts && tgt_keypts && probs && d_trans, GMF_ERR_BAD_ARG, "transformation_loss_backward: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "transformation_loss_backward: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_tl_backward(trans, src_keypts, tgt_keypts, probs, d_trans, B, N, S(stream)));
  return GMF_OK;
}

int gmf_pose_head_backward(gmf_handle* h, const gmf_pose_params* p, const float* feat_n, const float* src_keypts,
                           const float* tgt_keypts, const int* knn_idx, const float* fitness, const float* d_final_trans, int B,
                           int N, float* d_feat_n, float* d_sigma, gmf_stream_t stream) {
  GMF_REQUIRE(h && p && feat_n && src_keypts && tgt_keypts && knn_idx && fitness && d_final_trans && d_feat_n && d_sigma,
              GMF_ERR_BAD_ARG, "pose_head_backward: null pointer");
  const int Sn = p->num_seeds, k = p->k, iters = p->num_iterations;
  GMF_REQUIRE(B > 0 && N > 1 && Sn > 0 && Sn <= N, GMF_ERR_UNSUPPORTED_SHAPE, "pose_head_backward: need N > 1, 0 < num_seeds <= N");
  GMF_REQUIRE(k > 0 && k <= 64 && k <= N - 1, GMF_ERR_UNSUPPORTED_SHAPE, "pose_head_backward: need 0 < k <= min(64, N-1)");
  GMF_REQUIRE(iters > 0 && iters <= 64, GMF_ERR_BAD_ARG, "pose_head_backward: bad num_iterations");
  GMF_REQUIRE(p->refine_iters == 0, GMF_ERR_BAD_ARG, "pose_head_backward: the post-refinement (test mode) is not differentiable");
  GMF_REQUIRE((p->sigma > 0.f || h->sigma_dev) && p->sigma_d > 0.f, GMF_ERR_BAD_ARG, "pose_head_backward: sigma, sigma_d must be positive");
  SetDevice sd(h, stream);
  hipStream_t st = S(stream);
  const size_t BS = (size_t)B * Sn;
  float* snaps;
  unsigned char* conv;
  int* stop_it;
  if (int rc = arena_carve(h, {arena_buf(snaps, BS * iters * k), arena_buf(conv, BS * iters), arena_buf(stop_it, 1)})) return rc;
  // the forward's iterates and convergence flags of every seed (the stop iteration is a property of all seeds of a pair)
  GMF_HIP(gmf::launch_seed_power(feat_n, src_keypts, tgt_keypts, knn_idx, snaps, conv, nullptr, B, N, Sn, k, iters, p->sigma, p->sigma_d, st, nullptr, h->sigma_dev));
  GMF_HIP(hipMemsetAsync(d_feat_n, 0, (size_t)B * N * kC * sizeof(float), st));
  if (B > 1) GMF_HIP(gmf::launch_stop_iteration(conv, B, Sn, iters, stop_it, st));     // the reference's allclose spans the batch
  GMF_HIP(gmf::launch_pose_best_backward(feat_n, src_keypts, tgt_keypts, knn_idx, fitness, snaps, conv, d_final_trans, d_feat_n,
                                         d_sigma, B, N, Sn, k, iters, p->sigma, p->sigma_d, B > 1 ? stop_it : nullptr, st, h->sigma_dev));
  return GMF_OK;
}

int gmf_weighted_procrustes_backward(gmf_handle* h, const float* X, const float* Y, const float* w, const int* offsets, int B,
                                     float eps, const float* d_R, const float* d_t, float* d_w, gmf_stream_t stream) {
  GMF_REQUIRE(h && X && Y && w && offsets && d_R && d_t && d_w, GMF_ERR_BAD_ARG, "weighted_procrustes_backward: null pointer");
  GMF_REQUIRE(B > 0, GMF_ERR_UNSUPPORTED_SHAPE, "weighted_procrustes_backward: empty batch");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_wp_backward(X, Y, w, offsets, B, eps, d_R, d_t, d_w, S(stream)));
  return GMF_OK;
}

// ---- training of the sparse network -----------------------------------------------------------------------------------

int gmf_sparse_conv_wgrad(gmf_handle* h, const int* row_ptr, const int* pairs, const int* by_off, const int* off_start, int K,
                          const int* n_out, const float* xa, int ca, const float* xb, int cb, const float* dy, int cout, float* dW,
                          gmf_stream_t stream) {
  GMF_REQUIRE(h && n_out && xa && dy && dW, GMF_ERR_BAD_ARG, "sparse_conv_wgrad: null pointer");
  GMF_REQUIRE((row_ptr == nullptr) == (pairs == nullptr) && (row_ptr == nullptr) == (by_off == nullptr) &&
                  (row_ptr == nullptr) == (off_start == nullptr),
              GMF_ERR_BAD_ARG, "sparse_conv_wgrad: row_ptr, pairs, by_off and off_start go together");
  GMF_REQUIRE(K >= 1 && K <= gmf::kSparseMaxK && (row_ptr || K == 1), GMF_ERR_UNSUPPORTED_SHAPE,
              "sparse_conv_wgrad: K must be in 1..1024 (1 for the identity map)");
  GMF_REQUIRE(ca >= 1 && cb >= 0 && (cb == 0 || xb) && cout >= 1 && ca + cb <= 4096 && cout <= 4096, GMF_ERR_UNSUPPORTED_SHAPE,
              "sparse_conv_wgrad: channel counts must be in 1..4096 (cb may be 0)");
  SetDevice sd(h, stream);
  const int nslots = gmf::sparse_wgrad_slots(K);
  gmf::SparseWgradArgs a{row_ptr, reinterpret_cast<const int2*>(pairs), by_off, off_start, K, n_out, xa, ca, cb ? xb : nullptr,
                         cb, dy, cout, nslots, nullptr, nullptr, dW};
  if (int rc = arena_carve(h, {arena_buf(a.chunk_info, (size_t)K + 2), arena_buf(a.partial, (size_t)nslots * (ca + cb) * cout)}))
    return rc;
  GMF_HIP(gmf::launch_sparse_wgrad(a, S(stream)));
  return GMF_OK;
}

int gmf_sparse_conv_narrow_wgrad(gmf_handle* h, const int* row_ptr, const int* pairs, const int* by_off, const int* off_start, int K,
                                 const int* n_out, const float* x, int cin, const float* dy, int cout, float* dW,
                                 gmf_stream_t stream) {
  GMF_REQUIRE(h && row_ptr && pairs && by_off && off_start && n_out && x && dy && dW, GMF_ERR_BAD_ARG,
              "sparse_conv_narrow_wgrad: null pointer (the identity map has no narrow form)");
  GMF_REQUIRE(K >= 1 && K <= gmf::kSparseMaxK, GMF_ERR_UNSUPPORTED_SHAPE, "sparse_conv_narrow_wgrad: K must be in 1..1024");
  GMF_REQUIRE(cin >= 1 && cin <= gmf::kWgradNarrowMaxCin && cout >= 1 && cout <= gmf::kWgradNarrowMaxCout, GMF_ERR_UNSUPPORTED_SHAPE,
              "sparse_conv_narrow_wgrad: Cin must be in 1..8 and Cout in 1..64");
  SetDevice sd(h, stream);
  const int nslots = gmf::sparse_wgrad_narrow_slots(K);
  gmf::SparseWgradArgs a{row_ptr, reinterpret_cast<const int2*>(pairs), by_off, off_start, K, n_out, x, cin, nullptr, 0, dy, cout,
                         nslots, nullptr, nullptr, dW};
  if (int rc = arena_carve(h, {arena_buf(a.chunk_info, (size_t)K + 2), arena_buf(a.partial, (size_t)nslots * cin * cout)})) return rc;
  GMF_HIP(gmf::launch_sparse_wgrad_narrow(a, S(stream)));
  return GMF_OK;
}

int gmf_rownorm_eps(gmf_handle* h, int backward, const float* x, const float* dy, float* nrm, float* out, long long rows, int C,
                    gmf_stream_t stream) {
  GMF_REQUIRE(h && x && nrm && out && (!backward || dy), GMF_ERR_BAD_ARG, "rownorm_eps: null pointer");
  GMF_REQUIRE(rows > 0 && rows < (1LL << 31) && C > 0 && C <= 4096, GMF_ERR_UNSUPPORTED_SHAPE,
              "rownorm_eps: rows must be in 1 .. 2^31 - 1 and C in 1..4096");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_rownorm_eps(backward != 0, x, dy, nrm, out, rows, C, S(stream)));
  return GMF_OK;
}

int gmf_hardest_contrastive_forward(gmf_handle* h, const float* F0, long long N0, const float* F1, long long N1, int C,
                                    const long long* pairs, long long K, const long long* keys, const long long* pos_sel, long long P,
                                    const long long* sel0, long long H0, const long long* sel1, long long H1, float pos_thresh,
                                    float neg_thresh, long long* h01, long long* h10, unsigned char* keep0, unsigned char* keep1,
                                    float* D01, float* D10, float* terms, float* out, gmf_stream_t stream) {
  GMF_REQUIRE(h && F0 && F1 && pairs && keys && sel0 && sel1 && h01 && h10 && keep0 && keep1 && D01 && D10 && terms && out,
              GMF_ERR_BAD_ARG, "hardest_contrastive_forward: null pointer");
  GMF_REQUIRE(C >= 1 && C <= 64, GMF_ERR_UNSUPPORTED_SHAPE, "hardest_contrastive_forward: C must be in 1..64");
  GMF_REQUIRE(N0 >= 1 && N1 >= 1 && N0 < (1LL << 31) && N1 < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "hardest_contrastive_forward: N0 and N1 must be in 1 .. 2^31 - 1");
  GMF_REQUIRE(K >= 1 && P >= 1 && P < (1LL << 24) && (pos_sel || P == K), GMF_ERR_UNSUPPORTED_SHAPE,
              "hardest_contrastive_forward: K >= 1 and P in 1 .. 2^24 - 1 (P = K without pos_sel)");
  GMF_REQUIRE(H0 >= 1 && H1 >= 1 && H0 < (1LL << 31) && H1 < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "hardest_contrastive_forward: sel0 and sel1 must hold 1 .. 2^31 - 1 rows");
  SetDevice sd(h, stream);
  gmf::HclArgs a{F0, F1, (int)N0, (int)N1, C, pairs, K, keys, pos_sel, (int)P, sel0, (int)H0, sel1, (int)H1, pos_thresh, neg_thresh,
                 h01, h10, keep0, keep1, D01, D10, terms, out, h->status_dev, GMF_STATUS_LOSS_INDEX};
  GMF_HIP(gmf::launch_hcl_forward(a, S(stream)));
  return GMF_OK;
}

int gmf_hardest_contrastive_backward(gmf_handle* h, const float* F0, long long N0, const float* F1, long long N1, int C,
                                     const long long* pairs, long long K, const long long* pos_sel, long long P, const long long* h01,
                                     const long long* h10, const unsigned char* keep0, const unsigned char* keep1, const float* D01,
                                     const float* D10, const float* terms, const float* out, float neg_thresh, const float* g_pos,
                                     const float* g_neg, float* rows0, long long* dest0, float* rows1, long long* dest1,
                                     gmf_stream_t stream) {
  GMF_REQUIRE(h && F0 && F1 && pairs && h01 && h10 && keep0 && keep1 && D01 && D10 && terms && out && g_pos && g_neg && rows0 &&
                  dest0 && rows1 && dest1,
              GMF_ERR_BAD_ARG, "hardest_contrastive_backward: null pointer");
  GMF_REQUIRE(C >= 1 && C <= 64, GMF_ERR_UNSUPPORTED_SHAPE, "hardest_contrastive_backward: C must be in 1..64");
  GMF_REQUIRE(N0 >= 1 && N1 >= 1 && N0 < (1LL << 31) && N1 < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "hardest_contrastive_backward: N0 and N1 must be in 1 .. 2^31 - 1");
  GMF_REQUIRE(K >= 1 && P >= 1 && P < (1LL << 24) && (pos_sel || P == K), GMF_ERR_UNSUPPORTED_SHAPE,
              "hardest_contrastive_backward: K >= 1 and P in 1 .. 2^24 - 1 (P = K without pos_sel)");
  SetDevice sd(h, stream);
  gmf::HclBwdArgs a{F0, F1, (int)N0, (int)N1, C, pairs, K, pos_sel, (int)P, h01, h10, keep0, keep1, D01, D10, terms, out, neg_thresh,
                    g_pos, g_neg, rows0, dest0, rows1, dest1};
  GMF_HIP(gmf::launch_hcl_backward(a, S(stream)));
  return GMF_OK;
}

int gmf_rows_sum_by_dest(gmf_handle* h, const float* rows, long long E, const long long* order, const long long* row_start,
                         long long N, int C, float* out, gmf_stream_t stream) {
  GMF_REQUIRE(h && rows && order && row_start && out, GMF_ERR_BAD_ARG, "rows_sum_by_dest: null pointer");
  GMF_REQUIRE(E >= 1 && N >= 1 && N < (1LL << 31) && C >= 1 && C <= 64, GMF_ERR_UNSUPPORTED_SHAPE,
              "rows_sum_by_dest: E >= 1, N in 1 .. 2^31 - 1 and C in 1..64");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_rows_sum_by_dest(rows, E, order, row_start, N, C, out, S(stream)));
  return GMF_OK;
}

int gmf_batchnorm_masked_forward(gmf_handle* h, const float* x, const float* residual, const float* gamma, const float* beta,
                                 const int* n_rows, long long cap, int C, float eps, float momentum, int relu, float* y, float* mean,
                                 float* rstd, float* running_mean, float* running_var, gmf_stream_t stream) {
  GMF_REQUIRE(h && x && gamma && beta && n_rows && y && mean && rstd, GMF_ERR_BAD_ARG, "batchnorm_masked_forward: null pointer");
  GMF_REQUIRE((running_mean == nullptr) == (running_var == nullptr), GMF_ERR_BAD_ARG,
              "batchnorm_masked_forward: running stats come together");
  GMF_REQUIRE(cap >= 1 && cap < (1LL << 28) && C >= 1 && C <= 4096, GMF_ERR_UNSUPPORTED_SHAPE,
              "batchnorm_masked_forward: cap must be in 1 .. 2^28 - 1 and C in 1..4096");
  SetDevice sd(h, stream);
  float* part = nullptr;
  if (int rc = arena_carve(h, {arena_buf(part, gmf::bnm_part_floats(cap, C))})) return rc;
  GMF_HIP(gmf::launch_bnm_forward(x, residual, gamma, beta, n_rows, cap, C, eps, momentum, relu ? 1 : 0, y, mean, rstd, running_mean,
                                  running_var, part, h->status_dev, GMF_STATUS_BATCHNORM_ROWS, S(stream)));
  return GMF_OK;
}

int gmf_batchnorm_masked_backward(gmf_handle* h, const float* dy, const float* x, const float* y_relu, const float* mean,
                                  const float* rstd, const float* gamma, const int* n_rows, long long cap, int C, float* g, float* dx,
                                  float* dgamma, float* dbeta, gmf_stream_t stream) {
  GMF_REQUIRE(h && dy && x && mean && rstd && gamma && n_rows && g && dx && dgamma && dbeta, GMF_ERR_BAD_ARG,
              "batchnorm_masked_backward: null pointer");
  GMF_REQUIRE(cap >= 1 && cap < (1LL << 28) && C >= 1 && C <= 4096, GMF_ERR_UNSUPPORTED_SHAPE,
              "batchnorm_masked_backward: cap must be in 1 .. 2^28 - 1 and C in 1..4096");
  SetDevice sd(h, stream);
  float* part = nullptr;
  if (int rc = arena_carve(h, {arena_buf(part, gmf::bnm_part_floats(cap, C))})) return rc;
  GMF_HIP(gmf::launch_bnm_backward(dy, x, y_relu, mean, rstd, gamma, n_rows, cap, C, g, dx, dgamma, dbeta, part, S(stream)));
  return GMF_OK;
}

// ---- training of the image encoder (image_train_kernels.hip) ------------------------------------------------------------

// the checks the three convolution passes share: one of the five shapes, an image the kernel fits, pixel counts that index in int
static int conv2d_check(gmf_handle* h, const char* who, const gmf::Conv2dShape& s) {
  const std::string shape = std::string(who) + ": (cin, cout, ksize, stride) = (" + std::to_string(s.cin) + ", " + std::to_string(s.cout) +
                            ", " + std::to_string(s.ks) + ", " + std::to_string(s.stride) + ")";
  if (!gmf::conv2d_shape_ok(s))
    return fail(h, GMF_ERR_UNSUPPORTED_SHAPE, "gmf: " + shape + " is none of (3,64,7,2), (64,64,3,1), (128,128,3,1), (64,128,3,2), (64,128,1,2)");
  if (s.B <= 0 || s.H <= 0 || s.W <= 0)
    return fail(h, GMF_ERR_UNSUPPORTED_SHAPE, "gmf: " + std::string(who) + ": empty input [" + std::to_string(s.B) + ", " +
                                                  std::to_string(s.H) + ", " + std::to_string(s.W) + "]");
  if (s.in_pixels() >= (1LL << 30) || s.out_pixels() >= (1LL << 30))
    return fail(h, GMF_ERR_UNSUPPORTED_SHAPE, "gmf: " + std::string(who) + ": B * H * W must stay below 2^30 pixels: split the batch");
  return GMF_OK;
}

static bool dense_nhwc(const gmf::Conv2dShape& s, long long sb, long long sc, long long sh, long long sw) {
  return sc == 1 && sw == s.cin && sh == (long long)s.W * s.cin && sb == (long long)s.H * s.W * s.cin;
}

int gmf_conv2d_forward_f32(gmf_handle* h, const float* x, long long sb, long long sc, long long sh, long long sw, const float* w,
                           float* y, int B, int H, int W, int cin, int cout, int ksize, int stride, gmf_stream_t stream) {
  GMF_REQUIRE(h && x && w && y, GMF_ERR_BAD_ARG, "conv2d_forward_f32: null pointer");
  const gmf::Conv2dShape s{B, H, W, cin, cout, ksize, stride};
  if (int rc = conv2d_check(h, "conv2d_forward_f32", s)) return rc;
  GMF_REQUIRE(s.stem() ? (sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0) : dense_nhwc(s, sb, sc, sh, sw), GMF_ERR_BAD_ARG,
              "conv2d_forward_f32: x must be dense NHWC (only the 3-channel stem reads through non-negative element strides)");
  SetDevice sd(h, stream);
  float* wp;
  if (int rc = arena_carve(h, {arena_buf(wp, s.weight_floats())})) return rc;
  GMF_HIP(gmf::launch_conv2d_forward(s, x, sb, sc, sh, sw, w, wp, y, S(stream)));
  return GMF_OK;
}

int gmf_conv2d_dgrad(gmf_handle* h, const float* dy, const float* w, const float* dx_add, float* dx, int B, int H, int W, int cin,
                     int cout, int ksize, int stride, gmf_stream_t stream) {
  GMF_REQUIRE(h && dy && w && dx, GMF_ERR_BAD_ARG, "conv2d_dgrad: null pointer");
  const gmf::Conv2dShape s{B, H, W, cin, cout, ksize, stride};
  if (int rc = conv2d_check(h, "conv2d_dgrad", s)) return rc;
  GMF_REQUIRE(!s.stem(), GMF_ERR_UNSUPPORTED_SHAPE, "conv2d_dgrad: the stem (3, 64, 7, 2) has no dgrad (images carry no gradient)");
  SetDevice sd(h, stream);
  float* wp;
  if (int rc = arena_carve(h, {arena_buf(wp, s.weight_floats())})) return rc;
  GMF_HIP(gmf::launch_conv2d_dgrad(s, dy, w, wp, dx_add, dx, S(stream)));
  return GMF_OK;
}

int gmf_conv2d_wgrad(gmf_handle* h, const float* x, long long sb, long long sc, long long sh, long long sw, const float* dy, float* dw,
                     int B, int H, int W, int cin, int cout, int ksize, int stride, gmf_stream_t stream) {
  GMF_REQUIRE(h && x && dy && dw, GMF_ERR_BAD_ARG, "conv2d_wgrad: null pointer");
  const gmf::Conv2dShape s{B, H, W, cin, cout, ksize, stride};
  if (int rc = conv2d_check(h, "conv2d_wgrad", s)) return rc;
  GMF_REQUIRE(s.stem() ? (sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0) : dense_nhwc(s, sb, sc, sh, sw), GMF_ERR_BAD_ARG,
              "conv2d_wgrad: x must be dense NHWC (only the 3-channel stem reads through non-negative element strides)");
  SetDevice sd(h, stream);
  float* part;
  if (int rc = arena_carve(h, {arena_buf(part, (size_t)gmf::conv2d_wgrad_slabs(s) * s.weight_floats())})) return rc;
  GMF_HIP(gmf::launch_conv2d_wgrad(s, x, sb, sc, sh, sw, dy, part, dw, S(stream)));
  return GMF_OK;
}

static int maxpool_check(gmf_handle* h, const char* who, int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0) return fail(h, GMF_ERR_UNSUPPORTED_SHAPE, std::string("gmf: ") + who + ": empty input");
  if (C <= 0 || C % 4 != 0) return fail(h, GMF_ERR_UNSUPPORTED_SHAPE, std::string("gmf: ") + who + ": C = " + std::to_string(C) + " must be a positive multiple of 4");
  if ((long long)B * H * W * (C / 4) >= (1LL << 38))
    return fail(h, GMF_ERR_UNSUPPORTED_SHAPE, std::string("gmf: ") + who + ": B * H * W * C / 4 exceeds one launch: split the batch");
  return GMF_OK;
}

int gmf_maxpool3x3s2_forward(gmf_handle* h, const float* x, float* y, int B, int H, int W, int C, gmf_stream_t stream) {
  GMF_REQUIRE(h && x && y, GMF_ERR_BAD_ARG, "maxpool3x3s2_forward: null pointer");
  if (int rc = maxpool_check(h, "maxpool3x3s2_forward", B, H, W, C)) return rc;
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_maxpool_fwd(x, y, B, H, W, C, S(stream)));
  return GMF_OK;
}

int gmf_maxpool3x3s2_backward(gmf_handle* h, const float* x, const float* dy, float* dx, int B, int H, int W, int C,
                              gmf_stream_t stream) {
  GMF_REQUIRE(h && x && dy && dx, GMF_ERR_BAD_ARG, "maxpool3x3s2_backward: null pointer");
  if (int rc = maxpool_check(h, "maxpool3x3s2_backward", B, H, W, C)) return rc;
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_maxpool_bwd(x, dy, dx, B, H, W, C, S(stream)));
  return GMF_OK;
}

int gmf_batchnorm_residual_forward(gmf_handle* h, const float* x, const float* residual, const float* gamma, const float* beta,
                                   float* y, float* mean, float* rstd, float* running_mean, float* running_var, long long rows, int C,
                                   float eps, float momentum, int relu, gmf_stream_t stream) {
  GMF_REQUIRE(residual, GMF_ERR_BAD_ARG, "batchnorm_residual_forward: null pointer");
  return bn_dense_forward(h, "batchnorm_residual_forward", x, residual, gamma, beta, y, mean, rstd, running_mean, running_var, rows, C,
                          eps, momentum, relu, stream);
}

}  // extern "C"
