// C ABI of libgmf_hip.so (see include/gmf_hip.h).  Thin host layer: argument checks, the
// library-owned workspace arena, and the launch sequences.  No torch types, no host syncs.
#include "../../include/gmf_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "api_common.hpp"
#include "launchers_pose.hpp"
#include "launchers_solvers.hpp"
#include "launchers_spectral.hpp"
#include "launchers_pointcloud.hpp"
#include "launchers_sparse.hpp"
#include "launchers_dgr_input.hpp"
#include "launchers_correspondence.hpp"
#include "launchers_posegraph.hpp"
#include "launchers_clique.hpp"
#include "launchers_tsdf.hpp"
#include "launchers_rgbd.hpp"

namespace {

// the checks every descriptor entry shares
int check_cloud_args(gmf_handle* h, const char* what, const void* pts, const void* offsets, int B, long long total_rows, double r,
                     int max_nn) {
  GMF_REQUIRE(h && pts && offsets, GMF_ERR_BAD_ARG, std::string(what) + ": null pointer");
  GMF_REQUIRE(B > 0 && total_rows > 0 && total_rows < (1LL << 30) && B <= total_rows, GMF_ERR_UNSUPPORTED_SHAPE,
              std::string(what) + ": empty batch, more clouds than rows, or 2^30 rows or more");
  GMF_REQUIRE(r > 0 && std::isfinite(r), GMF_ERR_BAD_ARG, std::string(what) + ": radius / voxel size must be > 0 and finite");
  GMF_REQUIRE(max_nn >= 1 && max_nn <= gmf::kKnnMaxNN, GMF_ERR_BAD_ARG, std::string(what) + ": max_nn must be in 1..256");
  return GMF_OK;
}

// the checks gmf_pmc_graph and gmf_max_clique share
int check_pmc_args(gmf_handle* h, const char* what, const void* corr, const int* offsets, int B, long long total_rows, int max_n,
                          float inlier_threshold, int metric) {
  const std::string w(what);
  GMF_REQUIRE(h && offsets, GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(B > 0 && B <= 65535, GMF_ERR_UNSUPPORTED_SHAPE, w + ": B must be in 1..65535");
  GMF_REQUIRE(max_n >= 0 && total_rows >= 0, GMF_ERR_BAD_ARG, w + ": max_n and total_rows must be >= 0");
  GMF_REQUIRE(max_n <= gmf::kPmcMaxN, GMF_ERR_UNSUPPORTED_SHAPE, w + ": a pair holds at most 8192 rows");
  GMF_REQUIRE(total_rows < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE, w + ": total_rows must be below 2^31");
  GMF_REQUIRE(max_n == 0 || total_rows == 0 || corr, GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(inlier_threshold > 0.f && std::isfinite(inlier_threshold), GMF_ERR_BAD_ARG,
              w + ": inlier_threshold must be finite and > 0");
  GMF_REQUIRE(metric == gmf::kPmcSquared || metric == gmf::kPmcLength, GMF_ERR_BAD_ARG,
              w + ": metric must be 0 (squared lengths) or 1 (lengths)");
  return GMF_OK;
}

// the checks gmf_tsdf_allocate and gmf_tsdf_integrate share; fills `p`
int check_tsdf_args(gmf_handle* h, const char* what, const void* depth, const double* poses, const int* frame_offsets, int G, int F,
                    int H, int W, double fx, double fy, double cx, double cy, double voxel_length, double sdf_trunc,
                    double depth_scale, double depth_trunc, gmf::TsdfParams& p) {
  const std::string w(what);
  GMF_REQUIRE(h && frame_offsets, GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(G >= 1 && G <= gmf::kTsdfMaxFragments, GMF_ERR_UNSUPPORTED_SHAPE, w + ": G must be in 1..65535");
  GMF_REQUIRE(F >= 0 && H >= 1 && W >= 1 && (long long)F * H * W < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              w + ": F must be >= 0, H and W >= 1 and F H W below 2^31");
  GMF_REQUIRE(F == 0 || (depth && poses), GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(fx > 0 && fy > 0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy), GMF_ERR_BAD_ARG,
              w + ": the intrinsics must be finite, fx and fy > 0");
  GMF_REQUIRE(voxel_length > 0 && std::isfinite(voxel_length) && sdf_trunc > 0 && std::isfinite(sdf_trunc), GMF_ERR_BAD_ARG,
              w + ": voxel_length and sdf_trunc must be finite and > 0");
  GMF_REQUIRE(depth_scale > 0 && std::isfinite(depth_scale) && depth_trunc > 0 && !std::isnan(depth_trunc), GMF_ERR_BAD_ARG,
              w + ": depth_scale must be finite and > 0, depth_trunc > 0");
  p = gmf::TsdfParams{G, F, H, W, fx, fy, cx, cy, voxel_length, sdf_trunc, (float)depth_scale, (float)depth_trunc};
  return GMF_OK;
}

// the checks the gmf_rgbd_* entries share; fills `s`
int check_rgbd_shape(gmf_handle* h, const char* what, int F, int H, int W, int levels, gmf::RgbdShape& s) {
  const std::string w(what);
  GMF_REQUIRE(h, GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(F >= 1 && H >= 1 && W >= 1 && (long long)F * H * W < (1LL << 31) / gmf::kRgbdPlanes, GMF_ERR_UNSUPPORTED_SHAPE,
              w + ": F, H and W must be >= 1 and 6 F H W below 2^31");
  GMF_REQUIRE(levels >= 1 && levels <= gmf::kRgbdMaxLevels && (H >> (levels - 1)) >= 1 && (W >> (levels - 1)) >= 1,
              GMF_ERR_UNSUPPORTED_SHAPE, w + ": levels must be in 1..8 and leave the coarsest level a pixel");
  s = gmf::RgbdShape{F, H, W, levels};
  return GMF_OK;
}

// the checks gmf_rgbd_correspondences and gmf_rgbd_odometry share
int check_rgbd_pairs(gmf_handle* h, const char* what, const float* planes, const int* pair_source, const int* pair_target, int E,
                     double fx, double fy, double cx, double cy, double max_depth_diff) {
  const std::string w(what);
  GMF_REQUIRE(planes && pair_source && pair_target, GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(E >= 1 && E < (1 << 24), GMF_ERR_UNSUPPORTED_SHAPE, w + ": E must be in 1..2^24-1");
  GMF_REQUIRE(fx > 0 && fy > 0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy), GMF_ERR_BAD_ARG,
              w + ": the intrinsics must be finite, fx and fy > 0");
  GMF_REQUIRE(max_depth_diff >= 0 && std::isfinite(max_depth_diff), GMF_ERR_BAD_ARG, w + ": max_depth_diff must be finite and >= 0");
  return GMF_OK;
}

// neighbour lists of one descriptor call, in the workspace after the search grid
struct KnnLists {
  gmf::KnnScratch ws;
  int* idx;
  double* d2;
  int* count;
  double* spfh;
};

int take_knn(gmf_handle* h, long long N, int max_nn, bool spfh, KnnLists& k) {
  const size_t NK = (size_t)N * max_nn;
  ArenaList bufs;
  gmf::knn_scratch_list(N, k.ws, bufs);
  bufs.add(k.idx, NK);
  bufs.add(k.d2, NK);
  bufs.add(k.count, (size_t)N);
  bufs.add(k.spfh, spfh ? (size_t)N * 33 : 0);
  return arena_carve(h, bufs);
}

int voxel_call(gmf_handle* h, const char* what, const float* pts, const int* offsets, int B, long long total_rows, double voxel,
               float* out_pts, int* out_idx, int* out_offsets, long long* num_out, gmf_stream_t stream,
               const float* colors = nullptr, float* out_colors = nullptr) {
  if (int rc = check_cloud_args(h, what, pts, offsets, B, total_rows, voxel, 1)) return rc;
  GMF_REQUIRE((out_pts || out_idx) && out_offsets && num_out, GMF_ERR_BAD_ARG, std::string(what) + ": null pointer");
  SetDevice sd(h, stream);
  gmf::VoxelScratch ws;
  ArenaList bufs;
  gmf::voxel_scratch_list(total_rows, B, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  int host2[2] = {0, 0};
  GMF_HIP(gmf::launch_voxel(pts, offsets, B, total_rows, voxel, out_pts != nullptr, ws, out_pts, out_idx, out_offsets, host2,
                            S(stream), colors, out_colors));
  GMF_REQUIRE(host2[1] == 0, GMF_ERR_UNSUPPORTED_SHAPE,
              std::string(what) + ": a voxel index does not fit in int32 (voxel size too small for the extent) or a coordinate is "
                                  "not finite");
  *num_out = host2[0];
  return GMF_OK;
}

}  // namespace

extern "C" {

int gmf_abi_version(void) { return GMF_ABI_VERSION; }

int gmf_create(int device, gmf_handle** out) {
  if (!out) return GMF_ERR_BAD_ARG;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0 || device < 0 || device >= n) return GMF_ERR_NO_DEVICE;
  gmf_handle* h = new (std::nothrow) gmf_handle();
  if (!h) return GMF_ERR_OOM;
  h->device = device;
  // the sticky status word: host memory mapped into the device's address space (read by the host without a synchronisation)
  int prev = -1;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(device);
  void* hp = nullptr;
  if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess) {
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
      h->status_host = static_cast<int*>(hp);
      h->status_dev = static_cast<int*>(dp);
      *h->status_host = 0;
    } else {
      (void)hipHostFree(hp);
    }
  }
  if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
  if (!h->status_dev) { delete h; return GMF_ERR_OOM; }
  *out = h;
  return GMF_OK;
}

int gmf_set_workspace(gmf_handle* h, void* device_ptr, long long bytes) {
  GMF_REQUIRE(h, GMF_ERR_BAD_ARG, "set_workspace: null handle");
  GMF_REQUIRE((device_ptr == nullptr) == (bytes == 0) && bytes >= 0, GMF_ERR_BAD_ARG, "set_workspace: pass a pointer with its size, or NULL and 0");
  GMF_REQUIRE(((uintptr_t)device_ptr & 255) == 0, GMF_ERR_BAD_ARG, "set_workspace: the block must be 256-byte aligned");
  SetDevice sd(h);
  if (!h->arena_external && h->arena) {          // the library's own block goes (hipFree synchronises the device)
    hipError_t e = hipFree(h->arena);
    h->arena = nullptr;
    h->arena_bytes = 0;
    if (e != hipSuccess) return hip_fail(h, e, "hipFree(workspace)");
  }
  h->arena = device_ptr;
  h->arena_bytes = (size_t)bytes;
  h->arena_external = device_ptr != nullptr;
  return GMF_OK;
}

long long gmf_workspace_wanted(gmf_handle* h) { return h ? (long long)h->arena_wanted : 0; }

int gmf_status_read(gmf_handle* h, int* flags, int clear) {
  GMF_REQUIRE(h && flags, GMF_ERR_BAD_ARG, "status_read: null pointer");
  int* w = h->status_host;
  *flags = clear ? __atomic_exchange_n(w, 0, __ATOMIC_RELAXED) : __atomic_load_n(w, __ATOMIC_RELAXED);
  return GMF_OK;
}

int gmf_set_sigma_device(gmf_handle* h, const float* sigma_dev) {
  GMF_REQUIRE(h, GMF_ERR_BAD_ARG, "set_sigma_device: null handle");
  std::lock_guard<std::mutex> lock(h->mu);
  h->sigma_dev = sigma_dev;
  return GMF_OK;
}

static_assert(gmf::kSmMaxSplits == 32 && gmf::kPmcLocal == 384, "the ranges of spectral_col_splits and clique_local_rows in gmf::kKnobs");

int gmf_set_tuning(gmf_handle* h, const char* name, int value) {
  GMF_REQUIRE(h && name, GMF_ERR_BAD_ARG, "set_tuning: null pointer");
  std::lock_guard<std::mutex> lock(h->mu);        // (forwards read h->tune under the same lock)
  std::string why;                                // the knobs, their fields and the values they accept: gmf::kKnobs (encoder_plan.hpp)
  if (!gmf::set_knob(h->tune, name, value, &why)) return fail(h, GMF_ERR_BAD_ARG, "gmf: set_tuning: " + why);
  return GMF_OK;
}

// The current value of a knob (the counterpart of gmf_set_tuning: a caller that changes a knob for one call can put back what it found).
int gmf_get_tuning(gmf_handle* h, const char* name, int* value) {
  GMF_REQUIRE(h && name && value, GMF_ERR_BAD_ARG, "get_tuning: null pointer");
  std::lock_guard<std::mutex> lock(h->mu);
  if (!gmf::get_knob(h->tune, name, value)) return fail(h, GMF_ERR_BAD_ARG, std::string("gmf: get_tuning: unknown knob ") + name);
  return GMF_OK;
}

int gmf_profile_enable(gmf_handle* h, int on) {
  GMF_REQUIRE(h, GMF_ERR_BAD_ARG, "profile_enable: null handle");
  h->profile = (on != 0);
  h->prof_used = 0;
  return GMF_OK;
}

int gmf_profile_read(gmf_handle* h, double* scattn_ms_total, int* scattn_launches) {
  GMF_REQUIRE(h && scattn_ms_total && scattn_launches, GMF_ERR_BAD_ARG, "profile_read: null pointer");
  SetDevice sd(h);
  double total = 0.0;
  for (size_t i = 0; i < h->prof_used; ++i) {
    GMF_HIP(hipEventSynchronize(h->prof_events[i].second));
    float ms = 0.f;
    GMF_HIP(hipEventElapsedTime(&ms, h->prof_events[i].first, h->prof_events[i].second));
    total += ms;
  }
  *scattn_ms_total = total;
  *scattn_launches = (int)h->prof_used;
  h->prof_used = 0;
  return GMF_OK;
}

void gmf_destroy(gmf_handle* h) {
  if (!h) return;
  for (auto& e : h->prof_events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  int prev = -1;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(h->device);
  if (h->arena && !h->arena_external) (void)hipFree(h->arena);
  if (h->xs_event) (void)hipEventDestroy(h->xs_event);
  for (auto& sl : h->ptab_ring) {
    if (sl.ev) (void)hipEventDestroy(sl.ev);
    if (sl.host) (void)hipHostFree(sl.host);
  }
  for (void* p : h->graph_tables) (void)hipHostFree(p);
  if (h->status_host) (void)hipHostFree(h->status_host);
  if (prev >= 0 && prev != h->device) (void)hipSetDevice(prev);
  delete h;
}

const char* gmf_last_error_string(gmf_handle* h) { return h ? h->err.c_str() : "gmf: null handle"; }

long long gmf_workspace_bytes(gmf_handle* h) { return h ? (long long)h->arena_bytes : 0; }

// ---------------------------------------------------------------------------------------------
int gmf_pick_seeds(gmf_handle* h, const float* src_keypts, const float* scores, int B, int N, float nms_radius,
                   int use_nms, int num_seeds, int* seeds_out, gmf_stream_t stream) {
  GMF_REQUIRE(h && src_keypts && scores && seeds_out, GMF_ERR_BAD_ARG, "pick_seeds: null pointer");
  GMF_REQUIRE(B > 0 && N > 0 && num_seeds > 0 && num_seeds <= N, GMF_ERR_UNSUPPORTED_SHAPE, "pick_seeds: need 0 < num_seeds <= N");
  GMF_REQUIRE((size_t)num_seeds * 8 <= 156 * 1024, GMF_ERR_UNSUPPORTED_SHAPE, "pick_seeds: more than 19968 seeds (the winners' list lives in the LDS)");
  SetDevice sd(h, stream);
  hipStream_t st = S(stream);
  const float* keys = scores;
  float *kbuf, *scr;
  if (int rc = arena_carve(h, {arena_buf(kbuf, use_nms ? (size_t)B * N : 0), arena_buf(scr, use_nms ? gmf::nms_scratch_floats(B, N) : 0)}))
    return rc;
  if (use_nms) {
    GMF_HIP(gmf::launch_nms_keys(h->tune, src_keypts, scores, kbuf, B, N, nms_radius, st, scr));
    keys = kbuf;
  }
  GMF_HIP(gmf::launch_sort_topk(h->tune, keys, seeds_out, B, N, num_seeds, st));
  return GMF_OK;
}

static int pose_head_impl(gmf_handle* h, const gmf_pose_params* p, const float* feat_n, const float* src_keypts,
                          const float* tgt_keypts, const float* logits, const int* seeds_in, int B, int N, float* final_trans,
                          float* final_labels, int* seeds_out, int* knn_out, float* seed_trans, float* fitness,
                          gmf_stream_t stream, const int* n_points, double ratio);

int gmf_pose_head(gmf_handle* h, const gmf_pose_params* p, const float* feat_n, const float* src_keypts,
                  const float* tgt_keypts, const float* logits, const int* seeds_in, int B, int N, float* final_trans,
                  float* final_labels, int* seeds_out, int* knn_out, float* seed_trans, float* fitness,
                  gmf_stream_t stream) {
  GMF_REQUIRE(h && p, GMF_ERR_BAD_ARG, "pose_head: null pointer");
  GMF_REQUIRE(B > 0 && N > 1, GMF_ERR_UNSUPPORTED_SHAPE, "pose_head: need N > 1");
  return pose_head_impl(h, p, feat_n, src_keypts, tgt_keypts, logits, seeds_in, B, N, final_trans, final_labels, seeds_out, knn_out,
                        seed_trans, fitness, stream, nullptr, 0.0);
}

int gmf_pose_head_ragged(gmf_handle* h, const gmf_pose_params* p, double ratio, const float* feat_n, const float* src_keypts,
                         const float* tgt_keypts, const float* logits, const int* n_points, int B, float* final_trans,
                         float* final_labels, int* seeds_out, int* knn_out, float* seed_trans, float* fitness,
                         gmf_stream_t stream) {
  GMF_REQUIRE(h && p && n_points, GMF_ERR_BAD_ARG, "pose_head_ragged: null pointer");
  GMF_REQUIRE(B > 0, GMF_ERR_UNSUPPORTED_SHAPE, "pose_head_ragged: empty batch");
  GMF_REQUIRE(ratio > 0.0 && ratio <= 1.0, GMF_ERR_BAD_ARG, "pose_head_ragged: ratio must be in (0, 1]");
  GMF_REQUIRE(logits, GMF_ERR_BAD_ARG, "pose_head_ragged: the seeds come from the logits (no caller-provided seeds)");
  return pose_head_impl(h, p, feat_n, src_keypts, tgt_keypts, logits, nullptr, B, 0, final_trans, final_labels, seeds_out, knn_out,
                        seed_trans, fitness, stream, n_points, ratio);
}

static int pose_head_impl(gmf_handle* h, const gmf_pose_params* p, const float* feat_n, const float* src_keypts,
                          const float* tgt_keypts, const float* logits, const int* seeds_in, int B, int N, float* final_trans,
                          float* final_labels, int* seeds_out, int* knn_out, float* seed_trans, float* fitness,
                          gmf_stream_t stream, const int* n_points, double ratio) {
  GMF_REQUIRE(feat_n && src_keypts && tgt_keypts && final_trans && final_labels, GMF_ERR_BAD_ARG, "pose_head: null pointer");
  GMF_REQUIRE(seeds_in || logits, GMF_ERR_BAD_ARG, "pose_head: need logits or seeds_in");
  const bool ragged = n_points != nullptr;
  int Sn = p->num_seeds;
  const int k = p->k, iters = p->num_iterations;
  long long n_sum = (long long)B * N;
  SetDevice sd(h, stream);
  HostTable tab;
  const HostPart<gmf::PairTab> pairs = tab.add<gmf::PairTab>(ragged ? (size_t)B : 0);
  RingTaken ring;
  if (ragged) {
    // per-pair sizes from the host: S = int(n * ratio) seeds each; N, Sn below are the largest pair's (grids, buffer strides)
    if (int rc = check_ragged_sizes(h, n_points, B)) return rc;
    if (int rc = ring_take(h, tab, &ring)) return rc;
    gmf::plan_pair_table(n_points, B, ratio, k, pairs.host(ring.host), &N, &n_sum, &Sn);
    for (int b = 0; b < B; ++b) {
      GMF_REQUIRE(n_points[b] > k, GMF_ERR_UNSUPPORTED_SHAPE, "pose_head_ragged: every pair needs more than k correspondences (k = min(k, N - 1) "
                                                               "per pair is not supported in a ragged batch: run such a pair on its own)");
      GMF_REQUIRE((int)((double)n_points[b] * ratio) >= 1, GMF_ERR_UNSUPPORTED_SHAPE, "pose_head_ragged: a pair would have no seed (int(n * ratio) = 0)");
    }
  }
  GMF_REQUIRE(B > 0 && N > 1, GMF_ERR_UNSUPPORTED_SHAPE, "pose_head: need N > 1");
  GMF_REQUIRE(Sn > 0 && Sn <= N, GMF_ERR_UNSUPPORTED_SHAPE, "pose_head: need 0 < num_seeds <= N");
  GMF_REQUIRE(k > 0 && k <= 64 && k <= N - 1, GMF_ERR_UNSUPPORTED_SHAPE, "pose_head: need 0 < k <= min(64, N-1)");
  GMF_REQUIRE(iters > 0 && iters <= 64, GMF_ERR_BAD_ARG, "pose_head: bad num_iterations");
  // [r4] no limit on N (the reference has none: PointDSC.py:268-286, common.py:53-75; evaluation/test_3DMatch.py:143 feeds num_node = 'all'):
  // above 16 384 rows the seed selection reads its keys from global memory and the kNN selection streams the distance rows
  GMF_REQUIRE(seeds_in || (size_t)Sn * 8 <= 156 * 1024, GMF_ERR_UNSUPPORTED_SHAPE, "pose_head: more than 19968 seeds per pair (the winners' list lives in the LDS)");
  GMF_REQUIRE((p->sigma > 0.f || h->sigma_dev) && p->sigma_d > 0.f, GMF_ERR_BAD_ARG, "pose_head: sigma, sigma_d must be positive");
  hipStream_t st = S(stream);
  const size_t BS = (size_t)B * Sn;
  float *fimg, *dmat, *keys, *snaps, *sT, *fit;
  int *seeds, *knn, *counts, *best, *stop_it;
  unsigned char* conv;
  double* hsum;
  char* dtab;
  if (int rc = arena_carve(h, {arena_buf(fimg, (size_t)B * tiles_of(N) * kTileFloats),
                               arena_buf(dmat, BS * tiles_of(N) * 32),       // distance rows of the seeds, padded to whole tiles
                               arena_buf(keys, (size_t)B * N), arena_buf(seeds, BS), arena_buf(knn, BS * k),
                               arena_buf(snaps, BS * iters * k), arena_buf(conv, BS * iters), arena_buf(sT, BS * 16),
                               arena_buf(counts, BS), arena_buf(fit, BS), arena_buf(best, (size_t)B), arena_buf(hsum, BS * 15),
                               arena_buf(stop_it, 1), arena_buf(dtab, tab.bytes())}))
    return rc;
  const gmf::PairTab* const ptab = ragged ? pairs.dev(dtab) : nullptr;
  if (ragged) {
    if (int rc = ring_upload(h, ring, dtab, st)) return rc;
    // per-seed outputs are [B, S_max, ...] slots: the slots behind a pair's own seeds are defined (zero), not left-over memory
    if (seeds_out) GMF_HIP(hipMemsetAsync(seeds_out, 0, BS * sizeof(int), st));
    if (knn_out) GMF_HIP(hipMemsetAsync(knn_out, 0, BS * k * sizeof(int), st));
    if (seed_trans) GMF_HIP(hipMemsetAsync(seed_trans, 0, BS * 16 * sizeof(float), st));
    if (fitness) GMF_HIP(hipMemsetAsync(fitness, 0, BS * sizeof(float), st));
  }
  if (seeds_out) seeds = seeds_out;
  if (knn_out) knn = knn_out;
  if (seed_trans) sT = seed_trans;
  if (fitness) fit = fitness;

  const int* seeds_use = seeds_in;
  // the unit features as the split-fp16 image of k_seed_dist; [r5] the same launch hands the NMS its keys as a copy of the scores
  // (the all-pairs form with candidate splits starts from one: a hipMemcpyAsync of its own was 4 us + a kernel boundary at B = 1)
  const bool preset = !seeds_in && p->use_nms;
  GMF_HIP(gmf::launch_pack_rows_h2(feat_n, fimg, B, N, st, ptab, preset ? logits : nullptr, preset ? keys : nullptr,
                                   preset ? (ptab ? (long)n_sum : (long)B * N) : 0));
  if (!seeds_in) {
    const float* kk = logits;
    if (p->use_nms) {
      // dmat is free until k_seed_dist: it doubles as the grid-binning scratch of the NMS when it is large enough
      float* scr = (BS * N >= gmf::nms_scratch_floats(B, N)) ? dmat : nullptr;
      GMF_HIP(gmf::launch_nms_keys(h->tune, src_keypts, logits, keys, B, N, p->nms_radius, st, scr, ptab, (long)n_sum, true));
      kk = keys;
    }
    GMF_HIP(gmf::launch_sort_topk(h->tune, kk, seeds, B, N, Sn, st, ptab));
    seeds_use = seeds;
  } else if (seeds_out) {
    GMF_HIP(hipMemcpyAsync(seeds_out, seeds_in, BS * sizeof(int), hipMemcpyDeviceToDevice, st));
  }
  // feature-space distances of the seed rows by MFMA (k_seed_dist), then per-seed top-(k+1) selection
  // (the fused form - distances computed twice and never written - was built in round 4, is exact, and is not faster:
  // tools/ubench/archive/seed_knn_fused_r04.hip)
  GMF_HIP(gmf::launch_seed_dist(fimg, seeds_use, dmat, B, N, Sn, st, ptab));
  GMF_HIP(gmf::launch_knn_seeds(feat_n, seeds_use, dmat, knn, B, N, Sn, k, st, ptab));
  GMF_HIP(gmf::launch_seed_power(feat_n, src_keypts, tgt_keypts, knn, snaps, conv, hsum, B, N, Sn, k, iters, p->sigma, p->sigma_d, st, ptab, h->sigma_dev));
  GMF_HIP(gmf::launch_seed_kabsch(src_keypts, tgt_keypts, knn, snaps, conv, sT, B, N, Sn, k, iters, hsum, stop_it, st, ptab));
  GMF_HIP(gmf::launch_score_hyp(src_keypts, tgt_keypts, sT, counts, B, N, Sn, p->inlier_threshold, st, ptab));
  GMF_HIP(gmf::launch_finalize_pose(src_keypts, tgt_keypts, sT, counts, fit, final_trans, final_labels, best, B, N, Sn,
                                    p->inlier_threshold, p->refine_threshold, p->refine_iters, st, ptab));
  return GMF_OK;
}

int gmf_knn_from_distances(gmf_handle* h, const float* dist, int B, int N, int Sn, int k, int* knn_out, gmf_stream_t stream) {
  GMF_REQUIRE(h && dist && knn_out, GMF_ERR_BAD_ARG, "knn_from_distances: null pointer");
  GMF_REQUIRE(B > 0 && N > 1 && Sn > 0 && k > 0 && k <= 63 && k <= N - 1, GMF_ERR_UNSUPPORTED_SHAPE,
              "knn_from_distances: need 0 < k <= min(63, N - 1)");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_knn_seeds(nullptr, nullptr, dist, knn_out, B, N, Sn, k, S(stream), nullptr));
  return GMF_OK;
}

// self_first: the listed row itself is rank 0 of its distance row whatever ties with it (gmf_knn_rows_self_first)
static int knn_rows_impl(gmf_handle* h, const float* feat_n, const int* rows, int B, int N, int Sn, int k, int* knn_out,
                         gmf_stream_t stream, bool self_first) {
  GMF_REQUIRE(h && feat_n && rows && knn_out, GMF_ERR_BAD_ARG, "knn_rows: null pointer");
  GMF_REQUIRE(B > 0 && N > 1 && Sn > 0 && k > 0 && k <= N - 1, GMF_ERR_UNSUPPORTED_SHAPE, "knn_rows: need 0 < k <= N-1");
  SetDevice sd(h, stream);
  hipStream_t st = S(stream);
  if (k > 63) {            // (the selection kernels behind the distance rows rank up to 64 candidates: larger k keeps the in-LDS kNN)
    GMF_REQUIRE((size_t)N * 4 <= 150 * 1024, GMF_ERR_UNSUPPORTED_SHAPE, "knn_rows: k > 63 needs N <= 38400 (the in-LDS kNN)");
    if (!self_first) {
      GMF_HIP(gmf::launch_knn_seeds(feat_n, rows, nullptr, knn_out, B, N, Sn, k, st));
      return GMF_OK;
    }
  }
  // [r4] the pose head's own path (common.py:53-75 is what both compute): the rows' distances to every row of their pair by
  // MFMA (k_seed_dist on the split-fp16 feature image) and a threshold selection per row - 8 x 5000 x 5000: 10.7 ms -> below 1 ms
  // against one workgroup per row forming its distance row with vector instructions.  The distance rows are Sn x N floats per
  // pair: above 4 GiB the rows go through in slices, pair by pair.
  const int tiles = tiles_of(N);
  const size_t ld = (size_t)tiles * 32;
  const size_t cap = (size_t)1 << 30;                           // floats
  const bool whole = (size_t)B * Sn * ld <= cap;
  const int slice = whole ? Sn : (int)std::max<size_t>(1, std::min<size_t>((size_t)Sn, cap / ld));
  float *fimg, *dmat;
  if (int rc = arena_carve(h, {arena_buf(fimg, (size_t)B * tiles * kTileFloats), arena_buf(dmat, (size_t)(whole ? B : 1) * slice * ld)}))
    return rc;
  GMF_HIP(gmf::launch_pack_rows_h2(feat_n, fimg, B, N, st, nullptr));
  // distance rows -> [self first] -> selection, for nb pairs of n rows each
  auto select = [&](const float* img, const float* f, const int* rb, int* out, int nb, int n) -> int {
    GMF_HIP(gmf::launch_seed_dist(img, rb, dmat, nb, N, n, st, nullptr));
    if (self_first) GMF_HIP(gmf::launch_self_first(dmat, rb, nb, N, n, st));
    if (k > 63) GMF_HIP(gmf::launch_knn_lds(dmat, out, nb, N, n, k, st));
    else GMF_HIP(gmf::launch_knn_seeds(f, rb, dmat, out, nb, N, n, k, st, nullptr));
    return GMF_OK;
  };
  if (whole) return select(fimg, feat_n, rows, knn_out, B, Sn);
  for (int b = 0; b < B; ++b)
    for (int r0 = 0; r0 < Sn; r0 += slice) {
      const int n = std::min(slice, Sn - r0);
      if (int rc = select(fimg + (size_t)b * tiles * kTileFloats, feat_n + (size_t)b * N * 128, rows + (size_t)b * Sn + r0,
                          knn_out + ((size_t)b * Sn + r0) * k, 1, n))
        return rc;
    }
  return GMF_OK;
}

int gmf_knn_rows(gmf_handle* h, const float* feat_n, const int* rows, int B, int N, int Sn, int k, int* knn_out,
                 gmf_stream_t stream) {
  return knn_rows_impl(h, feat_n, rows, B, N, Sn, k, knn_out, stream, false);
}

int gmf_knn_rows_self_first(gmf_handle* h, const float* feat_n, const int* rows, int B, int N, int Sn, int k, int* knn_out,
                            gmf_stream_t stream) {
  return knn_rows_impl(h, feat_n, rows, B, N, Sn, k, knn_out, stream, true);
}

int gmf_nn_match(gmf_handle* h, const float* F0, const float* F1, int N0, int N1, int d, int mode, int* idx_out,
                 float* dist_out, gmf_stream_t stream) {
  GMF_REQUIRE(h && F0 && F1 && idx_out && dist_out, GMF_ERR_BAD_ARG, "nn_match: null pointer");
  GMF_REQUIRE(N0 > 0 && N1 > 0 && d > 0, GMF_ERR_UNSUPPORTED_SHAPE, "nn_match: empty input");
  GMF_REQUIRE(mode >= 0 && mode <= 2, GMF_ERR_BAD_ARG, "nn_match: mode must be 0 (PointDSC), 1 (DGR L2) or 2 (DGR SquareL2)");
  const int K = gmf::padded_desc_width(d);
  GMF_REQUIRE(K > 0, GMF_ERR_UNSUPPORTED_SHAPE, "nn_match: descriptor width above 128 is not supported");
  SetDevice sd(h, stream);
  const size_t n0 = (size_t)tiles_of(N0) * 32 * K, n1 = (size_t)tiles_of(N1) * 32 * K + 4096;
  float *i0, *i1, *nb;
  unsigned long long* best;
  if (int rc = arena_carve(h, {arena_buf(i0, n0),
                               arena_buf(i1, n1),      // + one stage of slack: the last stage may be read past the final tile
                               arena_buf(nb, (size_t)tiles_of(N1) * 32),       // whole tiles: the padding holds +inf
                               // (score, index) of every row's winner: one atomic minimum per key split
                               arena_buf(best, (size_t)N0)}))
    return rc;
  GMF_HIP(gmf::launch_nn_match(F0, F1, i0, i1, nb, best, idx_out, dist_out, N0, N1, d, mode, S(stream)));
  return GMF_OK;
}

// the checks the batched matching entries share: the descriptor width (-> *K, its padded width) and the two offset arrays
static int check_pair_offsets(gmf_handle* h, const char* what, const int* off0, const int* off1, int B, int d, int* K) {
  const std::string w(what);
  *K = gmf::padded_desc_width(d);
  GMF_REQUIRE(*K > 0, GMF_ERR_UNSUPPORTED_SHAPE, w + ": descriptor width above 128 is not supported");
  GMF_REQUIRE(off0[0] == 0 && off1[0] == 0, GMF_ERR_BAD_ARG, w + ": offsets must start at 0");
  for (int b = 0; b < B; ++b)
    GMF_REQUIRE(off0[b + 1] >= off0[b] && off1[b + 1] >= off1[b], GMF_ERR_BAD_ARG, w + ": offsets must ascend");
  return GMF_OK;
}

int gmf_nn_match_batched(gmf_handle* h, const float* F0, const float* F1, const int* off0, const int* off1, int B, int d, int mode,
                         int global_index, int* idx_out, float* dist_out, gmf_stream_t stream) {
  GMF_REQUIRE(h && off0 && off1, GMF_ERR_BAD_ARG, "nn_match_batched: null pointer");
  GMF_REQUIRE(B > 0 && d > 0, GMF_ERR_UNSUPPORTED_SHAPE, "nn_match_batched: empty batch");
  GMF_REQUIRE(mode >= 0 && mode <= 2, GMF_ERR_BAD_ARG, "nn_match_batched: mode must be 0 (PointDSC), 1 (DGR L2) or 2 (DGR SquareL2)");
  int K = 0;
  if (int rc = check_pair_offsets(h, "nn_match_batched", off0, off1, B, d, &K)) return rc;
  if (off0[B] == 0) return GMF_OK;                     // no query rows: nothing to write
  GMF_REQUIRE(F0 && F1 && idx_out && dist_out, GMF_ERR_BAD_ARG, "nn_match_batched: null pointer");
  SetDevice sd(h, stream);
  HostTable tab;
  const HostPart<gmf::MatchPair> pairs = tab.add<gmf::MatchPair>((size_t)B + 1);
  RingTaken ring;
  if (int rc = ring_take(h, tab, &ring)) return rc;
  gmf::MatchTotals tot;
  GMF_REQUIRE(gmf::plan_nn_match_batched(off0, off1, B, K, pairs.host(ring.host), &tot), GMF_ERR_UNSUPPORTED_SHAPE,
              "nn_match_batched: a pair has query rows and no key rows");
  GMF_REQUIRE(tot.wgs < (1L << 31) && tot.stages * tot.tps * 32 < (1L << 31), GMF_ERR_UNSUPPORTED_SHAPE, "nn_match_batched: batch too large");
  // the images hold whole tiles (queries) and whole stages (keys) of every pair: no slack behind the last stage is needed
  const size_t n0 = (size_t)tot.tiles0 * 32 * K, n1 = (size_t)tot.stages * tot.tps * 32 * K, nn = (size_t)tot.stages * tot.tps * 32;
  float *i0, *i1, *nb;
  unsigned long long* best;
  char* dtab;
  if (int rc = arena_carve(h, {arena_buf(i0, n0), arena_buf(i1, n1), arena_buf(nb, nn), arena_buf(best, (size_t)tot.rows0),
                               arena_buf(dtab, tab.bytes())})) return rc;
  if (int rc = ring_upload(h, ring, dtab, S(stream))) return rc;
  GMF_HIP(gmf::launch_nn_match_batched(F0, F1, i0, i1, nb, best, pairs.dev(dtab), B, tot, d, mode, global_index, idx_out, dist_out,
                                       S(stream)));
  return GMF_OK;
}

// gmf_nn_match_mutual_batched and gmf_build_correspondences: the checks of gmf_nn_match_batched, the two host plans (matching tables,
// chunk table) in ONE ring slot and ONE upload, one workspace list, then the chain of launchers_correspondence.hpp
static int run_correspondences(gmf_handle* h, const char* what, gmf::CorrArgs a, const int* off0, const int* off1, bool build,
                               gmf_stream_t stream) {
  const std::string w(what);
  const int B = a.B, d = a.d;
  GMF_REQUIRE(h && off0 && off1, GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(B > 0 && d > 0, GMF_ERR_UNSUPPORTED_SHAPE, w + ": empty batch");
  int K = 0;
  if (int rc = check_pair_offsets(h, what, off0, off1, B, d, &K)) return rc;
  if (build) {
    GMF_REQUIRE(a.in_dim == 3 || a.in_dim == 6, GMF_ERR_UNSUPPORTED_SHAPE, w + ": in_dim must be 3 or 6");
    GMF_REQUIRE(a.out_offsets, GMF_ERR_BAD_ARG, w + ": null pointer");
    GMF_REQUIRE(!a.gt_trans || (a.inlier_threshold > 0 && std::isfinite(a.inlier_threshold)), GMF_ERR_BAD_ARG,
                w + ": inlier_threshold must be > 0 and finite");
  }
  for (int b = 0; b < B; ++b)
    GMF_REQUIRE(off0[b + 1] == off0[b] || off1[b + 1] > off1[b], GMF_ERR_UNSUPPORTED_SHAPE, w + ": a pair has query rows and no key rows");
  if (off0[B] == 0) {                                    // no source rows: no output rows
    if (build) {
      SetDevice sd(h, stream);
      GMF_HIP(hipMemsetAsync(a.out_offsets, 0, (size_t)(B + 1) * sizeof(int), S(stream)));
    }
    return GMF_OK;
  }
  GMF_REQUIRE(a.F0 && a.F1 && (build || (a.idx && a.dist && a.mutual)), GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(!build || (a.kp0 && a.kp1 && a.corr && a.src_out && a.tgt_out && a.corr_pos), GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(!a.gt_trans == !a.labels, GMF_ERR_BAD_ARG, w + ": gt_trans and labels_out go together");
  GMF_REQUIRE(!a.src_desc_out == !a.tgt_desc_out, GMF_ERR_BAD_ARG, w + ": src_desc_out and tgt_desc_out go together");
  SetDevice sd(h, stream);
  // one ring slot: MatchPair [B + 1] | pair_chunk0 [B + 1] | CorrChunk [n_chunks], each part on a 16-byte boundary
  const long n_chunks = gmf::corr_chunk_count(off0, B);
  HostTable tab;
  const HostPart<gmf::MatchPair> pairs = tab.add<gmf::MatchPair>((size_t)B + 1);
  const HostPart<int> pair_chunk0 = tab.add<int>((size_t)B + 1);
  const HostPart<gmf::CorrChunk> chunks = tab.add<gmf::CorrChunk>((size_t)n_chunks);
  RingTaken ring;
  if (int rc = ring_take(h, tab, &ring)) return rc;
  gmf::MatchTotals tot;
  GMF_REQUIRE(gmf::plan_nn_match_batched(off0, off1, B, K, pairs.host(ring.host), &tot), GMF_ERR_UNSUPPORTED_SHAPE,
              w + ": a pair has query rows and no key rows");
  GMF_REQUIRE(tot.wgs < (1L << 31) && tot.stages * tot.tps * 32 < (1L << 31) && n_chunks < (1L << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              w + ": batch too large");
  gmf::corr_plan_chunks(off0, B, chunks.host(ring.host), pair_chunk0.host(ring.host));
  const size_t rows0 = (size_t)tot.rows0, nck = (size_t)n_chunks;
  char* dtab;
  ArenaList bufs{arena_buf(a.f0_img, (size_t)tot.tiles0 * 32 * K), arena_buf(a.f1_img, (size_t)tot.stages * tot.tps * 32 * K),
                 arena_buf(a.norm2, (size_t)tot.stages * tot.tps * 32), arena_buf(a.best, rows0),
                 arena_buf(a.colbest, a.use_mutual ? (size_t)off1[B] : 0), arena_buf(dtab, tab.bytes())};
  if (build) {                                           // (the caller of the flags alone brings idx, dist and mutual itself)
    bufs.add(a.idx, rows0);
    bufs.add(a.dist, rows0);
    bufs.add(a.mutual, rows0);
    bufs.add(a.rank, rows0);
    bufs.add(a.chunk_cnt, nck);
    bufs.add(a.chunk_sum, 6 * nck);
    bufs.add(a.chunk_excl, nck);
    bufs.add(a.mean, (size_t)6 * B);
  }
  if (int rc = arena_carve(h, bufs)) return rc;
  if (int rc = ring_upload(h, ring, dtab, S(stream))) return rc;
  a.tab = pairs.dev(dtab);
  a.pair_chunk0 = pair_chunk0.dev(dtab);
  a.chunks = chunks.dev(dtab);
  a.n_chunks = (int)n_chunks;
  a.n_keys = off1[B];
  GMF_HIP(gmf::launch_corr_match(a, tot, S(stream)));
  if (build) GMF_HIP(gmf::launch_corr_emit(a, S(stream)));
  return GMF_OK;
}

int gmf_nn_match_mutual_batched(gmf_handle* h, const float* F0, const float* F1, const int* off0, const int* off1, int B, int d,
                                int* idx_out, float* dist_out, unsigned char* mutual_out, gmf_stream_t stream) {
  gmf::CorrArgs a;
  a.F0 = F0; a.F1 = F1; a.B = B; a.d = d; a.use_mutual = 1;
  a.idx = idx_out; a.dist = dist_out; a.mutual = mutual_out;
  return run_correspondences(h, "nn_match_mutual_batched", a, off0, off1, false, stream);
}

int gmf_build_correspondences(gmf_handle* h, const float* F0, const float* F1, const float* src_keypts, const float* tgt_keypts,
                              const int* off0, const int* off1, int B, int d, int use_mutual, int in_dim, const float* gt_trans,
                              float inlier_threshold, int* out_offsets, long long* corr_out, float* src_out, float* tgt_out,
                              float* corr_pos_out, float* src_desc_out, float* tgt_desc_out, float* labels_out, gmf_stream_t stream) {
  gmf::CorrArgs a;
  a.F0 = F0; a.F1 = F1; a.kp0 = src_keypts; a.kp1 = tgt_keypts; a.B = B; a.d = d;
  a.use_mutual = use_mutual ? 1 : 0; a.in_dim = in_dim; a.gt_trans = gt_trans; a.inlier_threshold = inlier_threshold;
  a.out_offsets = out_offsets; a.corr = corr_out; a.src_out = src_out; a.tgt_out = tgt_out; a.corr_pos = corr_pos_out;
  a.src_desc_out = src_desc_out; a.tgt_desc_out = tgt_desc_out; a.labels = labels_out;
  return run_correspondences(h, "build_correspondences", a, off0, off1, true, stream);
}

// the checks gmf_matching_indices_count and _fill share
static int check_matching_args(gmf_handle* h, const char* what, const void* xyz0, const void* off0, const void* xyz1, const void* off1,
                               int B, long long total0, long long total1, const void* T, double radius) {
  GMF_REQUIRE(h && xyz0 && off0 && xyz1 && off1 && T, GMF_ERR_BAD_ARG, std::string(what) + ": null pointer");
  GMF_REQUIRE(B > 0 && total0 > 0 && total1 > 0 && total0 < (1LL << 30) && total1 < (1LL << 30), GMF_ERR_UNSUPPORTED_SHAPE,
              std::string(what) + ": empty batch, or 2^30 rows or more");
  GMF_REQUIRE(radius > 0 && std::isfinite(radius), GMF_ERR_BAD_ARG, std::string(what) + ": radius must be > 0 and finite");
  return GMF_OK;
}

int gmf_matching_indices_count(gmf_handle* h, const float* xyz0, const int* off0, const float* xyz1, const int* off1, int B,
                               long long total0, long long total1, const double* T, double radius, long long* row_start,
                               long long* pair_offsets, long long* num_pairs, gmf_stream_t stream) {
  if (int rc = check_matching_args(h, "matching_indices_count", xyz0, off0, xyz1, off1, B, total0, total1, T, radius)) return rc;
  GMF_REQUIRE(row_start && pair_offsets && num_pairs, GMF_ERR_BAD_ARG, "matching_indices_count: null pointer");
  SetDevice sd(h, stream);
  const size_t scan_bytes = gmf::matching_indices_scan_bytes(total0);
  int* cnt;
  char* scan_tmp;
  if (int rc = arena_carve(h, {arena_buf(cnt, (size_t)total0 + 1), arena_buf(scan_tmp, scan_bytes + 256)})) return rc;
  GMF_HIP(gmf::launch_matching_indices_count(xyz0, off0, xyz1, off1, B, total0, T, radius * radius, cnt, scan_tmp, scan_bytes, row_start,
                                             pair_offsets, S(stream)));
  long long k = 0;                                   // the one host read: the size of the output
  GMF_HIP(hipMemcpyAsync(&k, row_start + total0, sizeof(k), hipMemcpyDeviceToHost, S(stream)));
  GMF_HIP(hipStreamSynchronize(S(stream)));
  *num_pairs = k;
  return GMF_OK;
}

int gmf_matching_indices_fill(gmf_handle* h, const float* xyz0, const int* off0, const float* xyz1, const int* off1, int B,
                              long long total0, long long total1, const double* T, double radius, const long long* row_start,
                              long long* pairs, gmf_stream_t stream) {
  if (int rc = check_matching_args(h, "matching_indices_fill", xyz0, off0, xyz1, off1, B, total0, total1, T, radius)) return rc;
  GMF_REQUIRE(row_start && pairs, GMF_ERR_BAD_ARG, "matching_indices_fill: null pointer");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_matching_indices_fill(xyz0, off0, xyz1, off1, B, total0, T, radius * radius, row_start, pairs, S(stream)));
  return GMF_OK;
}

int gmf_inlier_input(gmf_handle* h, const int* nn, const long long* pred, const int* off0, const int* off1, int B, long long M,
                     long long* pred_out, const int* coords0, const int* coords1, int* coords_out, int feat_type, const float* a0,
                     const float* a1, int c, float* feats_out, const long long* pos_keys, const long long* pos_off,
                     const long long* seeds, unsigned char* labels_out, gmf_stream_t stream) {
  GMF_REQUIRE(h && off0, GMF_ERR_BAD_ARG, "inlier_input: null pointer");
  GMF_REQUIRE(B > 0 && M > 0 && M < (1LL << 30), GMF_ERR_UNSUPPORTED_SHAPE, "inlier_input: empty batch, or 2^30 pairs or more");
  GMF_REQUIRE((nn != nullptr) != (pred != nullptr), GMF_ERR_BAD_ARG, "inlier_input: pass the matches `nn` or the pairs `pred`, not both");
  GMF_REQUIRE(!nn || pred_out, GMF_ERR_BAD_ARG, "inlier_input: `nn` needs pred_out");
  GMF_REQUIRE(coords_out || labels_out, GMF_ERR_BAD_ARG, "inlier_input: nothing to write");
  if (coords_out) {
    GMF_REQUIRE(nn && off1 && coords0 && coords1 && feats_out, GMF_ERR_BAD_ARG, "inlier_input: the rows need nn, off1, both coordinate tensors and feats_out");
    GMF_REQUIRE(feat_type >= 0 && feat_type <= 2, GMF_ERR_BAD_ARG, "inlier_input: feat_type must be 0 (ones), 1 (feats) or 2 (coords)");
    GMF_REQUIRE(feat_type == 0 || (a0 && a1), GMF_ERR_BAD_ARG, "inlier_input: the features need their two source tensors");
    GMF_REQUIRE(feat_type != 1 || (c >= 1 && c <= gmf::kInlierMaxFeat), GMF_ERR_UNSUPPORTED_SHAPE, "inlier_input: 'feats' takes descriptors 1..64 wide");
  }
  if (labels_out) GMF_REQUIRE(pos_keys && pos_off && seeds, GMF_ERR_BAD_ARG, "inlier_input: the labels need pos_keys, pos_off and seeds");
  SetDevice sd(h, stream);
  gmf::InlierInput in;
  in.nn = nn; in.pred = pred; in.off0 = off0; in.off1 = off1; in.B = B; in.M = M; in.pred_out = pred_out;
  in.c0 = coords0; in.c1 = coords1; in.coords_out = coords_out; in.feat_type = feat_type; in.a0 = a0; in.a1 = a1; in.c = c;
  in.feats_out = feats_out; in.pos_keys = pos_keys; in.pos_off = pos_off; in.seeds = seeds; in.labels_out = labels_out;
  GMF_HIP(gmf::launch_inlier_input(in, S(stream)));
  return GMF_OK;
}

int gmf_procrustes_batched(gmf_handle* h, const float* A, const float* Bp, const float* weights, int n, int k,
                           float weight_threshold, float* T44, gmf_stream_t stream) {
  GMF_REQUIRE(h && A && Bp && T44, GMF_ERR_BAD_ARG, "procrustes_batched: null pointer");
  GMF_REQUIRE(n > 0 && k > 0, GMF_ERR_UNSUPPORTED_SHAPE, "procrustes_batched: empty input");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_rigid_transform(A, Bp, weights, T44, n, k, weight_threshold, S(stream)));
  return GMF_OK;
}

int gmf_post_refinement(gmf_handle* h, const float* T_in, const float* src_keypts, const float* tgt_keypts, int B, int N,
                        float refine_threshold, int iters, float* T_out, gmf_stream_t stream) {
  GMF_REQUIRE(h && T_in && src_keypts && tgt_keypts && T_out, GMF_ERR_BAD_ARG, "post_refinement: null pointer");
  GMF_REQUIRE(B > 0 && N > 0 && iters >= 0, GMF_ERR_UNSUPPORTED_SHAPE, "post_refinement: empty input");
  GMF_REQUIRE(refine_threshold > 0.f, GMF_ERR_BAD_ARG, "post_refinement: threshold must be positive");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_post_refine(T_in, src_keypts, tgt_keypts, T_out, B, N, refine_threshold, iters, S(stream)));
  return GMF_OK;
}

int gmf_weighted_procrustes(gmf_handle* h, const float* X, const float* Y, const float* w, const int* offsets, int B,
                            float eps, float* R, float* t, gmf_stream_t stream) {
  GMF_REQUIRE(h && X && Y && w && offsets && R && t, GMF_ERR_BAD_ARG, "weighted_procrustes: null pointer");
  GMF_REQUIRE(B > 0, GMF_ERR_UNSUPPORTED_SHAPE, "weighted_procrustes: empty batch");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_weighted_procrustes(X, Y, w, offsets, B, eps, R, t, S(stream)));
  return GMF_OK;
}

int gmf_global_registration(gmf_handle* h, const float* X, const float* Y, const float* w, const int* offsets, int B,
                            float eps, float quantization_size, int max_iter, int max_break_count,
                            double break_threshold_ratio, float* R, float* t, float* stats, int max_points,
                            gmf_stream_t stream) {
  GMF_REQUIRE(h && X && Y && offsets && R && t && stats, GMF_ERR_BAD_ARG, "global_registration: null pointer");
  GMF_REQUIRE(B > 0, GMF_ERR_UNSUPPORTED_SHAPE, "global_registration: empty batch");
  GMF_REQUIRE(quantization_size > 0.f && max_iter >= 0 && max_break_count >= 1, GMF_ERR_BAD_ARG,
              "global_registration: quantization_size must be > 0, max_iter >= 0, max_break_count >= 1");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_global_registration(X, Y, w, offsets, B, eps, quantization_size, max_iter, max_break_count,
                                          break_threshold_ratio, R, t, stats, max_points > 0 ? max_points : (1 << 30), S(stream)));
  return GMF_OK;
}

int gmf_ransac_correspondence(gmf_handle* h, const float* src, const float* tgt, const int* offsets, const unsigned char* mask,
                              int B, long long total_rows, int max_rows, int ransac_n, int num_hypotheses, float tau,
                              unsigned long long seed, int first_pair, float* T_out, unsigned char* inliers, float* fitness,
                              float* inlier_rmse, long long* hypothesis, long long* sample, gmf_stream_t stream) {
  GMF_REQUIRE(h && src && tgt && offsets && T_out && inliers && fitness && inlier_rmse && hypothesis && sample, GMF_ERR_BAD_ARG,
              "ransac_correspondence: null pointer");
  GMF_REQUIRE(B > 0 && total_rows > 0 && total_rows < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "ransac_correspondence: empty batch or more than 2^31 rows");
  GMF_REQUIRE(ransac_n >= 3 && ransac_n <= 8, GMF_ERR_BAD_ARG, "ransac_correspondence: ransac_n must be in 3..8");
  GMF_REQUIRE(num_hypotheses >= 1 && num_hypotheses <= (1 << 24), GMF_ERR_BAD_ARG,
              "ransac_correspondence: num_hypotheses must be in 1..2^24");
  GMF_REQUIRE(tau > 0.f && std::isfinite(tau), GMF_ERR_BAD_ARG, "ransac_correspondence: max_correspondence_distance must be > 0");
  GMF_REQUIRE(first_pair >= 0, GMF_ERR_BAD_ARG, "ransac_correspondence: first_pair must be >= 0");
  SetDevice sd(h, stream);
  gmf::RansacScratch ws;
  ArenaList bufs;
  gmf::ransac_scratch_list(total_rows, B, num_hypotheses, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_ransac(src, tgt, offsets, mask, B, total_rows, max_rows > 0 ? max_rows : (int)total_rows, ransac_n,
                             num_hypotheses, tau, seed, first_pair, ws, T_out, inliers, fitness, inlier_rmse, hypothesis, sample,
                             S(stream)));
  return GMF_OK;
}

int gmf_icp_point_to_point(gmf_handle* h, const float* src, const int* src_offsets, const float* tgt, const int* tgt_offsets,
                           int B, long long total_src, int max_src, int max_tgt, const float* init, float tau, int max_iter,
                           double rel_fitness, double rel_rmse, float* T_out, float* fitness, float* inlier_rmse,
                           int* iterations, long long* nn, gmf_stream_t stream) {
  GMF_REQUIRE(h && src && src_offsets && tgt && tgt_offsets && init && T_out && fitness && inlier_rmse && iterations && nn,
              GMF_ERR_BAD_ARG, "icp_point_to_point: null pointer");
  GMF_REQUIRE(B > 0 && total_src > 0 && total_src < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_point_to_point: empty batch or more than 2^31 source rows");
  GMF_REQUIRE(tau > 0.f && std::isfinite(tau), GMF_ERR_BAD_ARG, "icp_point_to_point: max_correspondence_distance must be > 0");
  GMF_REQUIRE(max_iter >= 0 && max_iter <= 100000, GMF_ERR_BAD_ARG, "icp_point_to_point: max_iteration must be in 0..100000");
  SetDevice sd(h, stream);
  gmf::IcpScratch ws;
  ArenaList bufs;
  gmf::icp_scratch_list(total_src, B, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_icp(src, src_offsets, tgt, tgt_offsets, B, total_src, max_src > 0 ? max_src : (int)total_src,
                          max_tgt > 0 ? max_tgt : (int)total_src, init, tau, max_iter, rel_fitness, rel_rmse, ws, T_out, fitness,
                          inlier_rmse, iterations, nn, S(stream)));
  return GMF_OK;
}

int gmf_icp_point_to_point_ex(gmf_handle* h, const float* src, const int* src_offsets, const float* tgt, const int* tgt_offsets,
                              int B, long long total_src, int max_src, int max_tgt, const float* init, float tau, int max_iter,
                              double rel_fitness, double rel_rmse, float* T_out, float* fitness, float* inlier_rmse,
                              int* iterations, long long* nn, long long total_tgt, int search, gmf_stream_t stream) {
  GMF_REQUIRE(h && src && src_offsets && tgt && tgt_offsets && init && T_out && fitness && inlier_rmse && iterations && nn,
              GMF_ERR_BAD_ARG, "icp_point_to_point_ex: null pointer");
  GMF_REQUIRE(B > 0 && total_src > 0 && total_src < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_point_to_point_ex: empty batch or more than 2^31 source rows");
  GMF_REQUIRE(total_tgt > 0 && total_tgt < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_point_to_point_ex: total_tgt must be in 1..2^31 - 1");
  GMF_REQUIRE(search == 0 || search == 1, GMF_ERR_BAD_ARG, "icp_point_to_point_ex: search must be 0 (brute force) or 1 (grid)");
  GMF_REQUIRE(tau > 0.f && std::isfinite(tau), GMF_ERR_BAD_ARG, "icp_point_to_point_ex: max_correspondence_distance must be > 0");
  GMF_REQUIRE(max_iter >= 0 && max_iter <= 100000, GMF_ERR_BAD_ARG, "icp_point_to_point_ex: max_iteration must be in 0..100000");
  // the grid's table has the next power of two >= 2 total_tgt slots, and its slots and scan are indexed with int32
  GMF_REQUIRE(search == 0 || total_tgt < (1LL << 29), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_point_to_point_ex: the grid search takes fewer than 2^29 target rows");
  if (search == 0)
    return gmf_icp_point_to_point(h, src, src_offsets, tgt, tgt_offsets, B, total_src, max_src, max_tgt, init, tau, max_iter,
                                  rel_fitness, rel_rmse, T_out, fitness, inlier_rmse, iterations, nn, stream);
  SetDevice sd(h, stream);
  gmf::IcpScratch ws;
  gmf::KnnScratch gs;
  ArenaList bufs;
  gmf::icp_scratch_list(total_src, B, ws, bufs);
  gmf::knn_scratch_list(total_tgt, gs, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_icp(src, src_offsets, tgt, tgt_offsets, B, total_src, max_src > 0 ? max_src : (int)total_src,
                          max_tgt > 0 ? max_tgt : (int)total_tgt, init, tau, max_iter, rel_fitness, rel_rmse, ws, T_out, fitness,
                          inlier_rmse, iterations, nn, S(stream), &gs, total_tgt));
  return GMF_OK;
}

int gmf_icp_point_to_plane(gmf_handle* h, const float* src, const int* src_offsets, const float* tgt, const float* tgt_normals,
                           const int* tgt_offsets, int B, long long total_src, int max_src, int max_tgt, const float* init,
                           float tau, int max_iter, double rel_fitness, double rel_rmse, float* T_out, float* fitness,
                           float* inlier_rmse, int* iterations, long long* nn, long long total_tgt, int search,
                           gmf_stream_t stream) {
  GMF_REQUIRE(h && src && src_offsets && tgt && tgt_normals && tgt_offsets && init && T_out && fitness && inlier_rmse &&
                  iterations && nn,
              GMF_ERR_BAD_ARG, "icp_point_to_plane: null pointer");
  GMF_REQUIRE(B > 0 && total_src > 0 && total_src < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_point_to_plane: empty batch or more than 2^31 source rows");
  GMF_REQUIRE(total_tgt > 0 && total_tgt < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_point_to_plane: total_tgt must be in 1..2^31 - 1");
  GMF_REQUIRE(search == 0 || search == 1, GMF_ERR_BAD_ARG, "icp_point_to_plane: search must be 0 (brute force) or 1 (grid)");
  GMF_REQUIRE(tau > 0.f && std::isfinite(tau), GMF_ERR_BAD_ARG, "icp_point_to_plane: max_correspondence_distance must be > 0");
  GMF_REQUIRE(max_iter >= 0 && max_iter <= 100000, GMF_ERR_BAD_ARG, "icp_point_to_plane: max_iteration must be in 0..100000");
  GMF_REQUIRE(search == 0 || total_tgt < (1LL << 29), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_point_to_plane: the grid search takes fewer than 2^29 target rows");
  GMF_REQUIRE(max_src <= total_src, GMF_ERR_BAD_ARG, "icp_point_to_plane: max_src exceeds total_src");
  const int bound_src = max_src > 0 ? max_src : (int)total_src;
  gmf::IcpPlaneScratch ps;
  ps.normals = tgt_normals;
  GMF_REQUIRE(gmf::icp_plane_plan(B, bound_src, ps.plan), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_point_to_plane: the step's B * ceil(max_src / kIcpPlaneRows) workgroups do not fit one launch");
  SetDevice sd(h, stream);
  gmf::IcpScratch ws;
  gmf::KnnScratch gs;
  ArenaList bufs;
  gmf::icp_scratch_list(total_src, B, ws, bufs);
  gmf::icp_plane_scratch_list(ps, bufs);
  if (search == 1) gmf::knn_scratch_list(total_tgt, gs, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_icp(src, src_offsets, tgt, tgt_offsets, B, total_src, bound_src, max_tgt > 0 ? max_tgt : (int)total_tgt, init,
                          tau, max_iter, rel_fitness, rel_rmse, ws, T_out, fitness, inlier_rmse, iterations, nn, S(stream),
                          search == 1 ? &gs : nullptr, total_tgt, &ps));
  return GMF_OK;
}

int gmf_icp_colored(gmf_handle* h, const float* src, const int* src_offsets, const float* tgt, const float* tgt_normals,
                    const int* tgt_offsets, int B, long long total_src, int max_src, int max_tgt, const float* init, float tau,
                    int max_iter, double rel_fitness, double rel_rmse, float* T_out, float* fitness, float* inlier_rmse,
                    int* iterations, long long* nn, long long total_tgt, int search, const float* src_intensity,
                    const float* tgt_intensity, const float* tgt_gradients, double lambda_geometric, gmf_stream_t stream) {
  GMF_REQUIRE(h && src && src_offsets && tgt && tgt_normals && tgt_offsets && init && T_out && fitness && inlier_rmse &&
                  iterations && nn && src_intensity && tgt_intensity && tgt_gradients,
              GMF_ERR_BAD_ARG, "icp_colored: null pointer");
  GMF_REQUIRE(B > 0 && total_src > 0 && total_src < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_colored: empty batch or more than 2^31 source rows");
  GMF_REQUIRE(total_tgt > 0 && total_tgt < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE, "icp_colored: total_tgt must be in 1..2^31 - 1");
  GMF_REQUIRE(search == 0 || search == 1, GMF_ERR_BAD_ARG, "icp_colored: search must be 0 (brute force) or 1 (grid)");
  GMF_REQUIRE(tau > 0.f && std::isfinite(tau), GMF_ERR_BAD_ARG, "icp_colored: max_correspondence_distance must be > 0");
  GMF_REQUIRE(max_iter >= 0 && max_iter <= 100000, GMF_ERR_BAD_ARG, "icp_colored: max_iteration must be in 0..100000");
  GMF_REQUIRE(lambda_geometric >= 0.0 && lambda_geometric <= 1.0, GMF_ERR_BAD_ARG,
              "icp_colored: lambda_geometric must be in 0..1");
  GMF_REQUIRE(search == 0 || total_tgt < (1LL << 29), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_colored: the grid search takes fewer than 2^29 target rows");
  GMF_REQUIRE(max_src <= total_src, GMF_ERR_BAD_ARG, "icp_colored: max_src exceeds total_src");
  const int bound_src = max_src > 0 ? max_src : (int)total_src;
  gmf::IcpPlaneScratch ps;
  ps.normals = tgt_normals;
  GMF_REQUIRE(gmf::icp_plane_plan(B, bound_src, ps.plan), GMF_ERR_UNSUPPORTED_SHAPE,
              "icp_colored: the step's B * ceil(max_src / kIcpPlaneRows) workgroups do not fit one launch");
  const gmf::IcpColorTerms ct{src_intensity, tgt_intensity, tgt_gradients, std::sqrt(lambda_geometric),
                              std::sqrt(1.0 - lambda_geometric)};
  SetDevice sd(h, stream);
  gmf::IcpScratch ws;
  gmf::KnnScratch gs;
  ArenaList bufs;
  gmf::icp_scratch_list(total_src, B, ws, bufs);
  gmf::icp_plane_scratch_list(ps, bufs);
  if (search == 1) gmf::knn_scratch_list(total_tgt, gs, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_icp(src, src_offsets, tgt, tgt_offsets, B, total_src, bound_src, max_tgt > 0 ? max_tgt : (int)total_tgt, init,
                          tau, max_iter, rel_fitness, rel_rmse, ws, T_out, fitness, inlier_rmse, iterations, nn, S(stream),
                          search == 1 ? &gs : nullptr, total_tgt, &ps, &ct));
  return GMF_OK;
}

// The host plan (chunk table, the edges' cloud indices, the cloud offsets) goes up in ONE ring slot and ONE upload.
int gmf_information_matrix(gmf_handle* h, const float* points, const int* cloud_offsets, int F, const int* edge_source,
                           const int* edge_target, int E, const double* transformation, float tau, double* info, int* count,
                           long long* nn, gmf_stream_t stream) {
  GMF_REQUIRE(h && points && cloud_offsets, GMF_ERR_BAD_ARG, "information_matrix: null pointer");
  GMF_REQUIRE(F > 0 && E >= 0, GMF_ERR_BAD_ARG, "information_matrix: F must be > 0 and E >= 0");
  GMF_REQUIRE(tau > 0.f && std::isfinite(tau), GMF_ERR_BAD_ARG, "information_matrix: max_correspondence_distance must be > 0");
  GMF_REQUIRE(cloud_offsets[0] == 0, GMF_ERR_BAD_ARG, "information_matrix: cloud_offsets must start at 0");
  for (int f = 0; f < F; ++f)
    GMF_REQUIRE(cloud_offsets[f + 1] > cloud_offsets[f], GMF_ERR_BAD_ARG, "information_matrix: cloud_offsets must increase (no empty cloud)");
  const long long N = cloud_offsets[F];
  // the grid's table has the next power of two >= 2 N slots, and its slots and scan are indexed with int32
  GMF_REQUIRE(N < (1LL << 29), GMF_ERR_UNSUPPORTED_SHAPE, "information_matrix: the grid takes fewer than 2^29 rows");
  if (E == 0) return GMF_OK;
  GMF_REQUIRE(edge_source && edge_target && transformation && info && count, GMF_ERR_BAD_ARG, "information_matrix: null pointer");
  long out_rows = 0;
  const long n_chunks = gmf::info_chunk_count(cloud_offsets, F, edge_source, edge_target, E, &out_rows);
  GMF_REQUIRE(n_chunks != -1, GMF_ERR_BAD_ARG, "information_matrix: an edge names a cloud outside 0..F-1");
  GMF_REQUIRE(n_chunks >= 0, GMF_ERR_UNSUPPORTED_SHAPE, "information_matrix: 2^31 or more source rows over the edges");
  SetDevice sd(h, stream);
  HostTable tab;
  const HostPart<int> cloud_off = tab.add<int>((size_t)F + 1), esrc = tab.add<int>((size_t)E), etgt = tab.add<int>((size_t)E);
  const HostPart<int> edge_chunk0 = tab.add<int>((size_t)E + 1);
  const HostPart<gmf::InfoChunk> chunks = tab.add<gmf::InfoChunk>((size_t)n_chunks);
  RingTaken ring;
  if (int rc = ring_take(h, tab, &ring)) return rc;
  std::copy_n(cloud_offsets, F + 1, cloud_off.host(ring.host));
  std::copy_n(edge_source, E, esrc.host(ring.host));
  std::copy_n(edge_target, E, etgt.host(ring.host));
  gmf::info_plan_chunks(cloud_offsets, edge_source, E, chunks.host(ring.host), edge_chunk0.host(ring.host));
  gmf::InfoScratch ws;
  char* dtab;
  ArenaList bufs;
  gmf::info_scratch_list(N, n_chunks, ws, bufs);
  bufs.add(dtab, tab.bytes());
  if (int rc = arena_carve(h, bufs)) return rc;
  if (int rc = ring_upload(h, ring, dtab, S(stream))) return rc;
  GMF_HIP(gmf::launch_information_matrix(points, cloud_off.dev(dtab), F, N, esrc.dev(dtab), etgt.dev(dtab), E, chunks.dev(dtab), n_chunks,
                                         edge_chunk0.dev(dtab), transformation, tau, ws, info, count, nn, S(stream)));
  return GMF_OK;
}

// The host plan: node_off | edge_off | hoff | esrc | etgt | node_list0 | the per-node edge lists, in one ring slot.
int gmf_posegraph_optimize(gmf_handle* h, double* poses, const int* node_offsets, const int* edge_offsets, int G,
                           const int* edge_source, const int* edge_target, const double* edge_transformation,
                           const double* edge_information, const unsigned char* edge_uncertain, const unsigned char* edge_mask,
                           const gmf_posegraph_options* opt, double* line_process, unsigned char* kept, int* stats, double* residual,
                           double* trace, gmf_stream_t stream) {
  GMF_REQUIRE(h && poses && node_offsets && edge_offsets && opt && stats && residual, GMF_ERR_BAD_ARG, "posegraph_optimize: null pointer");
  GMF_REQUIRE(G > 0, GMF_ERR_BAD_ARG, "posegraph_optimize: G must be > 0");
  GMF_REQUIRE(opt->max_iteration >= 0 && opt->max_iteration <= 100000 && opt->max_iteration_lm >= 0 && opt->max_iteration_lm <= 100000,
              GMF_ERR_BAD_ARG, "posegraph_optimize: max_iteration and max_iteration_lm must be in 0..100000");
  GMF_REQUIRE(opt->preference_loop_closure > 0 && std::isfinite(opt->preference_loop_closure), GMF_ERR_BAD_ARG,
              "posegraph_optimize: preference_loop_closure must be > 0");
  const int M = edge_offsets[G];
  GMF_REQUIRE(M == 0 || (edge_source && edge_target && edge_transformation && edge_information && edge_uncertain && line_process && kept),
              GMF_ERR_BAD_ARG, "posegraph_optimize: null pointer");
  const int bad = gmf::posegraph_check(node_offsets, edge_offsets, G, edge_source, edge_target);
  GMF_REQUIRE(bad != -1, GMF_ERR_BAD_ARG, "posegraph_optimize: offsets must ascend from 0 and every graph needs a node");
  GMF_REQUIRE(bad != -2, GMF_ERR_BAD_ARG, "posegraph_optimize: an edge names a node outside its graph");
  GMF_REQUIRE(bad != -3, GMF_ERR_BAD_ARG, "posegraph_optimize: an edge joins a node to itself");
  GMF_REQUIRE(bad == 0, GMF_ERR_UNSUPPORTED_SHAPE, "posegraph_optimize: a graph has more than 256 nodes or 65536 edges, which is what is built");
  const int N = node_offsets[G];
  SetDevice sd(h, stream);
  HostTable tab;
  const HostPart<int> node_off = tab.add<int>((size_t)G + 1), edge_off = tab.add<int>((size_t)G + 1);
  const HostPart<long long> h_off = tab.add<long long>((size_t)G + 1);
  const HostPart<int> esrc = tab.add<int>((size_t)M), etgt = tab.add<int>((size_t)M), node_list0 = tab.add<int>((size_t)N + 1);
  const HostPart<gmf::NodeEdge> lists = tab.add<gmf::NodeEdge>((size_t)2 * M);
  RingTaken ring;
  if (int rc = ring_take(h, tab, &ring)) return rc;
  std::copy_n(node_offsets, G + 1, node_off.host(ring.host));
  std::copy_n(edge_offsets, G + 1, edge_off.host(ring.host));
  long long* hoff = h_off.host(ring.host);
  hoff[0] = 0;
  for (int g = 0; g < G; ++g) {
    const long long n6 = 6LL * (node_offsets[g + 1] - node_offsets[g]);
    hoff[g + 1] = hoff[g] + n6 * n6;
  }
  const long long D = hoff[G];
  std::copy_n(edge_source, M, esrc.host(ring.host));      // (M = 0: nothing to copy, and the caller's arrays may be null)
  std::copy_n(edge_target, M, etgt.host(ring.host));
  gmf::posegraph_node_lists(node_offsets, edge_offsets, G, edge_source, edge_target, node_list0.host(ring.host), lists.host(ring.host));
  gmf::PoseGraphScratch ws;
  char* dtab;
  ArenaList bufs;
  gmf::posegraph_scratch_list(N, M, D, ws, bufs);
  bufs.add(dtab, tab.bytes());
  if (int rc = arena_carve(h, bufs)) return rc;
  if (int rc = ring_upload(h, ring, dtab, S(stream))) return rc;
  gmf::PoseGraphOptions o;
  o.max_iteration = opt->max_iteration; o.max_iteration_lm = opt->max_iteration_lm; o.reference_node = opt->reference_node;
  o.min_relative_increment = opt->min_relative_increment;
  o.min_relative_residual_increment = opt->min_relative_residual_increment;
  o.min_right_term = opt->min_right_term; o.min_residual = opt->min_residual;
  o.edge_prune_threshold = opt->edge_prune_threshold; o.preference_loop_closure = opt->preference_loop_closure;
  GMF_HIP(gmf::launch_posegraph(poses, node_off.dev(dtab), edge_off.dev(dtab), h_off.dev(dtab), G, esrc.dev(dtab), etgt.dev(dtab),
                                edge_transformation, edge_information, edge_uncertain, edge_mask, node_list0.dev(dtab), lists.dev(dtab),
                                o, ws, line_process, kept, stats, residual, trace, h->status_dev, GMF_STATUS_POSEGRAPH_PIVOT, S(stream)));
  return GMF_OK;
}

int gmf_ransac_feature_matching(gmf_handle* h, const float* src, const int* src_offsets, const float* tgt, const int* tgt_offsets,
                                const long long* nn, int B, long long total_src, long long total_tgt, int max_src, int ransac_n,
                                int max_iteration, int max_validation, float tau, float checker_distance,
                                float edge_length_threshold, unsigned long long seed, int first_pair, int search, float* T_out,
                                float* fitness, float* inlier_rmse, long long* hypothesis, long long* sample, long long* nn_out,
                                int* validated, int* hyp, int* count, long long* sum, gmf_stream_t stream) {
  GMF_REQUIRE(h && src && src_offsets && tgt && tgt_offsets && nn && T_out && fitness && inlier_rmse && hypothesis && sample &&
                  nn_out && validated,
              GMF_ERR_BAD_ARG, "ransac_feature_matching: null pointer");
  GMF_REQUIRE(B > 0 && total_src > 0 && total_src < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "ransac_feature_matching: empty batch or more than 2^31 source rows");
  GMF_REQUIRE(total_tgt > 0 && total_tgt < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE,
              "ransac_feature_matching: total_tgt must be in 1..2^31 - 1");
  GMF_REQUIRE(search == 0 || search == 1, GMF_ERR_BAD_ARG, "ransac_feature_matching: search must be 0 (brute force) or 1 (grid)");
  GMF_REQUIRE(ransac_n >= 3 && ransac_n <= 8, GMF_ERR_BAD_ARG, "ransac_feature_matching: ransac_n must be in 3..8");
  GMF_REQUIRE(max_iteration >= 1 && max_iteration <= (1 << 24), GMF_ERR_BAD_ARG,
              "ransac_feature_matching: max_iteration must be in 1..2^24");
  GMF_REQUIRE(max_validation >= 1 && max_validation <= 65536, GMF_ERR_BAD_ARG,
              "ransac_feature_matching: max_validation must be in 1..65536");
  GMF_REQUIRE(tau > 0.f && std::isfinite(tau), GMF_ERR_BAD_ARG, "ransac_feature_matching: max_correspondence_distance must be > 0");
  GMF_REQUIRE(!std::isnan(checker_distance) && !std::isinf(checker_distance), GMF_ERR_BAD_ARG,
              "ransac_feature_matching: checker_distance must be finite (negative: no distance checker)");
  GMF_REQUIRE(!std::isnan(edge_length_threshold) && edge_length_threshold <= 1.f, GMF_ERR_BAD_ARG,
              "ransac_feature_matching: edge_length_threshold must be <= 1 (<= 0: no edge-length checker)");
  GMF_REQUIRE(first_pair >= 0, GMF_ERR_BAD_ARG, "ransac_feature_matching: first_pair must be >= 0");
  // the grid's table has the next power of two >= 2 total_tgt slots, and its slots and scan are indexed with int32
  GMF_REQUIRE(search == 0 || total_tgt < (1LL << 29), GMF_ERR_UNSUPPORTED_SHAPE,
              "ransac_feature_matching: the grid search takes fewer than 2^29 target rows");
  SetDevice sd(h, stream);
  gmf::FmScratch ws;
  gmf::KnnScratch gs;
  ArenaList bufs;
  gmf::fm_scratch_list(total_src, B, max_iteration, max_validation, ws, bufs);
  if (search) gmf::knn_scratch_list(total_tgt, gs, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  if (hyp) ws.hyp = hyp;
  if (count) ws.cnt = reinterpret_cast<unsigned*>(count);
  if (sum) ws.sq = reinterpret_cast<unsigned long long*>(sum);
  GMF_HIP(gmf::launch_ransac_feature_matching(src, src_offsets, tgt, tgt_offsets, nn, B, total_src, total_tgt,
                                              max_src > 0 ? max_src : (int)total_src, ransac_n, max_iteration, max_validation, tau,
                                              checker_distance, edge_length_threshold, seed, first_pair, ws, search ? &gs : nullptr,
                                              T_out, fitness, inlier_rmse, hypothesis, sample, nn_out, validated, S(stream)));
  return GMF_OK;
}

int gmf_spectral_matching(gmf_handle* h, const float* corr, const float* src, const float* tgt, const int* offsets, int B, int max_n,
                          float inlier_threshold, const int* topk, int iterations, float* eig_out, float* labels_out, float* T_out,
                          gmf_stream_t stream) {
  GMF_REQUIRE(h && offsets && topk && T_out, GMF_ERR_BAD_ARG, "spectral_matching: null pointer");
  GMF_REQUIRE(B > 0 && B <= 65535, GMF_ERR_UNSUPPORTED_SHAPE, "spectral_matching: B must be in 1..65535");
  GMF_REQUIRE(max_n >= 0, GMF_ERR_BAD_ARG, "spectral_matching: max_n must be >= 0");
  GMF_REQUIRE(max_n == 0 || (corr && src && tgt && eig_out && labels_out), GMF_ERR_BAD_ARG, "spectral_matching: null pointer");
  GMF_REQUIRE(inlier_threshold > 0.f && std::isfinite(inlier_threshold), GMF_ERR_BAD_ARG,
              "spectral_matching: inlier_threshold must be finite and > 0");
  GMF_REQUIRE(iterations >= 1 && iterations <= 1000, GMF_ERR_BAD_ARG, "spectral_matching: iterations must be in 1..1000");
  SetDevice sd(h, stream);
  // the partial sums are [splits, total_rows]; the call does not read the offsets back, so total_rows is bounded by B max_n
  const long long total_rows = (long long)B * max_n;
  GMF_REQUIRE(total_rows < (1LL << 31), GMF_ERR_UNSUPPORTED_SHAPE, "spectral_matching: B max_n must be below 2^31");
  const int forced = h->tune.spectral_col_splits;
  float* partial = nullptr;
  if (int rc = arena_carve(h, {arena_buf(partial, gmf::sm_scratch_floats(total_rows, max_n, forced))})) return rc;
  GMF_HIP(gmf::launch_spectral_matching(corr, src, tgt, offsets, B, total_rows, max_n, inlier_threshold, topk, iterations, forced,
                                        partial, eig_out, labels_out, T_out, S(stream)));
  return GMF_OK;
}

int gmf_pmc_graph(gmf_handle* h, const float* corr, const int* offsets, int B, long long total_rows, int max_n,
                  float inlier_threshold, int metric, unsigned long long* bits_out, int* degree_out, gmf_stream_t stream) {
  if (int rc = check_pmc_args(h, "pmc_graph", corr, offsets, B, total_rows, max_n, inlier_threshold, metric)) return rc;
  GMF_REQUIRE(max_n == 0 || total_rows == 0 || (bits_out && degree_out), GMF_ERR_BAD_ARG, "pmc_graph: null pointer");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_pmc_graph(corr, offsets, B, total_rows, max_n, inlier_threshold, metric, bits_out, degree_out, S(stream)));
  return GMF_OK;
}

int gmf_max_clique(gmf_handle* h, const float* corr, const float* src, const float* tgt, const int* offsets, int B,
                   long long total_rows, int max_n, float inlier_threshold, int metric, long long max_steps, float* labels_out,
                   float* T_out, int* size_out, int* exact_out, long long* steps_out, int* degree_out, gmf_stream_t stream) {
  if (int rc = check_pmc_args(h, "max_clique", corr, offsets, B, total_rows, max_n, inlier_threshold, metric)) return rc;
  GMF_REQUIRE(T_out && size_out && exact_out && steps_out, GMF_ERR_BAD_ARG, "max_clique: null pointer");
  GMF_REQUIRE(max_n == 0 || total_rows == 0 || (src && tgt && labels_out && degree_out), GMF_ERR_BAD_ARG,
              "max_clique: null pointer");
  GMF_REQUIRE(max_steps >= 1, GMF_ERR_BAD_ARG, "max_clique: max_steps must be >= 1");
  SetDevice sd(h, stream);
  gmf::PmcScratch ws;
  ArenaList bufs;
  gmf::pmc_scratch_list(B, total_rows, max_n, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_max_clique(corr, src, tgt, offsets, B, total_rows, max_n, inlier_threshold, metric, max_steps,
                                 h->tune.clique_local_rows, ws, labels_out, T_out, size_out, exact_out, steps_out, degree_out, S(stream)));
  return GMF_OK;
}

int gmf_tsdf_allocate(gmf_handle* h, const void* depth, int depth_is_u16, const double* poses, const int* frame_offsets, int G, int F,
                      int H, int W, double fx, double fy, double cx, double cy, double voxel_length, double sdf_trunc,
                      double depth_scale, double depth_trunc, int stride, int max_units, int* unit_keys_out, int* birth_out,
                      int* unit_offsets_out, long long* num_units, gmf_stream_t stream) {
  gmf::TsdfParams p;
  if (int rc = check_tsdf_args(h, "tsdf_allocate", depth, poses, frame_offsets, G, F, H, W, fx, fy, cx, cy, voxel_length, sdf_trunc,
                               depth_scale, depth_trunc, p))
    return rc;
  GMF_REQUIRE(unit_keys_out && birth_out && unit_offsets_out && num_units, GMF_ERR_BAD_ARG, "tsdf_allocate: null pointer");
  GMF_REQUIRE(stride >= 1, GMF_ERR_BAD_ARG, "tsdf_allocate: stride must be >= 1");
  GMF_REQUIRE(max_units >= 1 && max_units <= (1 << 22), GMF_ERR_BAD_ARG, "tsdf_allocate: max_units must be in 1..2^22");
  SetDevice sd(h, stream);
  gmf::TsdfAllocScratch ws;
  ArenaList bufs;
  gmf::tsdf_alloc_scratch_list(G, max_units, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  int host2[2] = {0, 0};
  GMF_HIP(gmf::launch_tsdf_allocate(depth, depth_is_u16 != 0, poses, frame_offsets, p, stride, max_units, ws, unit_keys_out, birth_out,
                                    unit_offsets_out, host2, S(stream)));
  GMF_REQUIRE(!(host2[1] & gmf::kTsdfRange), GMF_ERR_UNSUPPORTED_SHAPE,
              "tsdf_allocate: a unit index lies outside +-32767 (or a pose is not finite): raise voxel_length");
  GMF_REQUIRE(!(host2[1] & gmf::kTsdfOverflow) && host2[0] <= max_units, GMF_ERR_UNSUPPORTED_SHAPE,
              "tsdf_allocate: the frames touch more than max_units = " + std::to_string(max_units) + " volume units: raise max_units");
  *num_units = host2[0];
  return GMF_OK;
}

namespace {

// gmf_tsdf_integrate (color, color_out null) and gmf_tsdf_integrate_color
int tsdf_integrate(gmf_handle* h, const char* what, bool colored, const void* depth, int depth_is_u16, const unsigned char* color,
                   const double* poses_inv, const int* frame_offsets, int G, int F, int H, int W, double fx, double fy, double cx,
                   double cy, double voxel_length, double sdf_trunc, double depth_scale, double depth_trunc, const int* unit_keys,
                   const int* unit_offsets, const int* birth, int num_units, float* tsdf_out, float* weight_out, float* color_out,
                   gmf_stream_t stream) {
  const std::string w(what);
  gmf::TsdfParams p;
  if (int rc = check_tsdf_args(h, what, depth, poses_inv, frame_offsets, G, F, H, W, fx, fy, cx, cy, voxel_length, sdf_trunc,
                               depth_scale, depth_trunc, p))
    return rc;
  GMF_REQUIRE(num_units >= 0 && num_units <= (1 << 22), GMF_ERR_BAD_ARG, w + ": num_units must be in 0..2^22");
  if (num_units == 0) return GMF_OK;
  GMF_REQUIRE(F >= 1 && unit_keys && unit_offsets && birth && tsdf_out && weight_out && (!colored || (color && color_out)),
              GMF_ERR_BAD_ARG, w + ": null pointer, or units without frames");
  SetDevice sd(h, stream);
  gmf::TsdfIntegrateScratch ws;
  ArenaList bufs;
  gmf::tsdf_integrate_scratch_list(p, colored, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_tsdf_integrate(depth, depth_is_u16 != 0, color, poses_inv, frame_offsets, p, unit_keys, unit_offsets, birth,
                                     num_units, ws, tsdf_out, weight_out, color_out, S(stream)));
  return GMF_OK;
}

// gmf_tsdf_extract (color, colors_out null) and gmf_tsdf_extract_color
int tsdf_extract(gmf_handle* h, const char* what, bool colored, const int* unit_keys, const int* unit_offsets, int G, int num_units,
                 const float* tsdf, const float* weight, const float* color, double voxel_length, float* points_out, float* colors_out,
                 long long max_points, int* point_offsets_out, long long* num_points, gmf_stream_t stream) {
  const std::string w(what);
  GMF_REQUIRE(h && unit_offsets && point_offsets_out, GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(points_out || num_points, GMF_ERR_BAD_ARG, w + ": without points_out the call counts into num_points");
  GMF_REQUIRE(!colored || !points_out || colors_out, GMF_ERR_BAD_ARG, w + ": points_out and colors_out are written together");
  GMF_REQUIRE(G >= 1 && G <= gmf::kTsdfMaxFragments, GMF_ERR_UNSUPPORTED_SHAPE, w + ": G must be in 1..65535");
  GMF_REQUIRE(num_units >= 0 && num_units <= (1 << 22), GMF_ERR_BAD_ARG, w + ": num_units must be in 0..2^22");
  GMF_REQUIRE(num_units == 0 || (unit_keys && tsdf && weight && (!colored || color)), GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(voxel_length > 0 && std::isfinite(voxel_length), GMF_ERR_BAD_ARG, w + ": voxel_length must be finite and > 0");
  GMF_REQUIRE(max_points >= 0, GMF_ERR_BAD_ARG, w + ": max_points must be >= 0");
  SetDevice sd(h, stream);
  if (num_units == 0) {
    GMF_HIP(hipMemsetAsync(point_offsets_out, 0, ((size_t)G + 1) * 4, S(stream)));
    if (!points_out) *num_points = 0;
    return GMF_OK;
  }
  gmf::TsdfExtractScratch ws;
  ArenaList bufs;
  gmf::tsdf_extract_scratch_list(num_units, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  int host_count = 0;
  GMF_HIP(gmf::launch_tsdf_extract(unit_keys, unit_offsets, G, num_units, tsdf, weight, color, voxel_length, ws, points_out, colors_out,
                                   max_points, point_offsets_out, &host_count, S(stream)));
  if (!points_out) *num_points = host_count;
  return GMF_OK;
}

}  // namespace

int gmf_tsdf_integrate(gmf_handle* h, const void* depth, int depth_is_u16, const double* poses_inv, const int* frame_offsets, int G,
                       int F, int H, int W, double fx, double fy, double cx, double cy, double voxel_length, double sdf_trunc,
                       double depth_scale, double depth_trunc, const int* unit_keys, const int* unit_offsets, const int* birth,
                       int num_units, float* tsdf_out, float* weight_out, gmf_stream_t stream) {
  return tsdf_integrate(h, "tsdf_integrate", false, depth, depth_is_u16, nullptr, poses_inv, frame_offsets, G, F, H, W, fx, fy, cx, cy,
                        voxel_length, sdf_trunc, depth_scale, depth_trunc, unit_keys, unit_offsets, birth, num_units, tsdf_out,
                        weight_out, nullptr, stream);
}

int gmf_tsdf_integrate_color(gmf_handle* h, const void* depth, int depth_is_u16, const unsigned char* color, const double* poses_inv,
                             const int* frame_offsets, int G, int F, int H, int W, double fx, double fy, double cx, double cy,
                             double voxel_length, double sdf_trunc, double depth_scale, double depth_trunc, const int* unit_keys,
                             const int* unit_offsets, const int* birth, int num_units, float* tsdf_out, float* weight_out,
                             float* color_out, gmf_stream_t stream) {
  return tsdf_integrate(h, "tsdf_integrate_color", true, depth, depth_is_u16, color, poses_inv, frame_offsets, G, F, H, W, fx, fy, cx,
                        cy, voxel_length, sdf_trunc, depth_scale, depth_trunc, unit_keys, unit_offsets, birth, num_units, tsdf_out,
                        weight_out, color_out, stream);
}

int gmf_tsdf_extract(gmf_handle* h, const int* unit_keys, const int* unit_offsets, int G, int num_units, const float* tsdf,
                     const float* weight, double voxel_length, float* points_out, long long max_points, int* point_offsets_out,
                     long long* num_points, gmf_stream_t stream) {
  return tsdf_extract(h, "tsdf_extract", false, unit_keys, unit_offsets, G, num_units, tsdf, weight, nullptr, voxel_length, points_out,
                      nullptr, max_points, point_offsets_out, num_points, stream);
}

int gmf_tsdf_extract_color(gmf_handle* h, const int* unit_keys, const int* unit_offsets, int G, int num_units, const float* tsdf,
                           const float* weight, const float* color, double voxel_length, float* points_out, float* colors_out,
                           long long max_points, int* point_offsets_out, long long* num_points, gmf_stream_t stream) {
  return tsdf_extract(h, "tsdf_extract_color", true, unit_keys, unit_offsets, G, num_units, tsdf, weight, color, voxel_length,
                      points_out, colors_out, max_points, point_offsets_out, num_points, stream);
}

int gmf_tsdf_extract_mesh(gmf_handle* h, const int* unit_keys, const int* unit_offsets, int G, int num_units, const float* tsdf,
                          const float* weight, const float* color, double voxel_length, float* points_out, float* normals_out,
                          float* colors_out, long long max_points, int* triangles_out, long long max_triangles, int* point_offsets_out,
                          int* triangle_offsets_out, long long* num_points, long long* num_triangles, gmf_stream_t stream) {
  const std::string w("tsdf_extract_mesh");
  const bool emit = points_out || normals_out || colors_out || triangles_out;
  GMF_REQUIRE(h && unit_offsets && point_offsets_out && triangle_offsets_out, GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(emit || (num_points && num_triangles), GMF_ERR_BAD_ARG,
              w + ": without outputs the call counts into num_points and num_triangles");
  GMF_REQUIRE(!emit || (points_out && normals_out && triangles_out && (!color == !colors_out)), GMF_ERR_BAD_ARG,
              w + ": points_out, normals_out and triangles_out are written together, and colors_out exactly with color");
  GMF_REQUIRE(G >= 1 && G <= gmf::kTsdfMaxFragments, GMF_ERR_UNSUPPORTED_SHAPE, w + ": G must be in 1..65535");
  GMF_REQUIRE(num_units >= 0 && num_units <= (1 << 22), GMF_ERR_BAD_ARG, w + ": num_units must be in 0..2^22");
  GMF_REQUIRE(num_units == 0 || (unit_keys && tsdf && weight), GMF_ERR_BAD_ARG, w + ": null pointer");
  GMF_REQUIRE(voxel_length > 0 && std::isfinite(voxel_length), GMF_ERR_BAD_ARG, w + ": voxel_length must be finite and > 0");
  GMF_REQUIRE(max_points >= 0 && max_triangles >= 0, GMF_ERR_BAD_ARG, w + ": max_points and max_triangles must be >= 0");
  SetDevice sd(h, stream);
  if (num_units == 0) {
    GMF_HIP(hipMemsetAsync(point_offsets_out, 0, ((size_t)G + 1) * 4, S(stream)));
    GMF_HIP(hipMemsetAsync(triangle_offsets_out, 0, ((size_t)G + 1) * 4, S(stream)));
    if (!emit) *num_points = *num_triangles = 0;
    return GMF_OK;
  }
  gmf::TsdfMeshScratch ws;
  ArenaList bufs;
  gmf::tsdf_mesh_scratch_list(num_units, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  int host_counts[2] = {0, 0};
  GMF_HIP(gmf::launch_tsdf_extract_mesh(unit_keys, unit_offsets, G, num_units, tsdf, weight, color, voxel_length, ws, points_out,
                                        normals_out, colors_out, max_points, triangles_out, max_triangles, point_offsets_out,
                                        triangle_offsets_out, host_counts, S(stream)));
  if (!emit) {
    *num_points = host_counts[0];
    *num_triangles = host_counts[1];
  }
  return GMF_OK;
}

int gmf_rgbd_pyramids(gmf_handle* h, const void* color, int color_kind, const void* depth, int depth_is_u16, int F, int H, int W,
                      double depth_scale, double depth_trunc, double min_depth, double max_depth, int levels, float* planes_out,
                      gmf_stream_t stream) {
  gmf::RgbdShape s;
  if (int rc = check_rgbd_shape(h, "rgbd_pyramids", F, H, W, levels, s)) return rc;
  GMF_REQUIRE(color && depth && planes_out, GMF_ERR_BAD_ARG, "rgbd_pyramids: null pointer");
  GMF_REQUIRE(color_kind >= gmf::kRgbdGray8 && color_kind <= gmf::kRgbdFloat, GMF_ERR_BAD_ARG,
              "rgbd_pyramids: color_kind must be 0 (uint8), 1 (uint8 RGB) or 2 (float32)");
  GMF_REQUIRE(depth_scale > 0 && std::isfinite(depth_scale) && depth_trunc > 0 && !std::isnan(depth_trunc), GMF_ERR_BAD_ARG,
              "rgbd_pyramids: depth_scale must be finite and > 0, depth_trunc > 0");
  GMF_REQUIRE(min_depth >= 0 && std::isfinite(min_depth) && max_depth > min_depth && !std::isnan(max_depth), GMF_ERR_BAD_ARG,
              "rgbd_pyramids: min_depth must be finite and >= 0, max_depth above it");
  SetDevice sd(h, stream);
  gmf::RgbdPyramidScratch ws;
  ArenaList bufs;
  gmf::rgbd_pyramid_scratch_list(s, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_rgbd_pyramids(color, color_kind, depth, depth_is_u16 != 0, s, (float)depth_scale, (float)depth_trunc,
                                    (float)min_depth, (float)max_depth, ws, planes_out, S(stream)));
  return GMF_OK;
}

int gmf_rgbd_correspondences(gmf_handle* h, const float* planes, int F, int H, int W, int levels, int level, const int* pair_source,
                             const int* pair_target, int E, const double* transformation, double fx, double fy, double cx, double cy,
                             double max_depth_diff, int* map_out, gmf_stream_t stream) {
  gmf::RgbdShape s;
  if (int rc = check_rgbd_shape(h, "rgbd_correspondences", F, H, W, levels, s)) return rc;
  if (int rc = check_rgbd_pairs(h, "rgbd_correspondences", planes, pair_source, pair_target, E, fx, fy, cx, cy, max_depth_diff)) return rc;
  GMF_REQUIRE(transformation && map_out, GMF_ERR_BAD_ARG, "rgbd_correspondences: null pointer");
  GMF_REQUIRE(level >= 0 && level < levels, GMF_ERR_BAD_ARG, "rgbd_correspondences: level must be in 0..levels-1");
  SetDevice sd(h, stream);
  gmf::RgbdOdometryScratch ws;
  ArenaList bufs;
  gmf::rgbd_odometry_scratch_list(s, E, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_rgbd_correspondences(planes, s, level, pair_source, pair_target, E, transformation, gmf::RgbdCamera{fx, fy, cx, cy},
                                           max_depth_diff, ws, map_out, S(stream)));
  return GMF_OK;
}

int gmf_rgbd_odometry(gmf_handle* h, const float* planes, int F, int H, int W, int levels, const int* pair_source, const int* pair_target,
                      int E, const double* odo_init, double fx, double fy, double cx, double cy, double max_depth_diff,
                      const int* iterations, unsigned char* success_out, double* transformation_out, double* information_out,
                      double* scales_out, int* trace_n_out, double* trace_out, gmf_stream_t stream) {
  gmf::RgbdShape s;
  if (int rc = check_rgbd_shape(h, "rgbd_odometry", F, H, W, levels, s)) return rc;
  if (int rc = check_rgbd_pairs(h, "rgbd_odometry", planes, pair_source, pair_target, E, fx, fy, cx, cy, max_depth_diff)) return rc;
  GMF_REQUIRE(iterations && success_out && transformation_out && information_out, GMF_ERR_BAD_ARG, "rgbd_odometry: null pointer");
  GMF_REQUIRE(!trace_n_out == !trace_out, GMF_ERR_BAD_ARG, "rgbd_odometry: trace_n_out and trace_out go together");
  for (int l = 0; l < levels; ++l)
    GMF_REQUIRE(iterations[l] >= 0 && iterations[l] <= 10000, GMF_ERR_BAD_ARG, "rgbd_odometry: iterations must be in 0..10000");
  SetDevice sd(h, stream);
  gmf::RgbdOdometryScratch ws;
  ArenaList bufs;
  gmf::rgbd_odometry_scratch_list(s, E, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_rgbd_odometry(planes, s, pair_source, pair_target, E, odo_init, gmf::RgbdCamera{fx, fy, cx, cy}, max_depth_diff,
                                    iterations, ws, success_out, transformation_out, information_out, scales_out, trace_n_out, trace_out,
                                    S(stream)));
  return GMF_OK;
}

int gmf_radius_knn(gmf_handle* h, const float* pts, const int* offsets, int B, long long total_rows, double radius, int max_nn,
                   int* idx, double* d2, int* count, gmf_stream_t stream) {
  if (int rc = check_cloud_args(h, "radius_knn", pts, offsets, B, total_rows, radius, max_nn)) return rc;
  GMF_REQUIRE(idx && count, GMF_ERR_BAD_ARG, "radius_knn: null pointer");
  SetDevice sd(h, stream);
  gmf::KnnScratch ws;
  ArenaList bufs;
  gmf::knn_scratch_list(total_rows, ws, bufs);
  if (int rc = arena_carve(h, bufs)) return rc;
  GMF_HIP(gmf::launch_radius_knn(pts, offsets, B, total_rows, radius, max_nn, ws, idx, d2, count, S(stream)));
  return GMF_OK;
}

int gmf_estimate_normals(gmf_handle* h, const float* pts, const int* offsets, int B, long long total_rows, double radius,
                         int max_nn, float* normals, gmf_stream_t stream) {
  if (int rc = check_cloud_args(h, "estimate_normals", pts, offsets, B, total_rows, radius, max_nn)) return rc;
  GMF_REQUIRE(normals, GMF_ERR_BAD_ARG, "estimate_normals: null pointer");
  SetDevice sd(h, stream);
  KnnLists k;
  if (int rc = take_knn(h, total_rows, max_nn, false, k)) return rc;
  GMF_HIP(gmf::launch_radius_knn(pts, offsets, B, total_rows, radius, max_nn, k.ws, k.idx, nullptr, k.count, S(stream)));
  GMF_HIP(gmf::launch_normals(pts, offsets, B, total_rows, k.idx, k.count, max_nn, normals, S(stream)));
  return GMF_OK;
}

int gmf_color_gradients(gmf_handle* h, const float* pts, const float* normals, const float* intensity, const int* offsets, int B,
                        long long total_rows, double radius, int max_nn, float* gradients, gmf_stream_t stream) {
  if (int rc = check_cloud_args(h, "color_gradients", pts, offsets, B, total_rows, radius, max_nn)) return rc;
  GMF_REQUIRE(normals && intensity && gradients, GMF_ERR_BAD_ARG, "color_gradients: null pointer");
  SetDevice sd(h, stream);
  KnnLists k;
  if (int rc = take_knn(h, total_rows, max_nn, false, k)) return rc;
  GMF_HIP(gmf::launch_radius_knn(pts, offsets, B, total_rows, radius, max_nn, k.ws, k.idx, nullptr, k.count, S(stream)));
  GMF_HIP(gmf::launch_color_gradient(pts, normals, intensity, offsets, B, total_rows, k.idx, k.count, max_nn, gradients,
                                     S(stream)));
  return GMF_OK;
}

int gmf_compute_fpfh(gmf_handle* h, const float* pts, const float* normals, const int* offsets, int B, long long total_rows,
                     double radius, int max_nn, float* features, gmf_stream_t stream) {
  if (int rc = check_cloud_args(h, "compute_fpfh", pts, offsets, B, total_rows, radius, max_nn)) return rc;
  GMF_REQUIRE(normals && features, GMF_ERR_BAD_ARG, "compute_fpfh: null pointer");
  SetDevice sd(h, stream);
  KnnLists k;
  if (int rc = take_knn(h, total_rows, max_nn, true, k)) return rc;
  GMF_HIP(gmf::launch_radius_knn(pts, offsets, B, total_rows, radius, max_nn, k.ws, k.idx, k.d2, k.count, S(stream)));
  GMF_HIP(gmf::launch_fpfh(pts, normals, offsets, B, total_rows, k.idx, k.d2, k.count, max_nn, k.spfh, features, S(stream)));
  return GMF_OK;
}

int gmf_voxel_down_sample(gmf_handle* h, const float* pts, const int* offsets, int B, long long total_rows, double voxel,
                          float* out_pts, int* out_offsets, long long* num_out, gmf_stream_t stream) {
  GMF_REQUIRE(out_pts, GMF_ERR_BAD_ARG, "voxel_down_sample: null pointer");
  return voxel_call(h, "voxel_down_sample", pts, offsets, B, total_rows, voxel, out_pts, nullptr, out_offsets, num_out, stream);
}

int gmf_voxel_down_sample_color(gmf_handle* h, const float* pts, const float* colors, const int* offsets, int B,
                                long long total_rows, double voxel, float* out_pts, float* out_colors, int* out_offsets,
                                long long* num_out, gmf_stream_t stream) {
  GMF_REQUIRE(out_pts && colors && out_colors, GMF_ERR_BAD_ARG, "voxel_down_sample_color: null pointer");
  return voxel_call(h, "voxel_down_sample_color", pts, offsets, B, total_rows, voxel, out_pts, nullptr, out_offsets, num_out, stream,
                    colors, out_colors);
}

int gmf_voxel_select(gmf_handle* h, const float* pts, const int* offsets, int B, long long total_rows, double voxel,
                     int* out_idx, int* out_offsets, long long* num_out, gmf_stream_t stream) {
  GMF_REQUIRE(out_idx, GMF_ERR_BAD_ARG, "voxel_select: null pointer");
  return voxel_call(h, "voxel_select", pts, offsets, B, total_rows, voxel, nullptr, out_idx, out_offsets, num_out, stream);
}

int gmf_similarity_matrix(gmf_handle* h, const float* feat_n, int B, int N, float sigma, float* M, int ldm,
                          gmf_stream_t stream) {
  GMF_REQUIRE(h && feat_n && M, GMF_ERR_BAD_ARG, "similarity_matrix: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "similarity_matrix: empty input");
  GMF_REQUIRE(ldm >= N, GMF_ERR_BAD_ARG, "similarity_matrix: ldm (row stride of M in floats) must be >= N");
  GMF_REQUIRE(sigma != 0.f || h->sigma_dev, GMF_ERR_BAD_ARG, "similarity_matrix: sigma must be non-zero");
  SetDevice sd(h, stream);
  const size_t n_img = gmf::similarity_image_floats(B, N);
  float* img;
  if (int rc = arena_carve(h, {arena_buf(img, n_img)})) return rc;
  GMF_HIP(gmf::launch_similarity_matrix(feat_n, img, M, B, N, ldm, sigma, S(stream), h->sigma_dev));
  return GMF_OK;
}

int gmf_spectral_matching_loss(gmf_handle* h, const float* M, int ldm, const float* gt_labels, int B, int N, int balanced,
                               float* loss_out, gmf_stream_t stream) {
  GMF_REQUIRE(h && M && gt_labels && loss_out, GMF_ERR_BAD_ARG, "spectral_matching_loss: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "spectral_matching_loss: empty input");
  GMF_REQUIRE(ldm >= N, GMF_ERR_BAD_ARG, "spectral_matching_loss: ldm (row stride of M in floats) must be >= N");
  SetDevice sd(h, stream);
  const size_t n_part = (size_t)2 * B * gmf::sm_parts_per_pair(B, N);
  double *part, *pair_loss;
  if (int rc = arena_carve(h, {arena_buf(part, n_part), arena_buf(pair_loss, (size_t)B)})) return rc;
  GMF_HIP(gmf::launch_sm_loss(M, ldm, gt_labels, part, pair_loss, B, N, balanced, loss_out, S(stream)));
  return GMF_OK;
}

int gmf_spectral_matching_loss_fused(gmf_handle* h, const float* feat_n, const float* gt_labels, int B, int N, float sigma,
                                     int balanced, float* loss_out, gmf_stream_t stream) {
  GMF_REQUIRE(h && feat_n && gt_labels && loss_out, GMF_ERR_BAD_ARG, "spectral_matching_loss_fused: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "spectral_matching_loss_fused: empty input");
  GMF_REQUIRE(sigma != 0.f || h->sigma_dev, GMF_ERR_BAD_ARG, "spectral_matching_loss_fused: sigma must be non-zero");
  SetDevice sd(h, stream);
  const size_t n_img = gmf::similarity_image_floats(B, N);
  const size_t n_part = (size_t)2 * B * gmf::sm_fused_parts_per_pair(B, N);
  float* img;
  double *part, *pair_loss;
  if (int rc = arena_carve(h, {arena_buf(img, n_img), arena_buf(part, n_part), arena_buf(pair_loss, (size_t)B)})) return rc;
  GMF_HIP(gmf::launch_sm_loss_fused(feat_n, gt_labels, img, part, pair_loss, B, N, sigma, balanced, loss_out, S(stream), h->sigma_dev));
  return GMF_OK;
}

int gmf_spectral_matching_backward(gmf_handle* h, const float* feat_n, const float* gt_labels, int B, int N, float sigma,
                                   int balanced, float* d_feat_n, float* d_sigma, gmf_stream_t stream) {
  GMF_REQUIRE(h && feat_n && gt_labels && d_feat_n && d_sigma, GMF_ERR_BAD_ARG, "spectral_matching_backward: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "spectral_matching_backward: empty input");
  GMF_REQUIRE(sigma != 0.f || h->sigma_dev, GMF_ERR_BAD_ARG, "spectral_matching_backward: sigma must be non-zero");
  SetDevice sd(h, stream);
  const size_t n_img = gmf::similarity_image_floats(B, N);
  const size_t n_part = (size_t)gmf::sm_backward_parts(B, N);
  float *img, *timg, *consts;
  double* part;
  if (int rc = arena_carve(h, {arena_buf(img, n_img), arena_buf(timg, n_img), arena_buf(consts, (size_t)4 * B), arena_buf(part, n_part)}))
    return rc;
  GMF_HIP(gmf::launch_sm_backward(feat_n, gt_labels, img, timg, consts, part, B, N, sigma, balanced, d_feat_n, d_sigma, S(stream), h->sigma_dev));
  return GMF_OK;
}

int gmf_classification_loss(gmf_handle* h, const float* pred, const float* gt, const float* weight, int B, int N,
                            int balanced, float* out6, gmf_stream_t stream) {
  GMF_REQUIRE(h && pred && gt && out6, GMF_ERR_BAD_ARG, "classification_loss: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "classification_loss: empty input");
  SetDevice sd(h, stream);
  const size_t n_part = (size_t)9 * gmf::classification_parts(B, N);
  double* part;
  if (int rc = arena_carve(h, {arena_buf(part, n_part)})) return rc;
  GMF_HIP(gmf::launch_classification_loss(pred, gt, weight, part, B, N, balanced, out6, S(stream)));
  return GMF_OK;
}

int gmf_transformation_loss(gmf_handle* h, const float* trans, const float* gt_trans, const float* src_keypts,
                            const float* tgt_keypts, const float* probs, int B, int N, float re_thre, float te_thre,
                            float* out5, gmf_stream_t stream) {
  GMF_REQUIRE(h && trans && gt_trans && src_keypts && tgt_keypts && probs && out5, GMF_ERR_BAD_ARG,
              "transformation_loss: null pointer");
  GMF_REQUIRE(B > 0 && N > 0, GMF_ERR_UNSUPPORTED_SHAPE, "transformation_loss: empty input");
  SetDevice sd(h, stream);
  const size_t n_part = (size_t)3 * B * gmf::transformation_slices(B, N);
  double* part;
  if (int rc = arena_carve(h, {arena_buf(part, n_part)})) return rc;
  GMF_HIP(gmf::launch_transformation_loss(trans, gt_trans, src_keypts, tgt_keypts, probs, part, B, N, re_thre, te_thre,
                                          out5, S(stream)));
  return GMF_OK;
}

int gmf_bias_relu_nhwc(gmf_handle* h, float* y, const float* bias, const float* residual, long long n_pixels, int C,
                       gmf_stream_t stream) {
  GMF_REQUIRE(h && y && bias, GMF_ERR_BAD_ARG, "bias_relu_nhwc: null pointer");
  GMF_REQUIRE(n_pixels > 0 && C > 0 && C % 4 == 0, GMF_ERR_UNSUPPORTED_SHAPE, "bias_relu_nhwc: need n_pixels > 0 and C a positive multiple of 4");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_bias_relu_nhwc(y, bias, residual, (long)n_pixels, C, S(stream)));
  return GMF_OK;
}

int gmf_stem_forward(gmf_handle* h, const float* x, long long sb, long long sc, long long sh, long long sw, const float* wimg,
                     const float* bias, float* y, int B, int H, int W, gmf_stream_t stream) {
  GMF_REQUIRE(h && x && wimg && bias && y, GMF_ERR_BAD_ARG, "stem_forward: null pointer");
  GMF_REQUIRE(B > 0 && H > 0 && W > 0, GMF_ERR_UNSUPPORTED_SHAPE, "stem_forward: empty input");
  GMF_REQUIRE(B <= 65535, GMF_ERR_UNSUPPORTED_SHAPE, "stem_forward: at most 65535 images per call");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_stem_h2(x, (long)sb, (long)sc, (long)sh, (long)sw, wimg, bias, y, B, H, W, S(stream), h->tune.conv_small));
  return GMF_OK;
}

int gmf_conv_nhwc(gmf_handle* h, const float* x, const float* wimg, const float* bias, const float* residual, float* y,
                  int B, int H, int W, int cin, int cout, int ksize, int stride, int relu, gmf_stream_t stream) {
  GMF_REQUIRE(h && x && wimg && bias && y, GMF_ERR_BAD_ARG, "conv_nhwc: null pointer");
  GMF_REQUIRE(B > 0 && H > 0 && W > 0, GMF_ERR_UNSUPPORTED_SHAPE, "conv_nhwc: empty input");
  const bool known = (cin == 64 && cout == 64 && ksize == 3 && stride == 1) || (cin == 64 && cout == 128 && ksize == 3 && stride == 2) ||
                     (cin == 128 && cout == 128 && ksize == 3 && stride == 1) || (cin == 64 && cout == 128 && ksize == 1 && stride == 2);
  GMF_REQUIRE(known, GMF_ERR_UNSUPPORTED_SHAPE,
              "conv_nhwc: supported are the ResNet-34 layer1 / layer2 shapes (64->64 3x3 s1, 64->128 3x3 s2, 128->128 3x3 s1, 64->128 1x1 s2)");
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_conv_nhwc_h2(h->tune, x, wimg, bias, residual, y, B, H, W, cin, cout, ksize, stride, relu, S(stream)));
  return GMF_OK;
}

}  // extern "C"

// ---- sparse coordinate engine, sparse convolution, ResUNetBN2C weight pack ------------------------------------------------

namespace {

int sparse_layout(gmf_handle* h, long long M, int D, int levels, int num_maps, const int* maps, gmf::SparsePlanLayout& lay) {
  GMF_REQUIRE(h && (maps || num_maps == 0), GMF_ERR_BAD_ARG, "sparse plan: null pointer");
  GMF_REQUIRE(D >= 1 && D <= gmf::kSparseMaxD, GMF_ERR_UNSUPPORTED_SHAPE, "sparse plan: D must be in 1..6");
  GMF_REQUIRE(M >= 1 && M < (1LL << 28), GMF_ERR_UNSUPPORTED_SHAPE, "sparse plan: the row count must be in 1 .. 2^28 - 1");
  GMF_REQUIRE(levels >= 1 && levels <= gmf::kSparseMaxLevels && num_maps >= 0 && num_maps <= gmf::kSparseMaxMaps,
              GMF_ERR_UNSUPPORTED_SHAPE, "sparse plan: 1..8 levels and 0..16 kernel maps");
  gmf::SparseMapDesc d[gmf::kSparseMaxMaps];
  for (int m = 0; m < num_maps; ++m) d[m] = {maps[3 * m], maps[3 * m + 1], maps[3 * m + 2]};
  GMF_REQUIRE(gmf::sparse_plan_layout(M, D, levels, num_maps, d, lay), GMF_ERR_UNSUPPORTED_SHAPE,
              "sparse plan: a kernel map needs an odd kernel size with k^D <= 1024, levels that exist and differ by at most one, "
              "and fewer than 2^31 pairs (rows x k^D)");
  return GMF_OK;
}

// The convolutions of ResUNetBN2C (resunet_new.py:424-721) in forward order: (kernel key, BatchNorm prefix or "", bias key or "")
struct ResunetLayer { const char* conv; const char* norm; const char* bias; };
const ResunetLayer kResunetLayers[GMF_SPARSE_RESUNET_LAYERS] = {
    {"conv1", "norm1", ""},
    {"block1.conv1", "block1.norm1", ""}, {"block1.conv2", "block1.norm2", ""},
    {"conv2", "norm2", ""},
    {"block2.conv1", "block2.norm1", ""}, {"block2.conv2", "block2.norm2", ""},
    {"conv3", "norm3", ""},
    {"block3.conv1", "block3.norm1", ""}, {"block3.conv2", "block3.norm2", ""},
    {"conv4", "norm4", ""},
    {"block4.conv1", "block4.norm1", ""}, {"block4.conv2", "block4.norm2", ""},
    {"conv4_tr", "norm4_tr", ""},
    {"block4_tr.conv1", "block4_tr.norm1", ""}, {"block4_tr.conv2", "block4_tr.norm2", ""},
    {"conv3_tr", "norm3_tr", ""},
    {"block3_tr.conv1", "block3_tr.norm1", ""}, {"block3_tr.conv2", "block3_tr.norm2", ""},
    {"conv2_tr", "norm2_tr", ""},
    {"block2_tr.conv1", "block2_tr.norm1", ""}, {"block2_tr.conv2", "block2_tr.norm2", ""},
    {"conv1_tr", "", ""},
    {"final", "", "final.bias"},
};

const gmf_tensor* find_tensor(const gmf_tensor* t, int n, const std::string& name) {
  for (int i = 0; i < n; ++i)
    if (t[i].name && name == t[i].name) return &t[i];
  return nullptr;
}

}  // namespace

extern "C" {

int gmf_sparse_plan_bytes(gmf_handle* h, long long M, int D, int levels, int num_maps, const int* maps, long long* bytes) {
  GMF_REQUIRE(bytes, GMF_ERR_BAD_ARG, "sparse_plan_bytes: null pointer");
  gmf::SparsePlanLayout lay;
  if (int rc = sparse_layout(h, M, D, levels, num_maps, maps, lay)) return rc;
  *bytes = (long long)lay.total;
  return GMF_OK;
}

int gmf_sparse_build_plan(gmf_handle* h, const int* coords, long long M, int D, int levels, int num_maps, const int* maps,
                          void* plan, long long plan_bytes, long long* offsets, gmf_stream_t stream) {
  GMF_REQUIRE(h && coords && plan && offsets, GMF_ERR_BAD_ARG, "sparse_build_plan: null pointer");
  gmf::SparsePlanLayout lay;
  if (int rc = sparse_layout(h, M, D, levels, num_maps, maps, lay)) return rc;
  GMF_REQUIRE(plan_bytes >= (long long)lay.total, GMF_ERR_BAD_ARG, "sparse_build_plan: the plan block is smaller than gmf_sparse_plan_bytes");
  int k = 0;
  offsets[k++] = (long long)lay.counts;
  for (int l = 0; l < levels; ++l) offsets[k++] = (long long)lay.coords[l];
  for (int m = 0; m < num_maps; ++m) {
    offsets[k++] = (long long)lay.row_ptr[m];
    offsets[k++] = (long long)lay.pairs[m];
    offsets[k++] = (long long)lay.by_off[m];
    offsets[k++] = (long long)lay.off_start[m];
  }
  SetDevice sd(h, stream);
  GMF_HIP(gmf::launch_sparse_build_plan(coords, lay, static_cast<char*>(plan), h->status_dev, GMF_STATUS_SPARSE_DUPLICATE,
                                        S(stream)));
  return GMF_OK;
}

int gmf_sparse_conv(gmf_handle* h, const int* row_ptr, const int* pairs, const int* by_off, const int* off_start, int K,
                    const int* n_out, long long cap_out,
                    const float* xa, int ca, const float* xb, int cb, const float* W, int cout, const float* scale,
                    const float* shift, const float* residual, int relu, int nsplit, float* y, gmf_stream_t stream) {
  GMF_REQUIRE(h && n_out && xa && W && y, GMF_ERR_BAD_ARG, "sparse_conv: null pointer");
  GMF_REQUIRE((row_ptr == nullptr) == (pairs == nullptr) && (row_ptr == nullptr) == (by_off == nullptr) &&
                  (row_ptr == nullptr) == (off_start == nullptr),
              GMF_ERR_BAD_ARG, "sparse_conv: row_ptr, pairs, by_off and off_start go together");
  GMF_REQUIRE(K >= 1 && K <= gmf::kSparseMaxK && (row_ptr || K == 1), GMF_ERR_UNSUPPORTED_SHAPE,
              "sparse_conv: K must be in 1..1024 (1 for the identity map)");
  GMF_REQUIRE(cap_out >= 1 && cap_out < (1LL << 28), GMF_ERR_UNSUPPORTED_SHAPE, "sparse_conv: cap_out must be in 1 .. 2^28 - 1");
  GMF_REQUIRE(ca >= 1 && cb >= 0 && (cb == 0 || xb) && cout >= 1 && ca + cb <= 4096 && cout <= 4096, GMF_ERR_UNSUPPORTED_SHAPE,
              "sparse_conv: channel counts must be in 1..4096 (cb may be 0)");
  GMF_REQUIRE(nsplit >= 1 && nsplit <= K, GMF_ERR_BAD_ARG, "sparse_conv: nsplit must be in 1..K");
  SetDevice sd(h, stream);
  GMF_REQUIRE(row_ptr || nsplit == 1, GMF_ERR_BAD_ARG, "sparse_conv: the identity map takes nsplit = 1");
  gmf::SparseConvArgs a{row_ptr, reinterpret_cast<const int2*>(pairs), by_off, off_start, K, n_out, cap_out, xa, ca,
                        cb ? xb : nullptr, cb, W, cout, scale, shift, residual, relu, nsplit, nullptr, y};
  if (row_ptr)
    if (int rc = arena_carve(h, {arena_buf(a.partial, (size_t)nsplit * cap_out * cout)})) return rc;
  GMF_HIP(gmf::launch_sparse_conv(a, S(stream)));
  return GMF_OK;
}

int gmf_sparse_conv_narrow(gmf_handle* h, const int* row_ptr, const int* pairs, int K, const int* n_out, long long cap_out,
                           const float* x, int cin, const float* W, int cout, const float* scale, const float* shift,
                           const float* residual, int relu, float* y, gmf_stream_t stream) {
  GMF_REQUIRE(h && row_ptr && pairs && n_out && x && W && y, GMF_ERR_BAD_ARG, "sparse_conv_narrow: null pointer");
  GMF_REQUIRE(K >= 1 && K <= gmf::kSparseMaxK, GMF_ERR_UNSUPPORTED_SHAPE, "sparse_conv_narrow: K must be in 1..1024");
  GMF_REQUIRE(cap_out >= 1 && cap_out < (1LL << 28), GMF_ERR_UNSUPPORTED_SHAPE,
              "sparse_conv_narrow: cap_out must be in 1 .. 2^28 - 1");
  GMF_REQUIRE(cin >= 1 && cin <= gmf::kSparseNarrowMaxCin && cout >= 1 && cout <= gmf::kSparseNarrowMaxCout,
              GMF_ERR_UNSUPPORTED_SHAPE, "sparse_conv_narrow: Cin must be in 1..8 and Cout in 1..64");
  SetDevice sd(h, stream);
  gmf::SparseNarrowArgs a{row_ptr, reinterpret_cast<const int2*>(pairs), K, n_out, cap_out, x, cin, W, cout, scale, shift,
                          residual, relu, y};
  GMF_HIP(gmf::launch_sparse_conv_narrow(a, S(stream)));
  return GMF_OK;
}

int gmf_sparse_head_l2(gmf_handle* h, const int* n_out, long long cap_out, const float* xa, int ca, const float* xb, int cb,
                       const float* W1, int hid, const float* W2, int cout, const float* bias, int normalize, float* y,
                       gmf_stream_t stream) {
  GMF_REQUIRE(h && n_out && xa && W1 && W2 && y && (cb == 0 || xb), GMF_ERR_BAD_ARG, "sparse_head_l2: null pointer");
  GMF_REQUIRE(cap_out >= 1 && cap_out < (1LL << 28), GMF_ERR_UNSUPPORTED_SHAPE, "sparse_head_l2: cap_out must be in 1 .. 2^28 - 1");
  constexpr int C = gmf::kSparseHeadMaxC;
  GMF_REQUIRE(ca >= 1 && ca <= C && cb >= 0 && cb <= C && hid >= 1 && hid <= C && cout >= 1 && cout <= C,
              GMF_ERR_UNSUPPORTED_SHAPE, "sparse_head_l2: ca, hid and cout must be in 1..64, cb in 0..64");
  SetDevice sd(h, stream);
  gmf::SparseHeadArgs a{n_out, cap_out, xa, ca, cb ? xb : nullptr, cb, W1, hid, W2, cout, bias, normalize ? 1 : 0, y};
  GMF_HIP(gmf::launch_sparse_head_l2(a, S(stream)));
  return GMF_OK;
}

int gmf_sparse_pack_resunet(gmf_handle* h, const gmf_tensor* tensors, int n_tensors, float* dev, long long dev_floats,
                            long long* layout, long long* need_floats) {
  GMF_REQUIRE(h && tensors && layout && need_floats, GMF_ERR_BAD_ARG, "sparse_pack_resunet: null pointer");
  std::vector<float> blob;
  auto put = [&](size_t n) { const size_t o = blob.size(); blob.resize(o + (n + 63) / 64 * 64, 0.f); return o; };
  for (int i = 0; i < GMF_SPARSE_RESUNET_LAYERS; ++i) {
    const ResunetLayer& L = kResunetLayers[i];
    const std::string kname = std::string(L.conv) + ".kernel";
    const gmf_tensor* kt = find_tensor(tensors, n_tensors, kname);
    GMF_REQUIRE(kt && kt->data, GMF_ERR_BAD_ARG, "sparse_pack_resunet: missing " + kname);
    // MinkowskiEngine's kernel: [k^D, Cin, Cout], or [Cin, Cout] when k^D = 1 (assumptions)
    GMF_REQUIRE(kt->ndim == 3 || kt->ndim == 2, GMF_ERR_BAD_ARG, "sparse_pack_resunet: " + kname + " must be [K, Cin, Cout] or [Cin, Cout]");
    const long long K = kt->ndim == 3 ? kt->shape[0] : 1;
    const long long cin = kt->ndim == 3 ? kt->shape[1] : kt->shape[0];
    const long long cout = kt->ndim == 3 ? kt->shape[2] : kt->shape[1];
    GMF_REQUIRE(K >= 1 && K <= gmf::kSparseMaxK && cin >= 1 && cout >= 1, GMF_ERR_UNSUPPORTED_SHAPE,
                "sparse_pack_resunet: " + kname + " has an unsupported shape");
    const size_t wo = put((size_t)(K * cin * cout));
    std::copy(kt->data, kt->data + K * cin * cout, blob.begin() + wo);
    long long so = -1, ho = -1;
    if (*L.norm) {
      const std::string p = std::string(L.norm) + ".bn.";
      const gmf_tensor* g = find_tensor(tensors, n_tensors, p + "weight");
      const gmf_tensor* b = find_tensor(tensors, n_tensors, p + "bias");
      const gmf_tensor* mu = find_tensor(tensors, n_tensors, p + "running_mean");
      const gmf_tensor* var = find_tensor(tensors, n_tensors, p + "running_var");
      GMF_REQUIRE(g && b && mu && var, GMF_ERR_BAD_ARG, "sparse_pack_resunet: missing " + p + "{weight,bias,running_mean,running_var}");
      for (const gmf_tensor* t : {g, b, mu, var})
        GMF_REQUIRE(t->ndim == 1 && t->shape[0] == cout, GMF_ERR_BAD_ARG, "sparse_pack_resunet: " + p + "* must be [" + std::to_string(cout) + "]");
      so = (long long)put((size_t)cout);
      ho = (long long)put((size_t)cout);
      for (long long c = 0; c < cout; ++c) {   // eval BatchNorm1d, eps 1e-5, folded in fp64
        const double sc = (double)g->data[c] / std::sqrt((double)var->data[c] + 1e-5);
        blob[so + c] = (float)sc;
        blob[ho + c] = (float)((double)b->data[c] - (double)mu->data[c] * sc);
      }
    } else if (*L.bias) {
      const gmf_tensor* b = find_tensor(tensors, n_tensors, L.bias);
      // MinkowskiEngine's bias: [1, Cout] (assumptions)
      GMF_REQUIRE(b && b->data && b->ndim == 2 && b->shape[0] == 1 && b->shape[1] == cout, GMF_ERR_BAD_ARG,
                  std::string("sparse_pack_resunet: ") + L.bias + " must be [1, " + std::to_string(cout) + "]");
      ho = (long long)put((size_t)cout);
      std::copy(b->data, b->data + cout, blob.begin() + ho);
    }
    long long* e = layout + 6 * i;
    e[0] = (long long)wo; e[1] = so; e[2] = ho; e[3] = K; e[4] = cin; e[5] = cout;
  }
  *need_floats = (long long)blob.size();
  if (!dev) return GMF_OK;
  GMF_REQUIRE(dev_floats >= (long long)blob.size(), GMF_ERR_BAD_ARG, "sparse_pack_resunet: the device block is too small");
  SetDevice sd(h);
  GMF_HIP(hipMemcpy(dev, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice));
  return GMF_OK;
}

}  // extern "C"
