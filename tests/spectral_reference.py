"""A float64 numpy restatement of the spectral-matching baseline of gmf_amd/spectral.py (`spectral_matching_batched`, `SM`; kernels
csrc/spectral_kernels.hip), and the fp32 floor of the reference's own arithmetic.  Per pair of N correspondences:

  1. d_ij = |c_i[0:3] - c_j[0:3]| - |c_i[3:6] - c_j[3:6]| (coordinate differences, then the root of the sum of squares)
  2. sigma = inlier_threshold / 3, m_ij = max(0, 4.5 - d_ij^2 / 2 / sigma^2), m_ii = 0
  3. v = ones; `iterations` times: v = M v; v = v / (|v|_2 + 1e-6)
  4. k = int(N * top_ratio); labels = 1 on the k rows of largest v, equal values to the smaller row
  5. T = rigid_transform_3d(src, tgt, v * labels): weights not normalised, centroids over sum w + 1e-6, R = V diag(1, 1, det) U^T

`floor(case)` runs the same steps in fp32 torch on the CPU in the reference's dense form (the [N, N] matrix, `bmm`, `argsort`)
and compares with the fp64 result: that is what the reference's own arithmetic is worth on the case, and the unit in which
tests/test_gpu_spectral.py bounds the device.  Nothing here is code under test."""
import functools

import numpy as np
import torch

from gmf_amd import synthetic

KINDS = {"3dmatch": (0.10, 0.1), "kitti": (0.6, 0.05)}      # kind -> (inlier_threshold, top_ratio)


def make_case(seed, N, kind):
    """(corr [N,6], src [N,3], tgt [N,3], inlier_threshold, top_ratio) of synthetic_pair(seed, N, kind), float32."""
    p = synthetic.synthetic_pair(seed, N, kind)
    thr, ratio = KINDS[kind]
    return p["corr_pos"], p["src_keypts"], p["tgt_keypts"], thr, ratio


def matrix_np(corr, thr):
    c = np.asarray(corr, np.float64)
    diff = c[:, None, :] - c[None, :, :]
    d = np.sqrt((diff[..., 0:3] ** 2).sum(-1)) - np.sqrt((diff[..., 3:6] ** 2).sum(-1))
    sigma = thr / 3
    M = np.maximum(0.0, 4.5 - d ** 2 / 2 / sigma ** 2)
    np.fill_diagonal(M, 0.0)
    return M


def eig_np(corr, thr, iterations=10):
    M = matrix_np(corr, thr)
    v = np.ones(M.shape[0])
    for _ in range(iterations):
        v = M @ v
        v = v / (np.sqrt((v ** 2).sum()) + 1e-6)
    return v


def labels_np(v, k):
    """1 on the k largest entries of v; equal values go to the smaller index."""
    order = np.argsort(-np.asarray(v, np.float64), kind="stable")
    lab = np.zeros(len(v))
    lab[order[:k]] = 1
    return lab


def pose_np(src, tgt, w):
    """Step 5 in float64 on the given weights -> [4,4]."""
    A, B, w = np.asarray(src, np.float64), np.asarray(tgt, np.float64), np.asarray(w, np.float64)
    den = w.sum() + 1e-6
    ca, cb = (A * w[:, None]).sum(0) / den, (B * w[:, None]).sum(0) / den
    H = (A - ca).T @ (w[:, None] * (B - cb))
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.diag([1.0, 1.0, np.linalg.det(V @ U.T)])
    R = V @ D @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, cb - R @ ca
    return T


def sm_np(corr, src, tgt, thr, ratio, iterations=10):
    """The five steps in float64 -> dict(eig [N], labels [N], trans [4,4], k, gap).  gap: v's k-th largest value minus its
    (k+1)-th, relative to max v (inf when k is 0 or N): how far the labels are from a tie."""
    N = len(corr)
    v = eig_np(corr, thr, iterations) if N else np.zeros(0)
    k = int(N * ratio)
    lab = labels_np(v, k)
    s = np.sort(v)[::-1]
    gap = float((s[k - 1] - s[k]) / s[0]) if 0 < k < N and s[0] > 0 else float("inf")
    return {"eig": v, "labels": lab, "trans": pose_np(src, tgt, v * lab), "k": k, "gap": gap}


def pose_t32(src, tgt, w):
    """Step 5 in fp32 torch, as the reference writes it (SVD of the 3 x 3 on the CPU) -> [4,4] float32 numpy."""
    A, B, w = (torch.as_tensor(np.asarray(x, np.float32)) for x in (src, tgt, w))
    den = w.sum() + 1e-6
    ca, cb = (A * w[:, None]).sum(0) / den, (B * w[:, None]).sum(0) / den
    H = (A - ca).T @ torch.diag_embed(w) @ (B - cb)
    U, _, V = torch.svd(H)
    D = torch.eye(3)
    D[2, 2] = torch.det(V @ U.T)
    R = V @ D @ U.T
    T = torch.eye(4)
    T[:3, :3], T[:3, 3] = R, cb - R @ ca
    return T.numpy()


def sm_t32(corr, src, tgt, thr, ratio, iterations=10):
    """The five steps in fp32 torch on the CPU in the reference's dense form -> dict(eig, labels, trans) float32 numpy."""
    c = torch.as_tensor(np.asarray(corr, np.float32))
    diff = c[:, None, :] - c[None, :, :]
    M = (diff[..., 0:3] ** 2).sum(-1) ** 0.5 - (diff[..., 3:6] ** 2).sum(-1) ** 0.5
    sigma = thr / 3
    M = torch.max(torch.zeros_like(M), 4.5 - M ** 2 / 2 / sigma ** 2)
    M.fill_diagonal_(0)
    v = torch.ones(len(c), 1)
    for _ in range(iterations):
        v = M @ v
        v = v / (torch.norm(v) + 1e-6)
    v = v[:, 0]
    lab = torch.zeros_like(v)
    lab[torch.argsort(v, descending=True)[:int(len(c) * ratio)]] = 1
    return {"eig": v.numpy(), "labels": lab.numpy(), "trans": pose_t32(src, tgt, (v * lab).numpy())}


def eig_error(eig, eig64):
    """max |eig - eig64| / max eig64: the measure of the eigenvector tests."""
    return float(np.abs(np.asarray(eig, np.float64) - eig64).max() / eig64.max())


@functools.lru_cache(maxsize=None)
def reference(seed, N, kind, iterations=10):
    """(case, sm_np result, sm_t32 result) of one named case, computed once per process.  Treat as read-only."""
    case = make_case(seed, N, kind)
    return case, sm_np(*case, iterations=iterations), sm_t32(*case, iterations=iterations)


def floor(case_key):
    """The fp32 floor of the eigenvector on case (seed, N, kind): eig_error of the reference's dense fp32 form."""
    _, r64, r32 = reference(*case_key)
    return eig_error(r32["eig"], r64["eig"])


def pose_floor(src, tgt, w):
    """The fp32 floor of step 5 on the given input: max |T32 - T64|."""
    return float(np.abs(pose_t32(src, tgt, w).astype(np.float64) - pose_np(src, tgt, w)).max())


def self_test():
    """The restatement's edge cases: N = 1, k = 0, an all-incompatible pair, and a tie."""
    one = sm_np(np.zeros((1, 6), np.float32), np.ones((1, 3), np.float32), np.ones((1, 3), np.float32), 0.1, 0.1)
    assert one["k"] == 0 and one["eig"][0] == 0 and not one["labels"].any() and np.array_equal(one["trans"], np.eye(4))
    c, s, t, thr, ratio = make_case(3, 5, "3dmatch")
    few = sm_np(c, s, t, thr, ratio)
    assert few["k"] == 0 and not few["labels"].any() and np.allclose(few["trans"], np.eye(4), atol=0)
    # all incompatible: the source rows on a line 1 apart, the target rows 100 apart: every |d| >> 3 sigma, M = 0, v = 0
    a = np.zeros((8, 3)); a[:, 0] = np.arange(8)
    b = np.zeros((8, 3)); b[:, 1] = 100 * np.arange(8)
    bad = sm_np(np.concatenate([a, b], 1), a, b, 0.1, 0.5)
    assert bad["k"] == 4 and not bad["eig"].any() and bad["labels"].sum() == 4 and np.array_equal(bad["trans"], np.eye(4))
    assert np.array_equal(labels_np(np.array([0.5, 0.7, 0.5, 0.5]), 2), [1, 1, 0, 0])      # a tie goes to the smaller index
    return True
