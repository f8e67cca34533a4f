"""CPU-side checks of the descriptor stages (gmf_amd/features.py): the numpy restatement the GPU tests hold the kernels to
(tests/fpfh_reference.py) against numpy.linalg and geometric invariants, the public names, their argument checks, the
no-device error, and the C ABI entries."""
import os
import re

import numpy as np
import pytest
import torch

import fpfh_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["radius_knn_batched", "estimate_normals_batched", "compute_fpfh_batched", "voxel_down_sample_batched",
         "voxel_select_batched", "voxel_down_sample", "voxel_select", "estimate_normals", "compute_fpfh_feature",
         "fpfh_descriptors"]
ABI = ["gmf_radius_knn", "gmf_estimate_normals", "gmf_compute_fpfh", "gmf_voxel_down_sample", "gmf_voxel_select"]


def _pack(S):
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)


def _random_rotations(r, n):
    q, _ = np.linalg.qr(r.normal(size=(n, 3, 3)))
    return q * np.sign(np.linalg.det(q))[:, None, None]


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------

def test_eigensolver_against_eigh():
    r = np.random.default_rng(0)
    Q = _random_rotations(r, 3000)
    lam = np.sort(r.uniform(0.01, 1.0, (3000, 3)), 1)
    lam[1000:2000, 0] = 0.0                              # rank 2 (a plane)
    S = Q @ (lam[:, :, None] * np.swapaxes(Q, 1, 2))
    S = 0.5 * (S + np.swapaxes(S, 1, 2))
    v = R.fast_eigen3x3(_pack(S))
    w, U = np.linalg.eigh(S)
    clear = (w[:, 1] - w[:, 0]) > 1e-3 * w[:, 2]
    assert clear.mean() > 0.95
    cos = np.abs((v * U[:, :, 0]).sum(1))
    assert np.all(cos[clear] > 1 - 1e-9), cos[clear].min()
    assert np.allclose((v * v).sum(1), 1, atol=1e-12)
    # a fixed sign: the same matrices give the same vectors, bit for bit
    assert np.array_equal(v, R.fast_eigen3x3(_pack(S)))


def test_eigensolver_diagonal_and_zero():
    A = np.array([[3, 0, 0, 1, 0, 2],      # diag (3, 1, 2): y
                  [1, 0, 0, 2, 0, 3],      # x
                  [2, 0, 0, 3, 0, 1],      # z
                  [1, 0, 0, 1, 0, 1],      # all equal: ties go to z
                  [1, 0, 0, 1, 0, 2],      # x and y tie below z: z (neither is strictly smallest)
                  [0, 0, 0, 0, 0, 0]], np.float64)
    v = R.fast_eigen3x3(A)
    assert np.array_equal(v, [[0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0]])


def test_plane_gives_z_normals():
    r = np.random.default_rng(1)
    P = np.c_[r.uniform(0, 1, (2000, 2)), np.zeros(2000)].astype(np.float32)
    n, _, cnt = R.estimate_normals(P, None, 0.08, 30)
    assert (cnt >= 3).all()
    assert np.allclose(np.abs(n[:, 2]), 1, atol=1e-12) and np.allclose(n[:, :2], 0, atol=1e-9)


def test_search_order_and_boundary():
    # a row at exactly the radius is outside; ties in d^2 go to the smaller row
    P = np.array([[0, 0, 0], [0.25, 0, 0], [0, 0.125, 0], [0, -0.125, 0], [0.2, 0, 0]], np.float32)
    idx, d2, cnt = R.radius_knn(P, None, 0.25, 8)
    assert cnt[0] == 4 and list(idx[0, :4]) == [0, 2, 3, 4] and idx[0, 4] == -1
    assert d2[0, 1] == d2[0, 2] == 0.015625
    idx, _, cnt = R.radius_knn(P, None, 0.25, 2)
    assert cnt[0] == 2 and list(idx[0]) == [0, 2]
    # two clouds never mix
    idx, _, cnt = R.radius_knn(np.concatenate([P, P]), [0, 5, 10], 0.3, 8)
    assert (idx[5:] < 5).all() and np.array_equal(cnt[:5], cnt[5:])


def _cloud(r, n=1500):
    # a few noisy planes and a sphere: normals with clear eigen-gaps
    a = np.c_[r.uniform(0, 1, (n, 2)), 0.002 * r.normal(size=n)]
    b = np.c_[0.002 * r.normal(size=n), r.uniform(0, 1, (n, 2))]
    s = r.normal(size=(n, 3))
    s = 0.3 * s / np.linalg.norm(s, axis=1, keepdims=True) + 0.5
    return np.concatenate([a, b, s]).astype(np.float32)


def test_fpfh_block_sums_and_rotation_invariance():
    r = np.random.default_rng(2)
    P = _cloud(r)
    rad_n, rad_f = 0.06, 0.15
    n0, _, _ = R.estimate_normals(P, None, rad_n, 30)
    lists0 = R.radius_knn(P, None, rad_f, 256)
    f0, bound0 = R.fpfh(P, n0.astype(np.float32), None, rad_f, 256, lists=lists0, edge_tol=1e-5)
    has = (lists0[1] > 0).any(1)
    sums = f0.reshape(-1, 3, 11).sum(2)
    assert np.allclose(sums[has], 200, atol=1e-9)
    assert (f0[~has] == f0[~has]).all()
    # rotated about the origin: the normals agree up to sign where the eigen-gap is clear, and with the rotated normals of the
    # original (the same signs) the features agree wherever the neighbourhoods do, up to what pairs near a bin edge may move
    # (the rotated fp32 coordinates move the pair features by ~1e-7, hence the wider edge band)
    Rot = _random_rotations(r, 1)[0]
    Q = (P.astype(np.float64) @ Rot.T).astype(np.float32)
    n1, A1, _ = R.estimate_normals(Q, None, rad_n, 30)
    w = np.linalg.eigvalsh(R.sym(A1))
    clear = (w[:, 1] - w[:, 0]) > 1e-2 * w[:, 2]
    assert clear.mean() > 0.9
    assert np.all(np.abs((n1 * (n0 @ Rot.T)).sum(1))[clear] > 1 - 1e-6)
    nr = (n0 @ Rot.T).astype(np.float32)
    lists1 = R.radius_knn(Q, None, rad_f, 256)
    f1, bound1 = R.fpfh(Q, nr, None, rad_f, 256, lists=lists1, edge_tol=1e-5)
    same = (lists0[0] == lists1[0]).all(1)
    assert same.mean() > 0.95
    err = np.abs(f0 - f1).max(1)
    assert (err <= 1e-6 * np.abs(f0).max(1) + bound0 + bound1)[same].mean() > 0.995
    assert (err[same] <= 1e-6 * np.abs(f0).max(1)[same]).mean() > 0.5


def test_voxel_restatements():
    P = np.array([[0.00, 0, 0], [0.04, 0, 0], [0.06, 0, 0], [0.11, 0, 0], [0.01, 0, 0]], np.float32)
    m, off = R.voxel_down_sample(P, None, 0.05)
    # origin -0.025: rows 0, 4 -> voxel 0; rows 1, 2 -> voxel 1 (0.065 / 0.05, 0.085 / 0.05); row 3 -> voxel 2
    assert list(off) == [0, 3]
    assert np.allclose(m[:, 0], [0.005, 0.05, 0.11], atol=1e-8)
    # one more row at -0.02 moves the origin to -0.045 and regroups the rest: {0, 5}, {1, 4}, {2}, {3}
    m3, off3 = R.voxel_down_sample(np.r_[P, [[-0.02, 0, 0]]].astype(np.float32), None, 0.05)
    assert list(off3) == [0, 4] and np.allclose(m3[:, 0], [-0.01, 0.025, 0.06, 0.11], atol=1e-8)
    sel, off = R.voxel_select(P, None, 0.05)
    assert list(sel) == [0, 2, 3] and list(off) == [0, 3]


# ---------------------------------------------------------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------------------------------------------------------

def test_public_names_exported():
    import gmf_amd
    for n in NAMES:
        assert hasattr(gmf_amd, n), n
        assert n in gmf_amd.__all__, n


def test_c_abi_declares_descriptors():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    for name in ABI:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load_library(), name), name
    assert "#define GMF_ABI_VERSION 5" in text


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_no_device_fails_loudly():
    import gmf_amd
    p = torch.rand(64, 3)
    n = torch.rand(64, 3)
    calls = [
        lambda: gmf_amd.radius_knn_batched(p, [0, 32, 64], 0.1, 30),
        lambda: gmf_amd.estimate_normals_batched(p, [0, 64], 0.1),
        lambda: gmf_amd.compute_fpfh_batched(p, n, None, 0.25),
        lambda: gmf_amd.voxel_down_sample_batched(p, [0, 64], 0.05),
        lambda: gmf_amd.voxel_select_batched(p, None, 0.05),
        lambda: gmf_amd.voxel_down_sample(p, 0.05),
        lambda: gmf_amd.voxel_select(p, 0.05),
        lambda: gmf_amd.estimate_normals(p, 0.1),
        lambda: gmf_amd.compute_fpfh_feature(p, n, 0.25),
        lambda: gmf_amd.fpfh_descriptors(p, 0.05),
        lambda: gmf_amd.fpfh_descriptors(p, 0.05, voxelize="select"),
    ]
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


def test_argument_checks():
    import gmf_amd
    p = torch.rand(64, 3)
    n = torch.rand(64, 3)
    bad = [
        (lambda: gmf_amd.radius_knn_batched(p.double(), None, 0.1, 30), "float32"),
        (lambda: gmf_amd.radius_knn_batched(p[:, :2], None, 0.1, 30), r"\[sum N,3\]"),
        (lambda: gmf_amd.radius_knn_batched(torch.zeros(0, 3), None, 0.1, 30), "non-empty"),
        (lambda: gmf_amd.radius_knn_batched(p.numpy(), None, 0.1, 30), "torch tensor"),
        (lambda: gmf_amd.radius_knn_batched(p, [0, 32], 0.1, 30), "offsets"),
        (lambda: gmf_amd.radius_knn_batched(p, [0, 40, 40, 64], 0.1, 30), "offsets"),
        (lambda: gmf_amd.radius_knn_batched(p, None, 0.0, 30), "radius"),
        (lambda: gmf_amd.radius_knn_batched(p, None, float("inf"), 30), "radius"),
        (lambda: gmf_amd.radius_knn_batched(p, None, 0.1, 0), "max_nn"),
        (lambda: gmf_amd.radius_knn_batched(p, None, 0.1, 257), "max_nn"),
        (lambda: gmf_amd.radius_knn_batched(p, None, 0.1, 2.5), "max_nn"),
        (lambda: gmf_amd.estimate_normals_batched(p, None, -1.0), "radius"),
        (lambda: gmf_amd.estimate_normals(p, 0.1, max_nn=300), "max_nn"),
        (lambda: gmf_amd.compute_fpfh_batched(p, n[:10], None, 0.25), "normals"),
        (lambda: gmf_amd.compute_fpfh_batched(p, n.double(), None, 0.25), "normals"),
        (lambda: gmf_amd.compute_fpfh_feature(p, n, float("nan")), "radius"),
        (lambda: gmf_amd.voxel_down_sample(p, 0.0), "voxel_size"),
        (lambda: gmf_amd.voxel_select_batched(p, [1, 64], 0.05), "offsets"),
        (lambda: gmf_amd.fpfh_descriptors(p, 0.05, voxelize="grid"), "voxelize"),
        (lambda: gmf_amd.fpfh_descriptors(p, -0.05), "voxel_size"),
    ]
    for f, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            f()
