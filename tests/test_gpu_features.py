"""GPU tests of the descriptor stages (gmf_amd/features.py, csrc/pointcloud_kernels.hip) against the float64 numpy restatement of
their contract (tests/fpfh_reference.py): the radius search bit for bit, normals, FPFH, both voxel grids, ragged batching,
determinism, graph capture, and the whole chain points -> FPFH -> matching -> RANSAC -> ICP on the 3DMatch demo fragments."""
import math
import os

import numpy as np
import pytest
import torch

import fpfh_reference as R
import gmf_amd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _eq(a, b):
    return torch.equal(a.cpu(), b.cpu())


def _np(t):
    return t.cpu().numpy()


_CACHE = {}


def _fixture(k):
    if "npz" not in _CACHE:
        _CACHE["npz"] = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
    return _CACHE["npz"][f"cloud{k}"]


def _down(k, v):
    key = (k, v)
    if key not in _CACHE:
        _CACHE[key] = R.voxel_down_sample(_fixture(k), None, v)[0]
    return _CACHE[key]


def _check_search(P, off, radius, max_nn):
    idx, d2, cnt = gmf_amd.radius_knn_batched(_g(P), off, radius, max_nn)
    ri, rd, rc = R.radius_knn(P, off, radius, max_nn)
    assert np.array_equal(_np(cnt), rc)
    assert np.array_equal(_np(idx), ri)
    assert np.array_equal(_np(d2).view(np.uint64), rd.view(np.uint64))
    return rc


# ---------------------------------------------------------------------------------------------------------------------------
# 1. search
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius,max_nn", [(0.08, 30), (0.15, 100), (0.15, 256)])
def test_search_uniform(radius, max_nn):
    P = np.random.default_rng(3).uniform(0, 1, (6000, 3)).astype(np.float32)
    rc = _check_search(P, None, radius, max_nn)
    assert rc.min() >= 1                         # the row itself


@pytest.mark.parametrize("v", [0.05, 0.025])
def test_search_fixture(v):
    for k in (0, 1):
        P = _down(k, v)
        _check_search(P, None, 2 * v, 30)
        rc = _check_search(P, None, 5 * v, 100)
        assert (rc == 100).mean() > 0.2          # the max_nn cut binds: the selection is on the tested path


def test_search_ragged():
    r = np.random.default_rng(4)
    clouds = [r.uniform(0, s, (n, 3)).astype(np.float32) for n, s in ((1000, 0.5), (3000, 1.0), (1, 1.0), (700, 0.3))]
    P = np.concatenate(clouds)
    off = np.r_[0, np.cumsum([len(c) for c in clouds])].tolist()
    _check_search(P, off, 0.1, 40)
    # the same points as one cloud give other lists: clouds do not mix
    idx, _, _ = gmf_amd.radius_knn_batched(_g(P), off, 0.1, 40)
    for b in range(len(clouds)):
        assert _np(idx[off[b]:off[b + 1]]).max() < off[b + 1] - off[b]


def test_search_dense_cluster():
    r = np.random.default_rng(5)
    c = r.normal(size=(4500, 3))
    c = 0.2 * c / np.linalg.norm(c, axis=1, keepdims=True) * r.uniform(0, 1, (4500, 1)) ** (1 / 3)
    P = np.concatenate([c, r.uniform(-1, 1, (1500, 3))]).astype(np.float32)
    rc = _check_search(P, None, 0.25, 100)
    assert rc[:4500].min() == 100
    _check_search(P, None, 0.25, 256)
    _check_search(P, None, 0.25, 1)


def test_search_exact_radius_boundary():
    P = np.array([[0, 0, 0], [0.25, 0, 0], [0, 0.125, 0], [0, -0.125, 0], [0, 0, -0.25], [0.2, 0, 0]], np.float32)
    idx, d2, cnt = gmf_amd.radius_knn_batched(_g(P), None, 0.25, 8)
    assert int(cnt[0]) == 4 and _np(idx[0, :5]).tolist() == [0, 2, 3, 5, -1]   # d^2 == r^2 exactly: outside
    _check_search(P, None, 0.25, 8)
    _check_search(P, None, 0.25000001, 8)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. normals, 3. FPFH
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", [0.05, 0.025])
def test_normals_fixture(v):
    for k in (0, 1):
        P = _down(k, v)
        n = _np(gmf_amd.estimate_normals(_g(P), 2 * v, 30)).astype(np.float64)
        ref, A, cnt = R.estimate_normals(P, None, 2 * v, 30)
        few = cnt < 3
        assert np.array_equal(n[few], np.tile([0.0, 0.0, 1.0], (few.sum(), 1)))
        w = np.linalg.eigvalsh(R.sym(A[~few]))
        clear = (w[:, 1] - w[:, 0]) > 1e-3 * w[:, 2]
        nn, rr = n[~few], ref[~few]
        assert np.abs(nn[clear] - rr[clear]).max() <= 1e-5           # the same sign, not only the same axis
        u = nn[~clear]
        assert np.allclose((u * u).sum(1), 1, atol=1e-6)
        q = np.einsum("ni,nij,nj->n", u, R.sym(A[~few][~clear]), u)
        assert np.all(q <= w[~clear, 0] + 1e-6 * w[~clear, 2])


@pytest.mark.parametrize("v", [0.05, 0.025])
def test_fpfh_fixture(v):
    for k in (0, 1):
        P = _down(k, v)
        Pg = _g(P)
        ng = gmf_amd.estimate_normals(Pg, 2 * v, 30)
        f = _np(gmf_amd.compute_fpfh_feature(Pg, ng, 5 * v, 100)).astype(np.float64)
        ref, bound = R.fpfh(P, _np(ng), None, 5 * v, 100)
        err = np.abs(f - ref).max(1)
        tol = 1e-5 * np.abs(ref).max(1)
        flagged = bound > 0
        assert np.all(err[~flagged] <= tol[~flagged]), err[~flagged].max()
        assert np.all(err[flagged] <= tol[flagged] + bound[flagged])
        sums = f.reshape(-1, 3, 11).sum(2)
        lists = R.radius_knn(P, None, 5 * v, 100)
        has = (lists[1] > 0).any(1)
        assert np.allclose(sums[has], 200, atol=1e-3)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. voxel grids
# ---------------------------------------------------------------------------------------------------------------------------

def _check_voxels(P, off, v):
    m, mo = gmf_amd.voxel_down_sample_batched(_g(P), off, v)
    rm, ro = R.voxel_down_sample(P, off, v)
    assert _np(mo).tolist() == list(ro)
    gm = _np(m)
    assert gm.shape == rm.shape
    ulp = np.spacing(np.abs(rm).astype(np.float32))
    assert np.all(np.abs(gm - rm) <= ulp)
    s, so = gmf_amd.voxel_select_batched(_g(P), off, v)
    rs, rso = R.voxel_select(P, off, v)
    assert _np(so).tolist() == list(rso) and np.array_equal(_np(s), rs)
    return gm


def test_voxel_fixture_and_synthetic():
    for k in (0, 1):
        for v in (0.05, 0.025):
            _check_voxels(_fixture(k), None, v)
    r = np.random.default_rng(6)
    P = np.concatenate([r.uniform(-3, 3, (20000, 3)), np.round(r.uniform(-1, 1, (5000, 3)) * 20) / 20]).astype(np.float32)
    _check_voxels(P, None, 0.05)
    _check_voxels(P, [0, 7000, 7001, 25000], 0.1)


def test_voxel_origin_follows_min_bound():
    P = np.array([[0.00, 0, 0], [0.04, 0, 0], [0.06, 0, 0], [0.11, 0, 0], [0.01, 0, 0]], np.float32)
    a = _check_voxels(P, None, 0.05)
    assert np.allclose(a[:, 0], [0.005, 0.05, 0.11], atol=1e-8)
    b = _check_voxels(np.r_[P, [[-0.02, 0, 0]]].astype(np.float32), None, 0.05)
    assert np.allclose(b[:, 0], [-0.01, 0.025, 0.06, 0.11], atol=1e-8)


def test_voxel_range_is_rejected():
    P = np.array([[0, 0, 0], [1e6, 0, 0]], np.float32)
    with pytest.raises(RuntimeError, match="int32"):
        gmf_amd.voxel_down_sample(_g(P), 1e-5)
    with pytest.raises(RuntimeError, match="int32"):
        gmf_amd.voxel_select(_g(P), 1e-5)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. batching, determinism, graph capture
# ---------------------------------------------------------------------------------------------------------------------------

def _stages(Pg, off, v):
    idx, d2, cnt = gmf_amd.radius_knn_batched(Pg, off, 5 * v, 100)
    n = gmf_amd.estimate_normals_batched(Pg, off, 2 * v, 30)
    f = gmf_amd.compute_fpfh_batched(Pg, n, off, 5 * v, 100)
    return [idx, d2, cnt, n, f]


def test_ragged_batch_equals_per_cloud_and_repeats():
    v = 0.05
    clouds = [_down(0, v), _down(1, v), _down(0, 0.025)[:3000]]
    P = np.concatenate(clouds)
    off = np.r_[0, np.cumsum([len(c) for c in clouds])].tolist()
    Pg = _g(P)
    batch = _stages(Pg, off, v)
    again = _stages(Pg, off, v)
    for a, b in zip(batch, again):
        assert _eq(a, b)
    for bi, c in enumerate(clouds):
        one = _stages(_g(c), None, v)
        for a, b in zip(batch, one):
            assert _eq(a[off[bi]:off[bi + 1]], b)
    # the voxel grids: batched = per cloud
    raw = [_fixture(0)[:12000], _fixture(1)[:9000]]
    R0 = np.concatenate(raw)
    roff = [0, 12000, 21000]
    m, mo = gmf_amd.voxel_down_sample_batched(_g(R0), roff, 0.05)
    s, so = gmf_amd.voxel_select_batched(_g(R0), roff, 0.05)
    mo, so = _np(mo), _np(so)
    for bi, c in enumerate(raw):
        assert _eq(m[mo[bi]:mo[bi + 1]], gmf_amd.voxel_down_sample(_g(c), 0.05))
        assert _eq(s[so[bi]:so[bi + 1]], gmf_amd.voxel_select(_g(c), 0.05))


def test_graph_capture_equals_eager():
    v = 0.05
    clouds = [_down(0, v), _down(1, v)]
    Pg = _g(np.concatenate(clouds))
    off = _g(np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.int32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                           # (also sizes the workspace before the capture)
            eager = [x.clone() for x in _stages(Pg, off, v)]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = _stages(Pg, off, v)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, captured):
        assert _eq(x, y)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------------------------------------------------------

def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K


def _pose_error(T, Tgt):
    Rr = T[:3, :3].T @ Tgt[:3, :3]
    re = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(Rr) - 1) / 2))))
    te = np.linalg.norm(T[:3, 3] - Tgt[:3, 3])
    return re, te


@pytest.mark.parametrize("voxelize", ["mean", "select"])
def test_end_to_end_registration(voxelize):
    r = np.random.default_rng(7)
    src = _fixture(0).astype(np.float64)
    Tgt = np.eye(4)
    Tgt[:3, :3] = _rot([0.3, 1.0, 0.2], 45)
    Tgt[:3, 3] = [0.3, -0.2, 0.346]
    assert abs(np.linalg.norm(Tgt[:3, 3]) - 0.5) < 0.01
    tgt = src @ Tgt[:3, :3].T + Tgt[:3, 3] + r.normal(0, 0.005, src.shape)
    v = 0.05
    xs, fs = gmf_amd.fpfh_descriptors(_g(src.astype(np.float32)), v, voxelize=voxelize)
    xt, ft = gmf_amd.fpfh_descriptors(_g(tgt.astype(np.float32)), v, voxelize=voxelize)
    assert torch.isfinite(fs).all() and torch.isfinite(ft).all()
    if voxelize == "mean":
        j, _ = gmf_amd.nn_match(fs, ft)
    else:
        j = gmf_amd.find_knn_gpu(fs, ft, nn_max_n=-1, knn=1)
    corres = torch.stack([torch.arange(len(j), device=DEV), j.view(-1)], 1)
    res = gmf_amd.registration_ransac_based_on_correspondence(xs, xt, corres, 2 * v, ransac_n=3, max_iteration=50000,
                                                               max_validation=50000, seed=1)
    icp = gmf_amd.registration_icp(xs, xt, 2 * v, init=res.transformation)
    T = _np(icp.transformation).astype(np.float64)
    re, te = _pose_error(T, Tgt)
    re0, te0 = _pose_error(_np(res.transformation).astype(np.float64), Tgt)
    print(f"[{voxelize}] M = {len(xs)} / {len(xt)}; RANSAC fitness {res.fitness:.3f}: {re0:.2f} deg, {100 * te0:.1f} cm; "
          f"ICP: {re:.3f} deg, {100 * te:.2f} cm")
    assert re < 15 and te < 0.30
    assert re < 2 and te < 0.05          # expected far better than the thresholds
