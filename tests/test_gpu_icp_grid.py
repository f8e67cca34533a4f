"""GPU tests of ICP's nearest-neighbour search on the hashed tau-grid (`search="grid"`: csrc/solver_kernels.hip, k_icp_nn_grid).

The grid search evaluates the brute-force search's own d^2 expression on the targets of the 27 cells around a transformed source
row and keeps the same (d^2 bits, row) minimum, so the contract is exact equality with `search="brute"` on all five outputs (T,
fitness, inlier_rmse, iterations, nn).  The brute-force path is pinned to a numpy restatement by tests/test_gpu_solvers.py; one
test here checks the grid against scipy's kd-tree directly."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import gmf_amd
from gmf_amd import synthetic
from test_gpu_solvers import DEV, _cloud_case, _eq, _g, _keypoint_case, _perturb

pytestmark = pytest.mark.gpu

F32 = np.float32


def _icp(search, s, q, T0, tau, **kw):
    return gmf_amd.icp_point_to_point_batched(s, q, T0, tau, search=search, **kw)


def _assert_equal(a, b, where=""):
    for k, name in enumerate(("T", "fitness", "inlier_rmse", "iterations", "nn")):
        assert bool(torch.isfinite(a[k].double()).all()), (where, name)            # (NaN would make torch.equal vacuous)
        assert _eq(a[k], b[k]), (where, name)


def _both(s, q, T0, tau, where="", **kw):
    """search="grid" and search="brute" on the same device tensors; asserts equality, returns the grid's outputs."""
    s, q, T0 = (x if torch.is_tensor(x) else _g(x) for x in (s, q, T0))
    grid = _icp("grid", s, q, T0, tau, **kw)
    _assert_equal(grid, _icp("brute", s, q, T0, tau, **kw), where)
    return grid


# ---------------------------------------------------------------------------------------------------------------------------
# 1. a hand-built scene of edge cases
# ---------------------------------------------------------------------------------------------------------------------------

def test_edge_scene():
    """tau = 0.25 (exact in fp32), identity init, no iteration: with T = I the transformed source row is the source row, and every
    difference below is exact in fp32, so the expected vector follows by hand.  h = tau (1 + 2^-10) = 2^-2 + 2^-12, and its small
    multiples, are exact in fp32 too."""
    tau = 0.25
    h = tau * (1 + 2.0 ** -10)
    assert F32(h) == h and F32(41 * h) == 41 * h
    inside = np.nextafter(F32(0.25), F32(0))
    src = np.array([
        [0, 0, 0],                                  # 0: its only target at exactly tau: out
        [0, 5, 0],                                  # 1: one target just inside tau
        [0, 10, 0],                                 # 2: two identical target rows: the smaller row
        [0, 15, 0],                                 # 3: three targets at 0.125 on a lattice: the smallest row
        [-3.1, -7.3, -2.2],                         # 4: negative coordinates
        [2 * h, -3 * h, h],                         # 5: on a cell corner, targets in the cells on both sides
        [-40 * h, -40 * h, -40 * h],                # 6: on a negative cell corner; one target exactly one cell edge away (out)
        [50, 50, 50],                               # 7: nothing within tau
        [1e6, 1e6, 1e6],                            # 8: 1e6 from the origin (fp32 spacing 2^-4): one in, one at exactly tau
    ], np.float64).astype(F32)
    tgt = np.array([
        [0.25, 0, 0],                               # 0
        [inside, 5, 0],                             # 1
        [0.1, 10, 0], [0.1, 10, 0],                 # 2 3
        [0.125, 15, 0], [-0.125, 15, 0], [0, 15, 0.125],      # 4 5 6
        [-3.05, -7.25, -2.15], [-3.3, -7.3, -2.2],  # 7 8
        [2 * h - 0.1, -3 * h, h], [2 * h, -3 * h + 0.2, h], [3 * h, -3 * h, h],      # 9 10 11
        [-41 * h, -40 * h, -40 * h], [-40 * h + 0.24, -40 * h, -40 * h],            # 12 13
        [1e6 + 0.125, 1e6, 1e6], [1e6 + 0.25, 1e6, 1e6], [1e6, 1e6 - 0.1875, 1e6],  # 14 15 16
    ], np.float64).astype(F32)
    want = [-1, 1, 2, 4, 7, 9, 13, -1, 14]
    T0 = np.eye(4, dtype=F32)
    out = _both(src[None], tgt[None], T0[None], tau, "edge", max_iteration=0)
    assert out[4][0].cpu().tolist() == want
    assert int(out[3][0]) == 0 and _eq(out[0][0], torch.eye(4))
    assert abs(float(out[1][0]) - 7 / 9) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# 2. against a kd-tree
# ---------------------------------------------------------------------------------------------------------------------------

KD_SEED, KD_NS, KD_NT = 23, 2000, 3000
KD_BAND = 1e-5


def kd_case():
    """The case, the transformed source rows as the kernels round them (fp64 transform, one rounding to fp32) and the float64
    kd-tree's nearest target of each."""
    src, tgt, T0, tau, _ = _cloud_case(KD_SEED, KD_NS, KD_NT)
    T = T0.astype(np.float64)
    P = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F32).astype(np.float64)
    Q = tgt.astype(np.float64)
    d, j = cKDTree(Q).query(P)
    return src, tgt, T0, tau, P, Q, d, j


def test_against_kdtree():
    src, tgt, T0, tau, P, Q, d, _ = kd_case()
    out = _icp("grid", _g(src)[None], _g(tgt)[None], _g(T0)[None], tau, max_iteration=0)
    nn = out[4][0].cpu().numpy()
    hit = nn >= 0
    assert hit.any() and (~hit).any()
    got = np.linalg.norm(P[hit] - Q[nn[hit]], axis=1)
    assert (np.abs(got - d[hit]) <= 1e-6 * d[hit]).all(), np.abs(got / d[hit] - 1).max()
    band = np.abs(d - tau) <= KD_BAND * tau
    assert band.mean() < 0.01
    assert np.array_equal(hit[~band], (d < tau)[~band])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. full loops
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [lambda: _keypoint_case(21, 1000), lambda: _cloud_case(23, 8000, 10000)],
                         ids=["keypoints-1000", "cloud-8k-10k"])
def test_full_loop_equals_brute_force(make):
    src, tgt, T0, tau, _ = make()
    out = _both(src[None], tgt[None], T0[None], tau)
    assert int(out[3][0]) >= 2 and float(out[1][0]) > 0.3           # (the loop ran and found its correspondences)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. tiny table, crowded slots
# ---------------------------------------------------------------------------------------------------------------------------

THREE_TAU = 0.08


def three_target_scene():
    """Three targets and 500 source rows around them.  tests/test_icp_grid_host.py restates the hash and checks that this scene
    meets two cells of one query in one slot and a far cell's target in a visited slot."""
    r = np.random.default_rng(51)
    tgt = np.array([[0.0, 0.0, 0.0], [0.12, 0.0, 0.0], [0.5, 0.5, 0.5]], F32)
    src = np.concatenate([tgt[r.integers(0, 3, 400)] + r.normal(0, 0.04, (400, 3)), r.uniform(-1, 1, (100, 3))]).astype(F32)
    return src, tgt


def test_three_targets():
    """Three targets: the table has its smallest size (64 slots) and each query's 27 cells alone fill a good part of it, so
    colliding cells, a slot reached twice and slots of far cells are all met (asserted on the host from the hash)."""
    src, tgt = three_target_scene()
    out = _both(src[None], tgt[None], np.eye(4, dtype=F32)[None], THREE_TAU, "three")
    assert 0.2 < float(out[1][0]) < 0.95


def test_all_targets_in_one_cell():
    """3000 targets inside one cell of the grid (cell edge ~0.05): one slot far over the size at which a source row's 32 lanes
    walk it together."""
    r = np.random.default_rng(52)
    tgt = r.uniform(0.005, 0.045, (3000, 3)).astype(F32)
    src = r.uniform(-0.06, 0.11, (500, 3)).astype(F32)
    out = _both(src[None], tgt[None], np.eye(4, dtype=F32)[None], 0.05, "one-cell")
    assert 0.1 < float(out[1][0]) < 1.0


def test_slot_sizes_around_the_shared_walk():
    """Cells of 31, 32, 33 (the walk changes hands above 32 rows), 64 and 65 targets, far from one another, as five pairs."""
    r = np.random.default_rng(53)
    S, Q = [], []
    for b, n in enumerate([31, 32, 33, 64, 65]):
        c = np.array([0.5 * b, -0.3 * b, 0.2 * b]) // 0.05 * (0.05 * (1 + 2.0 ** -10))       # a cell's corner
        Q.append((c + r.uniform(0.005, 0.045, (n, 3))).astype(F32))
        S.append((c + r.uniform(-0.05, 0.1, (120, 3))).astype(F32))
    soff = np.concatenate([[0], np.cumsum([len(x) for x in S])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(x) for x in Q])]).tolist()
    I = np.tile(np.eye(4, dtype=F32), (5, 1, 1))
    out = _both(np.concatenate(S), np.concatenate(Q), I, 0.05, "slots", source_offsets=soff, target_offsets=toff, max_iteration=3)
    assert (out[1].cpu().numpy() > 0.1).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. ragged batch
# ---------------------------------------------------------------------------------------------------------------------------

def _ragged_batch():
    """Eight pairs.  2 and 3 lie in one region of space (the same scene under the same motion, different rows and noise), so each
    one's cells also hold the other's rows; 5's sources are all far from its targets (C empty); 6 starts at its exact motion on a
    clean scene and converges passes before the others."""
    sizes = [(700, 900), (1, 1), (1200, 1000), (900, 1300), (40, 5), (300, 300), (800, 800), (2500, 3000)]
    cases = []
    for b, (Ns, Nt) in enumerate(sizes):
        r = np.random.default_rng([2 if b == 3 else b, 0x9d1d])          # pair 3 repeats pair 2's scene and motion
        X = r.uniform(0, 3, (3000, 3))
        R = synthetic.random_rotation(r)
        t = r.uniform(-0.3, 0.3, 3)
        Tg = np.eye(4)
        Tg[:3, :3], Tg[:3, 3] = R, t
        r = np.random.default_rng([b, 0x5eed])
        rows_s, rows_t = r.permutation(3000)[:Ns], r.permutation(3000)[:Nt]
        if min(Ns, Nt) < 100 or b == 6:
            rows_t = rows_s[np.arange(Nt) % Ns]                             # small pairs and pair 6: the targets are sources' images
        noise = 0.0 if b == 6 else 0.005
        tgt = (X[rows_t] @ R.T + t + r.normal(0, noise, (Nt, 3))).astype(F32)
        src = X[rows_s].astype(F32)
        if b == 6:
            T0 = Tg.astype(F32)
        else:
            T0 = _perturb(Tg, 0.3, 0.01, b) if min(Ns, Nt) < 100 else _perturb(Tg, 3.0, 0.05, b)
        if b == 5:
            tgt = tgt + F32(100.0)
        cases.append((src, tgt, T0))
    return cases


def test_ragged_batch():
    cases = _ragged_batch()
    tau = 0.08
    soff = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]).tolist()
    S, Q = (np.concatenate([c[k] for c in cases]) for k in (0, 1))
    I = np.stack([c[2] for c in cases])
    out = _both(S, Q, I, tau, "batch", source_offsets=soff, target_offsets=toff)
    for b, (s, q, T0) in enumerate(cases):
        one = _icp("grid", _g(s)[None], _g(q)[None], _g(T0)[None], tau)
        for k in range(4):
            assert _eq(out[k][b], one[k][0]), (b, k)
        assert _eq(out[4][soff[b]:soff[b + 1]], one[4][0]), b
    T, fit, rmse, it, nn = (x.cpu() for x in out)
    assert float(fit[5]) == 0 and float(rmse[5]) == 0 and int(it[5]) == 1
    assert torch.equal(T[5], torch.as_tensor(cases[5][2])) and (nn[soff[5]:soff[6]] == -1).all()
    assert int(it[6]) + 2 <= min(int(it[b]) for b in (0, 2, 3, 7)), it.tolist()
    assert float(fit[1]) == 1.0 and float(fit[2]) > 0.2 and float(fit[3]) > 0.2
    # pairs 2 and 3 overlap in space: a grid keyed by cell alone would hand pair 2 rows of pair 3
    lo2, hi2 = Q[toff[2]:toff[3]].min(0), Q[toff[2]:toff[3]].max(0)
    assert ((Q[toff[3]:toff[4]] > lo2) & (Q[toff[3]:toff[4]] < hi2)).all(1).mean() > 0.9


# ---------------------------------------------------------------------------------------------------------------------------
# 6. determinism and graph capture
# ---------------------------------------------------------------------------------------------------------------------------

def test_determinism_and_graph_capture():
    cases = _ragged_batch()
    soff = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]).tolist()
    S = _g(np.concatenate([c[0] for c in cases]))
    Q = _g(np.concatenate([c[1] for c in cases]))
    I = _g(np.stack([c[2] for c in cases]))

    def run():
        return _icp("grid", S, Q, I, 0.08, source_offsets=soff, target_offsets=toff)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        first = [x.clone() for x in run()]
        eager = [x.clone() for x in run()]               # (also sizes the workspace and uploads the offsets before the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for x, y in zip(first, eager):
        assert _eq(x, y)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = run()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, captured):
        assert _eq(x, y)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. wrappers
# ---------------------------------------------------------------------------------------------------------------------------

def test_registration_icp_wrapper():
    src, tgt, T0, tau, _ = _cloud_case(61, 1500, 2000)
    a = gmf_amd.registration_icp(_g(src), _g(tgt), tau, init=_g(T0), search="grid")
    b = gmf_amd.registration_icp(_g(src), _g(tgt), tau, init=_g(T0), search="brute")
    assert _eq(a.transformation, b.transformation) and _eq(a.correspondence_set, b.correspondence_set)
    assert a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse
    assert a.correspondence_set.shape[0] > 100


def test_register_with_grid_icp(monkeypatch):
    from gmf_amd import dgr
    from test_gpu_fcgf import _NC, _dgr, _quantized_cloud, _tokens
    seen = []
    real = dgr.registration_icp

    def spy(*a, **kw):
        res = real(*a, **kw)
        seen.append((kw.get("search"), res.fitness, int(res.correspondence_set.shape[0])))
        return res

    monkeypatch.setattr(dgr, "registration_icp", spy)
    xyz0 = _quantized_cloud()
    xyz1 = xyz0 + (np.array([8, 16, -8], np.float64) * _NC["voxel_size"]).astype(F32)
    d = _dgr()
    assert d.icp_search == "brute"
    pt, qt = _tokens()
    Tb = d.register(xyz0, xyz1, p_tokens=pt, q_tokens=qt)
    d.icp_search = "grid"
    Tg = d.register(xyz0, xyz1, p_tokens=pt, q_tokens=qt)
    assert Tg.dtype == np.float64 and np.isfinite(Tg).all()
    assert np.array_equal(Tg, Tb)
    assert [x[0] for x in seen] == ["brute", "grid"] and seen[0][1:] == seen[1][1:]
    assert seen[1][1] > 0.5 and seen[1][2] > 100                     # ICP had correspondences to work on


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the C ABI entry itself: search = 0 and the argument checks
# ---------------------------------------------------------------------------------------------------------------------------

def _ex_args(s, q, T0, tau, max_iter=30):
    """Device buffers and the argument list of gmf_icp_point_to_point_ex for one pair, up to and including `nn`."""
    from gmf_amd._util import handle_and_stream
    ns, nt = s.shape[0], q.shape[0]
    so = torch.tensor([0, ns], dtype=torch.int32, device=DEV)
    to = torch.tensor([0, nt], dtype=torch.int32, device=DEV)
    out = dict(T=torch.zeros((1, 4, 4), device=DEV), fit=torch.zeros(1, device=DEV), rmse=torch.zeros(1, device=DEV),
               it=torch.zeros(1, dtype=torch.int32, device=DEV), nn=torch.zeros(ns, dtype=torch.int64, device=DEV))
    keep = (s, q, T0, so, to)
    args = [s.data_ptr(), so.data_ptr(), q.data_ptr(), to.data_ptr(), 1, ns, ns, nt, T0.data_ptr(), tau, max_iter, 1e-6, 1e-6,
            out["T"].data_ptr(), out["fit"].data_ptr(), out["rmse"].data_ptr(), out["it"].data_ptr(), out["nn"].data_ptr()]
    h, st = handle_and_stream(s)
    return h, st, args, out, keep


def test_c_abi_ex_entry():
    src, tgt, T0, tau, _ = _cloud_case(71, 1200, 1500)
    s, q, I = _g(src), _g(tgt), _g(T0)[None].contiguous()
    want = _icp("brute", s[None], q[None], I, tau)
    for search in (0, 1):
        h, st, args, out, keep = _ex_args(s, q, I, tau)
        h.call("gmf_icp_point_to_point_ex", *args, len(tgt), search, st)
        got = (out["T"], out["fit"], out["rmse"], out["it"], out["nn"][None])
        _assert_equal(got, want, f"search={search}")
    assert int(want[3][0]) >= 2 and float(want[1][0]) > 0.5
    h, st, args, out, keep = _ex_args(s, q, I, tau)
    bad = [
        (args, 0, 1, "total_tgt"), (args, -5, 0, "total_tgt"), (args, 1 << 31, 1, "total_tgt"),
        (args, len(tgt), 2, "search must be"), (args, len(tgt), -1, "search must be"),
        (args, 1 << 29, 1, "fewer than 2\\^29"),
        ([None] + args[1:], len(tgt), 1, "null pointer"), (args[:-1] + [None], len(tgt), 1, "null pointer"),
        (args[:9] + [0.0] + args[10:], len(tgt), 1, "max_correspondence_distance"),
        (args[:10] + [-1] + args[11:], len(tgt), 1, "max_iteration"),
        (args[:4] + [0] + args[5:], len(tgt), 1, "empty batch"),
    ]
    for a, total_tgt, search, msg in bad:
        with pytest.raises(RuntimeError, match=r"status -\d+.*icp_point_to_point_ex.*" + msg):
            h.call("gmf_icp_point_to_point_ex", *a, total_tgt, search, st)
    gmf_amd.check_status()
