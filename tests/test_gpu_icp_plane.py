"""GPU tests of point-to-plane ICP (gmf_amd.icp_point_to_plane_batched: csrc/solver_kernels.hip, k_icp_plane_partials and
k_icp_plane_solve) and of its way into registration_icp, local_refinement_batched and multiway_registration.

The device is held to the float64 restatement in tests/icp_plane_reference.py with the gates tests/test_gpu_solvers.py uses for
the point-to-point form (test_icp_matches_restatement, test_icp_recovers_clean_scene); tests/test_icp_plane_host.py shows that
the restatement alone moves by less than a tenth of those gates under one-ulp perturbations.  Everything else is exact: the
search, the batch, the sign of the normals and graph capture change no bit."""

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import gmf_amd
import icp_plane_reference as R
from gmf_amd.solvers import ICP_PLANE_ROWS
from test_gpu_solvers import DEV, _eq, _g, _perturb
from test_icp_plane_host import reference_run

pytestmark = pytest.mark.gpu

NAMES = ("T", "fitness", "inlier_rmse", "iterations", "nn")
EYE = np.eye(4, dtype=np.float32)


def _plane(s, q, n, T0, tau=R.TAU, **kw):
    s, q, n, T0 = (x if torch.is_tensor(x) else _g(x) for x in (s, q, n, T0))
    return gmf_amd.icp_point_to_plane_batched(s, q, n, T0, tau, **kw)


def _one(s, q, n, T0=EYE, **kw):
    """One pair given as numpy rows."""
    return _plane(s[None], q[None], n[None], np.asarray(T0, np.float32)[None], **kw)


def _assert_equal(a, b, where=""):
    for k, name in enumerate(NAMES):
        assert bool(torch.isfinite(a[k].double()).all()), (where, name)            # (NaN would make torch.equal vacuous)
        assert _eq(a[k], b[k]), (where, name)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.CASES))
def test_matches_restatement(name):
    src, tgt, nrm, _, (Tr, fr, rr, itr, _) = reference_run(name)
    T, fit, rmse, it, nn = _one(src, tgt, nrm)
    T = T[0].cpu().numpy()
    print(f"{name}: max|dT| = {np.abs(T - Tr).max():.3e}, fitness {float(fit[0]):.6f} / {fr:.6f}, rmse {float(rmse[0]):.6e} / "
          f"{rr:.6e}, passes {int(it[0])} / {itr}")
    assert np.abs(T - Tr).max() < 1e-4, np.abs(T - Tr).max()
    assert abs(float(fit[0]) - fr) <= 2.0 / len(src)
    if R.CASES[name][2] == 0:
        assert float(rmse[0]) < 1e-6 and rr < 1e-6         # rounding noise of fp32 coordinates of magnitude 2 on both sides
    else:
        assert abs(float(rmse[0]) - rr) <= 1e-4 * rr
    assert abs(int(it[0]) - itr) <= 2, (int(it[0]), itr)
    assert abs(int((nn[0] >= 0).sum()) - round(fr * len(src))) <= 2


def test_recovers_the_ground_truth():
    src, tgt, nrm, Tg, _ = reference_run("clean")
    T, fit, _, _, _ = _one(src, tgt, nrm)
    T = T[0].cpu().numpy().astype(np.float64)
    assert R.rotation_error_deg(T, Tg) < 0.1
    assert np.linalg.norm(T[:3, 3] - Tg[:3, 3]) < 0.01
    assert float(fit[0]) > 0.99


# ---------------------------------------------------------------------------------------------------------------------------
# 2. what the estimator shares with the point-to-point form
# ---------------------------------------------------------------------------------------------------------------------------

def test_max_iteration_zero_equals_point_to_point():
    src, tgt, nrm, _, _ = reference_run("noisy")
    T0 = _perturb(np.eye(4), 1.0, 0.01, 4)
    for search in ("brute", "grid"):
        a = _one(src, tgt, nrm, T0, max_iteration=0, search=search)
        b = gmf_amd.icp_point_to_point_batched(_g(src)[None], _g(tgt)[None], _g(T0)[None], R.TAU, max_iteration=0, search=search)
        assert _eq(a[0], b[0]) and _eq(a[1], b[1]) and _eq(a[3], b[3]) and _eq(a[4], b[4])
        assert int(a[3][0]) == 0 and float(a[1][0]) > 0.05
        # the split changes the order of the d^2 sum: one fp32 ulp
        ra, rb = np.float32(a[2][0].item()), np.float32(b[2][0].item())
        assert abs(float(ra) - float(rb)) <= float(np.spacing(rb)), (ra, rb)


@pytest.mark.parametrize("name", list(R.CASES))
def test_brute_equals_grid(name):
    src, tgt, nrm, _, _ = reference_run(name)
    _assert_equal(_one(src, tgt, nrm, search="grid"), _one(src, tgt, nrm, search="brute"), name)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. a ragged batch equals its pairs one by one
# ---------------------------------------------------------------------------------------------------------------------------

RAGGED_NS = [1, 5, 255, 256, 257, ICP_PLANE_ROWS - 1, ICP_PLANE_ROWS, ICP_PLANE_ROWS + 1, 2 * ICP_PLANE_ROWS + 3]
EMPTY_PAIR = 3                                              # this pair's targets are moved away: C is empty


def _ragged_batch():
    cases = []
    for b, Ns in enumerate(RAGGED_NS + [40]):
        src, tgt, nrm, _ = R.corner(10 + b, 700 + 50 * b, Ns, 0.001)
        if b == EMPTY_PAIR:
            tgt = tgt + np.float32(100.0)
        cases.append((src, tgt, nrm, _perturb(np.eye(4), 0.5, 0.01, b)))
    return cases


@pytest.mark.parametrize("search", ["brute", "grid"])
def test_ragged_batch_equals_pairs(search):
    cases = _ragged_batch()
    soff = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]).tolist()
    S, Q, N = (np.concatenate([c[k] for c in cases]) for k in range(3))
    I = np.stack([c[3] for c in cases])
    out = _plane(S, Q, N, I, source_offsets=soff, target_offsets=toff, search=search)
    moved = 0
    for b, (s, q, n, T0) in enumerate(cases):
        one = _one(s, q, n, T0, search=search)
        for k in range(4):
            assert bool(torch.isfinite(out[k][b].double()).all()), (b, NAMES[k])
            assert _eq(out[k][b], one[k][0]), (b, NAMES[k])
        assert _eq(out[4][soff[b]:soff[b + 1]], one[4][0]), b
        moved += int(not torch.equal(out[0][b].cpu(), torch.as_tensor(T0)))
    assert moved >= len(cases) - 3                          # (the comparison is not one of untouched inits)
    T, fit, rmse, it, nn = (x.cpu() for x in out)
    e = EMPTY_PAIR
    assert float(fit[e]) == 0 and float(rmse[e]) == 0 and int(it[e]) == 1
    assert torch.equal(T[e], torch.as_tensor(cases[e][3])) and (nn[soff[e]:soff[e + 1]] == -1).all()
    # device offsets size the grid with the batch's total instead of the largest pair: the same bits
    dso, dto = (torch.tensor(o, dtype=torch.int32, device=DEV) for o in (soff, toff))
    _assert_equal(_plane(S, Q, N, I, source_offsets=dso, target_offsets=dto, search=search), out, "device offsets")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the normals: signs, the degenerate plane, NaN
# ---------------------------------------------------------------------------------------------------------------------------

def test_sign_flips_change_no_bit():
    src, tgt, nrm, _, _ = reference_run("noisy")
    flip = np.where(np.random.default_rng(3).random((len(nrm), 1)) < 0.5, np.float32(-1), np.float32(1))
    assert 0.4 < (flip < 0).mean() < 0.6
    _assert_equal(_one(src, tgt, nrm * flip), _one(src, tgt, nrm), "flipped")


def test_degenerate_plane_returns_init():
    src, tgt, nrm, _, _ = reference_run("small")
    flat = np.zeros_like(nrm)
    flat[:, 2] = 1.0
    T0 = _perturb(np.eye(4), 0.5, 0.01, 6)
    T, fit, _, it, _ = _one(src, tgt, flat, T0)
    assert _eq(T[0], torch.as_tensor(T0)) and int(it[0]) == 1 and float(fit[0]) > 0.5


def test_nan_normals_add_nothing():
    src, tgt, nrm, _, _ = reference_run("noisy")
    bad = np.random.default_rng(12).random(len(nrm)) < 0.2
    holes, zeros = nrm.copy(), nrm.copy()
    holes[bad, 1] = np.nan
    holes[bad & (np.arange(len(nrm)) % 2 == 0), 0] = np.inf
    zeros[bad] = 0.0
    a = _one(src, tgt, holes)
    _assert_equal(a, _one(src, tgt, zeros), "NaN normals")
    assert int(a[3][0]) >= 2                                 # the loop ran: those rows were met


# ---------------------------------------------------------------------------------------------------------------------------
# 5. graph capture
# ---------------------------------------------------------------------------------------------------------------------------

def test_graph_capture_equals_eager():
    cases = _ragged_batch()
    soff = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]).tolist()
    S, Q, N = (_g(np.concatenate([c[k] for c in cases])) for k in range(3))
    I = _g(np.stack([c[3] for c in cases]))

    def run():
        return _plane(S, Q, N, I, source_offsets=soff, target_offsets=toff, search="grid")

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        first = [x.clone() for x in run()]
        eager = [x.clone() for x in run()]               # (also sizes the workspace and uploads the offsets before the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _assert_equal(first, eager, "repeat")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = run()
    g.replay()
    torch.cuda.synchronize()
    _assert_equal(captured, eager, "graph")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the callers
# ---------------------------------------------------------------------------------------------------------------------------

def test_registration_icp_point_to_plane():
    src, tgt, nrm, _, _ = reference_run("noisy")
    T0 = _perturb(np.eye(4), 0.5, 0.01, 7)
    r = gmf_amd.registration_icp(src, _g(tgt), R.TAU, init=T0, estimation="point_to_plane", target_normals=nrm)
    T, fit, rmse, _, nn = _one(src, tgt, nrm, T0)
    assert _eq(r.transformation, T[0])
    assert r.fitness == float(fit[0]) and r.inlier_rmse == float(rmse[0])
    nn = nn[0].cpu()
    rows = torch.nonzero(nn >= 0).view(-1)
    assert torch.equal(r.correspondence_set.cpu(), torch.stack([rows, nn[rows]], 1)) and len(rows) > 1000
    # the default is still point-to-point
    p = gmf_amd.registration_icp(_g(src), _g(tgt), R.TAU, init=_g(T0))
    assert _eq(p.transformation, gmf_amd.icp_point_to_point_batched(_g(src)[None], _g(tgt)[None], _g(T0)[None], R.TAU)[0][0])


VOXELS, PASSES = (0.1, 0.05, 0.025), (50, 30, 14)
FRAGMENT_ROWS = 90000                                       # about 7000 rows per m^2: three per finest voxel


def _fragments():
    """Three overlapping fragments cut from the corner scene (fragment k: the surface up to 1.5 along axis k, a random 70 % of
    its rows), each in its own frame.  -> clouds, poses (fragment -> world, pose 0 = I)."""
    r = np.random.default_rng([2, 0xf4a6])
    X, _ = R.corner_surface(r, FRAGMENT_ROWS)
    clouds, poses = [], []
    for k in range(3):
        keep = (X[:, k] <= 1.5) & (r.random(len(X)) < 0.7)
        P = np.eye(4)
        if k:
            P[:3, :3] = R.rotation(r.normal(size=3), 10.0)
            P[:3, 3] = r.uniform(-0.2, 0.2, 3)
        Pi = np.linalg.inv(P)
        clouds.append((X[keep] @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32))
        poses.append(P)
    return clouds, poses


def _pose_gates(T, Tg, where):
    T = np.asarray(T, np.float64)
    assert R.rotation_error_deg(T, Tg) < 0.1, (where, R.rotation_error_deg(T, Tg))
    assert np.linalg.norm(T[:3, 3] - Tg[:3, 3]) < 0.01, (where, np.linalg.norm(T[:3, 3] - Tg[:3, 3]))


def test_local_refinement_point_to_plane_equals_the_chain():
    clouds, poses = _fragments()
    pts = _g(np.concatenate(clouds))
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist()
    src, tgt = [0, 1], [1, 2]
    Xg = [np.linalg.inv(poses[t]) @ poses[s] for s, t in zip(src, tgt)]
    init = _g(np.stack([_perturb(X, 3.0, 0.04, 40 + e) for e, X in enumerate(Xg)]))
    T, info = gmf_amd.local_refinement_batched(pts, off, src, tgt, init, voxel_size=VOXELS, max_iter=PASSES,
                                               estimation="point_to_plane")
    # the same chain from the public functions, edge by edge
    Tc = init.clone()
    for vs, it in zip(VOXELS, PASSES):
        down, doff = gmf_amd.voxel_down_sample_batched(pts, off, vs)
        doff = doff.tolist()
        nrm = gmf_amd.estimate_normals_batched(down, doff, 2 * vs, 30)
        # every down-sampled row has at least 3 rows within 2 voxels (itself included, as the normals' neighbour set counts):
        # no normal is the (0, 0, 1) of a row without neighbours
        for f in range(3):
            c = down[doff[f]:doff[f + 1]].cpu().numpy().astype(np.float64)
            d, _ = cKDTree(c).query(c, k=3, distance_upper_bound=2 * vs)
            assert np.isfinite(d).all(), (vs, f, int((~np.isfinite(d)).any(1).sum()))
        for e, (s, t) in enumerate(zip(src, tgt)):
            cs, ct = down[doff[s]:doff[s + 1]], down[doff[t]:doff[t + 1]]
            Tc[e] = gmf_amd.icp_point_to_plane_batched(cs[None], ct[None], nrm[doff[t]:doff[t + 1]][None], Tc[e][None].contiguous(),
                                                       0.05 * 1.4, max_iteration=it, search="grid")[0][0]
    assert bool(torch.isfinite(T).all()) and _eq(T, Tc)
    assert _eq(info, gmf_amd.information_matrix_batched(down, doff, src, tgt, Tc, 1.4 * VOXELS[-1])[0])
    for e in range(2):
        _pose_gates(T[e].cpu().numpy(), Xg[e], e)
    # a budget that splits the edges into chunks of one changes no bit
    T1, info1 = gmf_amd.local_refinement_batched(pts, off, src, tgt, init, voxel_size=VOXELS, max_iter=PASSES,
                                                 estimation="point_to_plane", memory_budget=1)
    assert _eq(T1, T) and _eq(info1, info)
    # and the default estimator is still the point-to-point one
    Tp = gmf_amd.local_refinement_batched(pts, off, src, tgt, init, voxel_size=VOXELS[:1], max_iter=PASSES[:1])[0]
    Te = gmf_amd.local_refinement_batched(pts, off, src, tgt, init, voxel_size=VOXELS[:1], max_iter=PASSES[:1],
                                          estimation="point_to_point")[0]
    assert _eq(Tp, Te) and not _eq(Tp, gmf_amd.local_refinement_batched(pts, off, src, tgt, init, voxel_size=VOXELS[:1],
                                                                        max_iter=PASSES[:1], estimation="point_to_plane")[0])


def test_multiway_registration_point_to_plane():
    clouds, poses = _fragments()
    pts = _g(np.concatenate(clouds))
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist()
    src, tgt = [0, 1, 0], [1, 2, 2]
    X = np.stack([_perturb(np.linalg.inv(poses[t]) @ poses[s], 1.0, 0.02, 50 + e) for e, (s, t) in enumerate(zip(src, tgt))])
    out = gmf_amd.multiway_registration(pts, off, src, tgt, _g(X), voxel_size=VOXELS, max_iter=PASSES,
                                        icp_estimation="point_to_plane")
    torch.cuda.synchronize()
    P = out["poses"].cpu().numpy()
    assert np.isfinite(P).all() and out["kept"].cpu().numpy().all()
    for f in range(3):
        _pose_gates(P[f], poses[f], f)
    gmf_amd.check_status()
