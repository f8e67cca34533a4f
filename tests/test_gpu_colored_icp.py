"""GPU tests of coloured ICP: the colour gradients (csrc/pointcloud_kernels.hip, k_color_gradient), the coloured step
(csrc/solver_kernels.hip, k_icp_color_partials), the voxel grid with colours and the multi-scale chain
(gmf_amd.color_gradients_batched, icp_colored_batched, registration_colored_icp, voxel_down_sample_colored_batched,
colored_refinement_batched).

The device is held to the float64 restatement in tests/colored_icp_reference.py with the project's 1e-4 gates; everything else is
exact: the search, the batch, the sign of the normals, graph capture, gradients passed or computed and the chain change no bit.

Measured on an MI355X (the figures each test prints):
  gradients, max |g - g_ref| / max |g_ref|: clean 3.5e-8, noisy 3.5e-8, small 3.5e-8, corner 3.4e-8 (gate 1e-4: the rounding
  of the result to fp32);
  icp_colored_batched, max |dT|: clean 7.8e-10, noisy 2.4e-8, small 2.5e-8, corner 1.1e-8, with non-finite rows 1.3e-8
  (gate 1e-4)."""

import math

import numpy as np
import pytest
import torch

import gmf_amd
import colored_icp_reference as C
from gmf_amd.solvers import ICP_PLANE_ROWS
from test_colored_icp_host import reference_run, scene

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("T", "fitness", "inlier_rmse", "iterations", "nn")
EYE = np.eye(4, dtype=np.float32)
CASES = [("plane", name) for name in C.PLANE_CASES] + [("corner", "corner")]
IDS = [name for _, name in CASES]
GATE = 1e-4


def _g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _eq(a, b):
    return torch.equal(a.cpu(), b.cpu())


def _colored(s, q, cs, ct, n, T0, tau=C.TAU, **kw):
    s, q, cs, ct, n, T0 = (x if torch.is_tensor(x) else _g(x) for x in (s, q, cs, ct, n, T0))
    if kw.get("target_gradients") is not None and not torch.is_tensor(kw["target_gradients"]):
        kw["target_gradients"] = _g(kw["target_gradients"])
    return gmf_amd.icp_colored_batched(s, q, cs, ct, n, T0, tau, **kw)


def _one(sc, T0=EYE, nrm=None, cs=None, ct=None, **kw):
    """One pair given as a scene."""
    nrm = sc["nrm"] if nrm is None else nrm
    cs = sc["cs"] if cs is None else cs
    ct = sc["ct"] if ct is None else ct
    if kw.get("target_gradients") is not None:
        kw["target_gradients"] = np.asarray(kw["target_gradients"])[None]
    return _colored(sc["src"][None], sc["tgt"][None], cs[None], ct[None], nrm[None], np.asarray(T0, np.float32)[None], **kw)


def _assert_equal(a, b, where=""):
    for k, name in enumerate(NAMES):
        assert bool(torch.isfinite(a[k].double()).all()), (where, name)            # (NaN would make torch.equal vacuous)
        assert _eq(a[k], b[k]), (where, name)


_DEVICE_RUNS = {}


def device_run(kind, name):
    """The device's result from the identity with everything at its default, computed once."""
    if (kind, name) not in _DEVICE_RUNS:
        _DEVICE_RUNS[kind, name] = [x.clone() for x in _one(scene(kind, name))]
    return _DEVICE_RUNS[kind, name]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_gradients_match_restatement(kind, name):
    sc = scene(kind, name)
    for colors in (sc["ct"], sc["It"]):                      # colours, or the intensity itself: the same bits
        g = gmf_amd.color_gradients_batched(_g(sc["tgt"]), _g(sc["nrm"]), _g(colors), None, 2 * C.TAU, C.MAX_NN)
        g = g.cpu().numpy().astype(np.float64)
        ref = sc["G64"]
        err, scale = np.abs(g - ref).max(), np.abs(ref).max()
        print(f"{name}: max|g - g_ref| = {err:.3e}, max|g_ref| = {scale:.3e}, ratio {err / scale:.3e}, zeroed {int(sc['zeroed'].sum())}")
        assert np.isfinite(g).all() and err <= GATE * scale, (err, scale)
        assert (g[sc["zeroed"]] == 0).all()
        assert (np.abs(g[~sc["zeroed"]]).sum(1) > 0).all()


def test_gradients_of_a_ragged_batch_equal_the_clouds_alone():
    scs = [scene(kind, name) for kind, name in CASES]
    off = np.concatenate([[0], np.cumsum([len(s["tgt"]) for s in scs])]).tolist()
    P, N, Cc = (_g(np.concatenate([s[k] for s in scs])) for k in ("tgt", "nrm", "ct"))
    g = gmf_amd.color_gradients_batched(P, N, Cc, off, 2 * C.TAU)
    flip = _g(np.where(np.random.default_rng(5).random((P.shape[0], 1)) < 0.5, np.float32(-1), np.float32(1)))
    assert _eq(gmf_amd.color_gradients_batched(P, N * flip, Cc, off, 2 * C.TAU), g)          # the normals' signs
    for b, s in enumerate(scs):
        one = gmf_amd.color_gradients_batched(_g(s["tgt"]), _g(s["nrm"]), _g(s["ct"]), None, 2 * C.TAU)
        assert _eq(g[off[b]:off[b + 1]], one), b


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_matches_restatement(kind, name):
    sc = reference_run(kind, name)
    Tr, fr, rr, itr, nnr, rejected = sc["run"]
    T, fit, rmse, it, nn = device_run(kind, name)
    T = T[0].cpu().numpy().astype(np.float64)
    dT = np.abs(T - Tr).max()
    print(f"{name}: max|dT| = {dT:.3e}, fitness {float(fit[0]):.6f} / {fr:.6f}, rmse {float(rmse[0]):.6e} / {rr:.6e}, "
          f"passes {int(it[0])} / {itr}")
    assert rejected == 0
    assert int(it[0]) == itr
    assert np.array_equal(nn[0].cpu().numpy(), nnr)
    assert dT <= GATE, dT
    assert abs(float(fit[0]) - fr) <= 1e-6 and abs(float(rmse[0]) - rr) <= 1e-4 * rr + 1e-7


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_ground_truth(kind, name):
    """The device is no further from the truth than the restatement plus what the 1e-4 gate on T's entries allows: sqrt(3) 1e-4
    in the translation, and in the rotation the angle between two rotations whose entries differ by 1e-4, at most
    |dR|_F / sqrt(2) (1 + O(angle^2)) = 3e-4 / sqrt(2) rad."""
    sc = reference_run(kind, name)
    T = device_run(kind, name)[0][0].cpu().numpy().astype(np.float64)
    rot, tr = C.rotation_error_deg(T, sc["Tg"]), C.translation_error(T, sc["Tg"])
    rot_r, tr_r = C.rotation_error_deg(sc["run"][0], sc["Tg"]), C.translation_error(sc["run"][0], sc["Tg"])
    print(f"{name}: device {rot:.5f} deg {1e3 * tr:.4f} mm, restatement {rot_r:.5f} deg {1e3 * tr_r:.4f} mm")
    assert tr <= tr_r + math.sqrt(3) * GATE
    assert rot <= rot_r + math.degrees(1.01 * 3 * GATE / math.sqrt(2))
    if kind == "plane":                                      # and it is the motion point-to-plane ICP cannot see
        assert rot <= 2.0 / 5 and tr <= 0.03 / 5
        p = gmf_amd.icp_point_to_plane_batched(_g(sc["src"])[None], _g(sc["tgt"])[None], _g(sc["nrm"])[None], _g(EYE)[None], C.TAU)
        assert _eq(p[0][0], torch.as_tensor(EYE)) and int(p[3][0]) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact equalities
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_brute_equals_grid(kind, name):
    out = device_run(kind, name)
    assert int(out[3][0]) >= 2
    _assert_equal(_one(scene(kind, name), search="grid"), out, name)


@pytest.mark.parametrize("search", ["brute", "grid"])
def test_ragged_batch_equals_pairs(search):
    scs = [scene(kind, name) for kind, name in CASES]
    # and a pair short of one part, one of exactly a part and one just over it, cut from the corner scene
    for ns in (ICP_PLANE_ROWS - 1, ICP_PLANE_ROWS, ICP_PLANE_ROWS + 1):
        s = dict(scene("corner", "corner"))
        s["src"], s["cs"], s["Is"] = s["src"][:ns], s["cs"][:ns], s["Is"][:ns]
        scs.append(s)
    soff = np.concatenate([[0], np.cumsum([len(s["src"]) for s in scs])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(s["tgt"]) for s in scs])]).tolist()
    S, Q, Cs, Ct, N = (np.concatenate([s[k] for s in scs]) for k in ("src", "tgt", "cs", "ct", "nrm"))
    I = np.stack([EYE] * len(scs))
    out = _colored(S, Q, Cs, Ct, N, I, source_offsets=soff, target_offsets=toff, search=search)
    for b, s in enumerate(scs):
        one = _one(s, search=search)
        for k in range(4):
            assert bool(torch.isfinite(out[k][b].double()).all()), (b, NAMES[k])
            assert _eq(out[k][b], one[k][0]), (b, NAMES[k])
        assert _eq(out[4][soff[b]:soff[b + 1]], one[4][0]), b
        assert not torch.equal(out[0][b].cpu(), torch.as_tensor(EYE)) and int(out[3][b]) >= 2
    # device offsets size the grid with the batch's total instead of the largest pair: the same bits
    dso, dto = (torch.tensor(o, dtype=torch.int32, device=DEV) for o in (soff, toff))
    _assert_equal(_colored(S, Q, Cs, Ct, N, I, source_offsets=dso, target_offsets=dto, search=search), out, "device offsets")
    # intensities instead of colours: the same bits
    Is, It = (np.concatenate([s[k] for s in scs]) for k in ("Is", "It"))
    _assert_equal(_colored(S, Q, Is, It, N, I, source_offsets=soff, target_offsets=toff, search=search), out, "intensities")


@pytest.mark.parametrize("kind,name", [("plane", "noisy"), ("corner", "corner")], ids=["noisy", "corner"])
def test_sign_flips_change_no_bit(kind, name):
    sc = scene(kind, name)
    flip = np.where(np.random.default_rng(3).random((len(sc["nrm"]), 1)) < 0.5, np.float32(-1), np.float32(1))
    assert 0.4 < (flip < 0).mean() < 0.6
    _assert_equal(_one(sc, nrm=sc["nrm"] * flip), device_run(kind, name), "flipped")


@pytest.mark.parametrize("search", ["brute", "grid"])
def test_max_iteration_zero_equals_point_to_point(search):
    """All five outputs.  (inlier_rmse is the same fp64 sum of d^2 taken in the split step's tree instead of k_icp_step's: equal
    after the rounding to fp32 on these inputs, as the restatement's 1e-16 against fp32's 6e-8 lets one expect.)"""
    sc = scene("plane", "noisy")
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, 3] = [0.004, -0.003, 0.002]
    a = _one(sc, T0, max_iteration=0, search=search)
    b = gmf_amd.icp_point_to_point_batched(_g(sc["src"])[None], _g(sc["tgt"])[None], _g(T0)[None], C.TAU, max_iteration=0, search=search)
    _assert_equal(a, b, search)
    assert int(a[3][0]) == 0 and float(a[1][0]) > 0.9 and float(a[2][0]) > 1e-3


def test_graph_capture_equals_eager():
    scs = [scene(kind, name) for kind, name in CASES]
    soff = np.concatenate([[0], np.cumsum([len(s["src"]) for s in scs])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(s["tgt"]) for s in scs])]).tolist()
    S, Q, Cs, Ct, N = (_g(np.concatenate([s[k] for s in scs])) for k in ("src", "tgt", "cs", "ct", "nrm"))
    I = _g(np.stack([EYE] * len(scs)))

    def run():
        return _colored(S, Q, Cs, Ct, N, I, source_offsets=soff, target_offsets=toff, search="grid")

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
    assert int(eager[3].min()) >= 2


@pytest.mark.parametrize("kind,name", [("plane", "small"), ("corner", "corner")], ids=["small", "corner"])
def test_gradients_passed_equal_gradients_computed(kind, name):
    sc = scene(kind, name)
    G = gmf_amd.color_gradients_batched(_g(sc["tgt"]), _g(sc["nrm"]), _g(sc["ct"]), None, 2 * C.TAU, C.MAX_NN)
    _assert_equal(_colored(sc["src"][None], sc["tgt"][None], sc["cs"][None], sc["ct"][None], sc["nrm"][None], EYE[None],
                           target_gradients=G[None]), device_run(kind, name), name)
    # and they are used: other gradients give another pose
    other = _colored(sc["src"][None], sc["tgt"][None], sc["cs"][None], sc["ct"][None], sc["nrm"][None], EYE[None],
                     target_gradients=torch.zeros_like(G)[None])
    assert not _eq(other[0], device_run(kind, name)[0])


def test_registration_colored_icp():
    sc = scene("plane", "small")
    r = gmf_amd.registration_colored_icp(sc["src"], _g(sc["tgt"]), sc["cs"], _g(sc["ct"]), sc["nrm"], C.TAU)
    T, fit, rmse, _, nn = device_run("plane", "small")
    assert _eq(r.transformation, T[0])
    assert r.fitness == float(fit[0]) and r.inlier_rmse == float(rmse[0])
    nn = nn[0].cpu()
    rows = torch.nonzero(nn >= 0).view(-1)
    assert torch.equal(r.correspondence_set.cpu(), torch.stack([rows, nn[rows]], 1)) and len(rows) > 200
    ri = gmf_amd.registration_colored_icp(sc["src"], sc["tgt"], sc["Is"], sc["It"], sc["nrm"], C.TAU, init=np.eye(4), search="grid")
    assert _eq(ri.transformation, T[0])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. non-finite inputs
# ---------------------------------------------------------------------------------------------------------------------------

def test_non_finite_rows_add_nothing():
    sc = scene("corner", "corner")
    nt, ns = len(sc["tgt"]), len(sc["src"])
    r = np.random.default_rng(12)
    pick = r.random(nt)
    bad_c, bad_g, bad_n = pick < 0.07, (pick >= 0.07) & (pick < 0.14), (pick >= 0.14) & (pick < 0.21)
    bad_s = r.random(ns) < 0.05
    It, G, nrm, Is = sc["It"].copy(), sc["G"].copy(), sc["nrm"].copy(), sc["Is"].copy()
    It[bad_c] = np.nan
    G[bad_g, 1] = np.nan
    G[bad_g & (np.arange(nt) % 2 == 0), 0] = np.inf
    nrm[bad_n, 2] = np.nan
    Is[bad_s] = np.inf
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, 3] = [0.004, -0.003, 0.002]
    # C, fitness and rmse do not see them
    a0 = _one(sc, T0, nrm=nrm, cs=Is, ct=It, target_gradients=G, max_iteration=0)
    c0 = _one(sc, T0, cs=sc["Is"], ct=sc["It"], target_gradients=sc["G"], max_iteration=0)
    _assert_equal(a0, c0, "pass 0")
    nn0 = a0[4][0].cpu().numpy()
    met = nn0[nn0 >= 0]
    assert bad_c[met].sum() > 20 and bad_g[met].sum() > 20 and bad_n[met].sum() > 20 and (bad_s & (nn0 >= 0)).sum() > 20
    # the same rows dropped through the normals alone: the same bits
    a = _one(sc, nrm=nrm, cs=Is, ct=It, target_gradients=G)
    only_n = sc["nrm"].copy()
    only_n[bad_c | bad_g | bad_n, 0] = np.nan
    b = _one(sc, nrm=only_n, cs=Is, ct=sc["It"], target_gradients=sc["G"])
    _assert_equal(a, b, "dropped through the normals")
    assert int(a[3][0]) >= 2 and not _eq(a[0], device_run("corner", "corner")[0])
    # and the restatement, which leaves those rows' terms out
    Tr, fr, rr, itr, nnr, rejected = C.icp_colored_np(sc["src"], sc["tgt"], Is, It, nrm, G, np.eye(4), C.TAU)
    dT = np.abs(a[0][0].cpu().numpy().astype(np.float64) - Tr).max()
    print(f"non-finite rows: max|dT| = {dT:.3e}, passes {int(a[3][0])} / {itr}")
    assert rejected == 0 and int(a[3][0]) == itr and np.array_equal(a[4][0].cpu().numpy(), nnr) and dT <= GATE
    assert abs(float(a[1][0]) - fr) <= 1e-6 and abs(float(a[2][0]) - rr) <= 1e-4 * rr


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the voxel grid with colours
# ---------------------------------------------------------------------------------------------------------------------------

def test_voxel_grid_with_colours():
    scs = [scene("corner", "corner"), scene("plane", "small")]
    off = [0, len(scs[0]["tgt"]), len(scs[0]["tgt"]) + len(scs[1]["tgt"])]
    P, Cc = (_g(np.concatenate([s[k] for s in scs])) for k in ("tgt", "ct"))
    for voxel in (0.05, 0.21):
        pd, cd, od = gmf_amd.voxel_down_sample_colored_batched(P, Cc, off, voxel)
        p0, o0 = gmf_amd.voxel_down_sample_batched(P, off, voxel)
        assert _eq(pd, p0) and _eq(od, o0) and pd.shape == cd.shape and pd.shape[0] < 0.8 * P.shape[0]
        od = od.tolist()
        for b, s in enumerate(scs):
            mp, mc = C.voxel_means_np(s["tgt"], s["ct"], voxel)
            assert od[b + 1] - od[b] == len(mp)
            got_p, got_c = (x[od[b]:od[b + 1]].cpu().numpy() for x in (pd, cd))
            assert np.array_equal(got_p, mp.astype(np.float32))
            ulp = np.spacing(np.abs(mc).astype(np.float32)).astype(np.float64)
            assert (np.abs(got_c.astype(np.float64) - mc) <= ulp).all()
    # one cloud without offsets
    one = gmf_amd.voxel_down_sample_colored_batched(_g(scs[0]["tgt"]), _g(scs[0]["ct"]), None, 0.05)
    assert _eq(one[0], pd.new_tensor(C.voxel_means_np(scs[0]["tgt"], scs[0]["ct"], 0.05)[0].astype(np.float32)))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the multi-scale chain
# ---------------------------------------------------------------------------------------------------------------------------

VOXELS, PASSES = (0.1, 0.05), (20, 10)
FRAGMENT_ROWS = 40000


def _fragments():
    """Three overlapping coloured fragments cut from the corner scene (fragment k: the surface up to 1.5 along axis k, a random
    70 % of its rows), each in its own frame.  -> clouds, colours, poses (fragment -> world, pose 0 = I)."""
    r = np.random.default_rng([2, 0xf4a6])
    X, _ = C.corner_surface(r, FRAGMENT_ROWS)
    col = C.field_colors(X)
    clouds, colors, poses = [], [], []
    for k in range(3):
        keep = (X[:, k] <= 1.5) & (r.random(len(X)) < 0.7)
        P = np.eye(4)
        if k:
            P[:3, :3] = C.rotation(r.normal(size=3), 10.0)
            P[:3, 3] = r.uniform(-0.2, 0.2, 3)
        Pi = np.linalg.inv(P)
        clouds.append((X[keep] @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32))
        colors.append(col[keep])
        poses.append(P)
    return clouds, colors, poses


def _perturb(T, deg, dist, seed):
    r = np.random.default_rng(seed)
    D = np.eye(4)
    D[:3, :3] = C.rotation(r.normal(size=3), deg)
    v = r.normal(size=3)
    D[:3, 3] = dist * v / np.linalg.norm(v)
    return (D @ np.asarray(T, np.float64)).astype(np.float32)


def test_colored_refinement_equals_the_chain():
    clouds, colors, poses = _fragments()
    pts, col = _g(np.concatenate(clouds)), _g(np.concatenate(colors))
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist()
    src, tgt = [0, 1], [1, 2]
    Xg = [np.linalg.inv(poses[t]) @ poses[s] for s, t in zip(src, tgt)]
    init = _g(np.stack([_perturb(X, 2.0, 0.03, 40 + e) for e, X in enumerate(Xg)]))
    T, info = gmf_amd.colored_refinement_batched(pts, col, off, src, tgt, init, voxel_size=VOXELS, max_iter=PASSES)
    # the same chain from the public functions, edge by edge
    Tc = init.clone()
    for vs, it in zip(VOXELS, PASSES):
        down, cdown, doff = gmf_amd.voxel_down_sample_colored_batched(pts, col, off, vs)
        doff = doff.tolist()
        nrm = gmf_amd.estimate_normals_batched(down, doff, 2 * vs, 30)
        grd = gmf_amd.color_gradients_batched(down, nrm, cdown, doff, 2 * 1.4 * vs, 30)
        assert int((grd.abs().sum(1) > 0).sum()) > 0.9 * len(grd)
        for e, (s, t) in enumerate(zip(src, tgt)):
            rs, rt = slice(doff[s], doff[s + 1]), slice(doff[t], doff[t + 1])
            Tc[e] = gmf_amd.icp_colored_batched(down[rs][None], down[rt][None], cdown[rs][None], cdown[rt][None], nrm[rt][None],
                                                Tc[e][None].contiguous(), 1.4 * vs, max_iteration=it, search="grid",
                                                target_gradients=grd[rt][None])[0][0]
    assert bool(torch.isfinite(T).all()) and _eq(T, Tc)
    assert _eq(info, gmf_amd.information_matrix_batched(down, doff, src, tgt, Tc, 1.4 * VOXELS[-1])[0])
    for e in range(2):
        Te = T[e].cpu().numpy().astype(np.float64)
        assert C.rotation_error_deg(Te, Xg[e]) < 0.1 and C.translation_error(Te, Xg[e]) < 0.01, e
    # a budget that splits the edges into chunks of one changes no bit
    T1, info1 = gmf_amd.colored_refinement_batched(pts, col, off, src, tgt, init, voxel_size=VOXELS, max_iter=PASSES, memory_budget=1)
    assert _eq(T1, T) and _eq(info1, info)
