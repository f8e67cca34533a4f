"""The RGB-D odometry on the device (gmf_amd.rgbd; csrc/rgbd_kernels.hip) against its numpy restatement (tests/rgbd_reference.py) on
the fixture of tests/test_rgbd_host.py (48 x 64, five close poses of a textured plane and sphere): planes and correspondence maps
exactly, the sums of an iteration within n 2^-52 sum|terms|, the end-to-end pose within tol = sum_i cond(A_i) n_i 2^-52, the
bound of another summation order (test_rgbd_host.py checks the margins that make it sound).

Observed on an MI355X (printed by the tests): the pose differs from the restatement's by 3.3e-16 to 1.3e-15 entry by entry (tol
1.7e-9 to 3.4e-9: nothing but the order of summation differs), the sums by at most 0.046 of their bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import rgbd_reference as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
K = R.INTRINSIC
POSE_TOL_POSEGRAPH = 16 * 1.399e-14             # tests/test_gpu_multiway.py: TOL["poses"]
CASES = [(0, 1, None), (1, 2, None), (2, 3, None), (3, 4, None), (0, 2, None), (0, 2, (0, 1))]     # (source, target, init)
CASES_B = [(0, 1, None), (2, 3, None), (3, 4, None)]      # the second option set, on the pairs whose margins carry the pose bound


def _dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _g(x, dtype=None):
    return torch.as_tensor(np.array(x), dtype=dtype).to(_dev())          # a copy: the fixtures are read-only


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_planes(got, ref):
    """float32 planes bit for bit, NaN in the same places (a NaN's payload is not compared)."""
    nan = np.isnan(ref)
    return got.dtype == ref.dtype == np.float32 and got.shape == ref.shape and np.array_equal(np.isnan(got), nan) \
        and np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])


def extra_frames():
    """The fixture's five frames, then a frame without depth (5) and two of a constant-colour fronto-parallel plane (6, 7)."""
    gray, depth, _ = R.fixture()
    gray = np.concatenate([gray, gray[:1], np.full((2, R.H, R.W), 128, np.uint8)])
    depth = np.concatenate([depth, np.zeros((1, R.H, R.W), np.uint16), np.full((2, R.H, R.W), 1500, np.uint16)])
    return gray, depth


@pytest.fixture(scope="module")
def pyr():
    import gmf_amd
    gray, depth = extra_frames()
    return gmf_amd.rgbd_pyramids(_g(gray), _g(depth))


@pytest.fixture(scope="module")
def pyr_b():
    import gmf_amd
    gray, depth, _ = R.fixture()
    return gmf_amd.rgbd_pyramids(_g(gray), _g(depth), min_depth=R.OPTIONS_B["min_depth"], max_depth=R.OPTIONS_B["max_depth"])


def run(pyr, cases, **kw):
    """rgbd_odometry(return_trace=True) on (source, target, init) cases -> dict of numpy arrays."""
    import gmf_amd
    init = None
    if any(c[2] is not None for c in cases):
        init = _g(np.stack([np.eye(4) if c[2] is None else (c[2] if isinstance(c[2], np.ndarray) else R.ground_truth(*c[2]))
                            for c in cases]), torch.float64)
    ok, T, info, tr = gmf_amd.rgbd_odometry(pyr, pair_source=[c[0] for c in cases], pair_target=[c[1] for c in cases], intrinsic=K,
                                            odo_init=init, return_trace=True, **kw)
    out = dict(success=ok.cpu().numpy(), T=T.cpu().numpy(), information=info.cpu().numpy())
    out.update({k: v.cpu().numpy() for k, v in tr.items()})
    return out


@pytest.fixture(scope="module")
def batch(pyr):
    return run(pyr, CASES)


# ---- planes -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("crop", [False, True])
def test_planes_bitwise_for_every_input_form(crop):
    import gmf_amd
    gray, depth, _ = R.fixture()
    if crop:
        gray, depth = gray[:, :47, :61], depth[:, :47, :61]
    metres = depth.astype(np.float32) / np.float32(1000.0)
    metres[1, 3, 5], metres[1, 20, 30], metres[2, 7, 7], metres[3, 0, 0] = np.nan, np.inf, -1.0, 0.0
    as_float = (gray.astype(np.float32) * np.float32(0.0037)) + np.float32(0.01)
    forms = [(gray, depth), (R.rgb_of(gray), depth), (as_float, depth), (gray, metres), (R.rgb_of(gray), metres), (as_float, metres)]
    for color, dep in forms:
        ref = R.pyramid(color, dep)
        got = gmf_amd.rgbd_pyramids(_g(color), _g(dep))
        assert got.levels == 3
        for l in range(3):
            g = got.planes(l).cpu().numpy()
            assert g.shape == ref[l].shape == (5, 6, gray.shape[1] >> l, gray.shape[2] >> l)
            for c, name in enumerate(R.NAMES):
                assert same_planes(g[:, c], ref[l][:, c]), (color.dtype, color.ndim, dep.dtype, l, name)
        assert np.isnan(ref[0][:, 1]).any() == (dep.dtype == np.float32)          # the NaN places are exercised by the float depth
    # the depth window: the second option set cuts the far plane's corners and changes the planes
    ref = R.pyramid(gray, depth, depth_trunc=1.6, min_depth=1.0, max_depth=1.55)
    got = gmf_amd.rgbd_pyramids(_g(gray), _g(depth), depth_trunc=1.6, min_depth=1.0, max_depth=1.55)
    assert np.isnan(ref[0][:, 1]).any() and not np.isnan(ref[0][:, 1]).all()
    for l in range(3):
        assert same_planes(got.planes(l).cpu().numpy(), ref[l]), l


# ---- correspondence maps ------------------------------------------------------------------------------------------------------

def test_correspondence_maps_equal(pyr):
    import gmf_amd
    ref = R.fixture_pyramid()
    push = R.PUSH_POSE
    pairs = [(0, 1), (1, 2), (3, 2), (0, 4)]
    poses = [("identity", lambda s, t: np.eye(4)), ("ground truth", R.ground_truth), ("push", lambda s, t: push)]
    cases = [(s, t, name, f(s, t)) for s, t in pairs for name, f in poses]
    T = _g(np.stack([c[3] for c in cases]), torch.float64)
    for l in range(3):
        got = gmf_amd.rgbd_correspondence_map(pyr, [c[0] for c in cases], [c[1] for c in cases], T, K, level=l).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == (len(cases), R.H >> l, R.W >> l)
        for e, (s, t, name, pose) in enumerate(cases):
            want = R.correspondence_map(R.level_intrinsic(K, l), pose, ref[l][s, 1], ref[l][t, 1], 0.03)
            assert np.array_equal(got[e], want), (l, s, t, name, int((got[e] != want).sum()))
            assert (want >= 0).sum() > 30
    # the other tie rule is another map (48 entries differ), so the comparison above tells them apart
    other = R.correspondence_map(K, R.ground_truth(0, 1), ref[0][0, 1], ref[0][1, 1], 0.03, tie_largest=True)
    got_gt = gmf_amd.rgbd_correspondence_map(pyr, [0], [1], _g(R.ground_truth(0, 1)[None], torch.float64), K).cpu().numpy()[0]
    assert int((got_gt != other).sum()) == 48
    got0 = gmf_amd.rgbd_correspondence_map(pyr, [0], [1], _g(np.eye(4)[None], torch.float64), K).cpu().numpy()[0]
    # and max_depth_diff is honoured
    wide = gmf_amd.rgbd_correspondence_map(pyr, [0], [1], _g(np.eye(4)[None], torch.float64), K, max_depth_diff=0.07).cpu().numpy()[0]
    assert np.array_equal(wide, R.correspondence_map(K, np.eye(4), ref[0][0, 1], ref[0][1, 1], 0.07)) and not np.array_equal(wide, got0)


# ---- one iteration from a given pose ------------------------------------------------------------------------------------------

def test_first_iteration_of_every_level_within_the_sum_bound(pyr):
    ref = R.fixture_pyramid()
    worst = 0.0
    for l, its in ((2, (1, 0, 0)), (1, (0, 1, 0)), (0, (0, 0, 1))):
        starts = []
        for s, t, init in CASES:
            r = R.fixture_odometry(s, t, init)
            starts.append((s, t, next(it["T_in"] for it in r["trace"] if it["level"] == l)))
        got = run(pyr, starts, iterations=its)
        for e, (s, t, T_in) in enumerate(starts):
            Ps, Pt = [p[s] for p in ref], [p[t] for p in ref]
            sc = R.scales(R.correspondence_map(K, T_in, Ps[0][1], Pt[0][1], 0.03), Ps[0][0], Pt[0][0])
            Kl = R.level_intrinsic(K, l)
            J, r = R.jacobian_rows(Kl, T_in, Ps[l], Pt[l], R.correspondence_map(Kl, T_in, Ps[l][1], Pt[l][1], 0.03), *sc)
            want = R.sums(J, r)
            n = want["n"]
            n0 = int((R.correspondence_map(K, T_in, Ps[0][1], Pt[0][1], 0.03) >= 0).sum())
            assert got["n"][e, 0] == n and n > 100, (l, s, t)
            assert np.all(np.abs(got["scales"][e] - sc) <= n0 * EPS * np.abs(sc)), (l, s, t, got["scales"][e], sc)
            for key in ("A", "b", "r2"):
                diff, bound = np.abs(got[key][e, 0] - want[key]), n * EPS * np.asarray(want[key + "_abs"])
                worst = max(worst, float(np.max(diff / bound)))
                assert np.all(diff <= bound), (l, s, t, key, float(np.max(diff / bound)))
            x = np.linalg.solve(want["A"], -want["b"])
            assert np.allclose(got["x"][e, 0], x, rtol=0, atol=np.linalg.cond(want["A"]) * n * EPS * max(1.0, np.abs(x).max()))
            assert same_bits(got["pose"][e, 0], got["T"][e])
    print(f"sums: largest |difference| / (n 2^-52 sum|terms|) = {worst:.3e}")


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def check_end_to_end(got, cases, options):
    worst = 0.0
    for e, (s, t, init) in enumerate(cases):
        r = R.fixture_odometry(s, t, init, options)
        assert r["success"] and got["success"][e], (s, t, init)
        assert got["n"][e].tolist() == [it["n"] for it in r["trace"]], (s, t, init)
        tol = r["tol"]
        d = float(np.abs(got["T"][e] - r["T"]).max())
        worst = max(worst, d / tol)
        print(f"pair {s}->{t} init {init} options {options}: max|T - T_ref| = {d:.3e} (tol {tol:.3e})")
        assert d <= tol, (s, t, init)
        G, G_abs = r["information"], r["information_abs"]
        count = int(G[5, 5])
        assert got["information"][e, 3, 3] == got["information"][e, 4, 4] == got["information"][e, 5, 5] == count
        assert np.all(np.abs(got["information"][e] - G) <= count * EPS * G_abs), (s, t, init)
        assert np.array_equal(got["information"][e], got["information"][e].T)
        gt = R.ground_truth(s, t)
        (rot, tr), (rot_ref, tr_ref) = R.pose_error(got["T"][e], gt), R.pose_error(r["T"], gt)
        assert tr <= tr_ref + tol and np.radians(rot) <= np.radians(rot_ref) + tol          # metres and radians
        # the margins of test_rgbd_host.py against what the device actually moved, over every iteration's pose
        moved = max(float(np.abs(got["pose"][e, i] - it["T"]).max()) for i, it in enumerate(r["trace"]))
        assert r["pixel_margin"] > 10 * moved * (K[0] + 1) and r["depth_margin"] > 10 * moved * 2, (s, t, init, moved)
        assert rot < 0.6 and tr < 0.010                       # and the motion is found: 1.15 deg / 13.6 mm per step to start with
    return worst


def test_end_to_end_pose_counts_and_information(batch, pyr_b):
    worst = check_end_to_end(batch, CASES, "A")
    got_b = run(pyr_b, CASES_B, max_depth_diff=R.OPTIONS_B["max_depth_diff"])
    worst = max(worst, check_end_to_end(got_b, CASES_B, "B"))
    print(f"pose: largest |difference| / tol = {worst:.3e}")
    assert not same_bits(got_b["T"][0], batch["T"][0])


def test_failures_beside_a_good_pair(pyr, batch):
    got = run(pyr, [(0, 5, None), (1, 2, None), (6, 7, None), (5, 0, None)])
    assert got["success"].tolist() == [False, True, False, False]
    for e in (0, 2, 3):
        assert np.array_equal(got["T"][e], np.eye(4)) and np.array_equal(got["information"][e], np.eye(6))
    # no level-0 correspondence: nothing runs, no scales; the flat plane: scales, one iteration whose system is singular
    assert (got["n"][0] == -1).all() and np.isnan(got["scales"][0]).all() and (got["n"][3] == -1).all()
    assert got["n"][2, 0] > 100 and (got["n"][2, 1:] == -1).all() and np.isfinite(got["scales"][2]).all()
    assert np.isfinite(got["A"][2, 0]).all() and abs(np.linalg.det(got["A"][2, 0])) < 1e-6 and np.isnan(got["x"][2, 0]).all()
    for key in ("T", "information", "n", "A", "b", "r2", "x", "pose", "scales"):
        assert same_bits(got[key][1], batch[key][1]), key


def test_two_runs_and_any_batch_position_have_the_same_bits(pyr, batch):
    again = run(pyr, CASES)
    assert all(same_bits(again[k], batch[k]) for k in batch)
    alone = run(pyr, [CASES[1]])
    for pos in (0, 3, 5):
        order = [c for c in CASES if c != CASES[1]]
        order.insert(pos, CASES[1])
        got = run(pyr, order)
        for key in batch:
            assert same_bits(got[key][pos], alone[key][0]) and same_bits(alone[key][0], batch[key][1]), (pos, key)


def test_frames_given_directly_equal_the_pyramids(batch):
    import gmf_amd
    gray, depth = extra_frames()
    ok, T, info = gmf_amd.rgbd_odometry(_g(gray), _g(depth), pair_source=[1], pair_target=[2], intrinsic=K)
    assert ok.dtype == torch.bool and ok.tolist() == [True] and T.dtype == info.dtype == torch.float64
    assert same_bits(T.cpu().numpy()[0], batch["T"][1]) and same_bits(info.cpu().numpy()[0], batch["information"][1])
    # the last row of odo_init is not read: the pose that comes back ends in 0 0 0 1
    init = np.stack([R.ground_truth(0, 1), R.ground_truth(0, 1)])
    init[1, 3] = [5.0, -2.0, float("nan"), 0.5]
    ok, T, info = gmf_amd.rgbd_odometry(_g(gray), _g(depth), pair_source=[0, 0], pair_target=[2, 2], intrinsic=K,
                                        odo_init=_g(init, torch.float64))
    assert ok.tolist() == [True, True] and same_bits(T.cpu().numpy()[0], batch["T"][5]) and same_bits(T.cpu().numpy()[1], batch["T"][5])
    assert T[1, 3].tolist() == [0.0, 0.0, 0.0, 1.0] and same_bits(info.cpu().numpy()[1], batch["information"][5])
    none = gmf_amd.rgbd_odometry(_g(gray), _g(depth), pair_source=[], pair_target=[], intrinsic=K)
    assert none[0].shape == (0,) and none[1].shape == (0, 4, 4) and none[2].shape == (0, 6, 6)


def test_more_pairs_than_run_together_have_the_bits_of_a_small_call():
    """Pairs run together in chunks (the level-0 maps within 1 GiB, at most 65535 pairs: a grid's y extent).  At 12 x 16 pixels
    65600 pairs are two chunks; the pairs around the seam and the last ones equal the same pairs in a call of their own."""
    import gmf_amd
    gray, depth, _ = R.fixture()
    rows, cols = slice(16, 28), slice(24, 40)                                   # the sphere's edge over the plane
    Kc = (K[0], K[1], K[2] - 24, K[3] - 16)
    pyr = gmf_amd.rgbd_pyramids(_g(gray[:, rows, cols]), _g(depth[:, rows, cols]), levels=1)
    E = 65600
    src = [(3 * e) % 5 for e in range(E)]
    tgt = [(s + 1 + e % 3) % 5 for e, s in enumerate(src)]
    init = np.tile(np.eye(4), (E, 1, 1))
    init[:, 0, 3] = 1e-4 * (np.arange(E) % 7)
    init_dev = _g(init, torch.float64)
    ok, T, info, tr = gmf_amd.rgbd_odometry(pyr, pair_source=src, pair_target=tgt, intrinsic=Kc, odo_init=init_dev, iterations=(3,),
                                            return_trace=True)
    cmap = gmf_amd.rgbd_correspondence_map(pyr, src, tgt, init_dev, Kc)
    assert cmap.shape == (E, 12, 16)
    pick = [0, 1, 65533, 65534, 65535, 65536, 65537, E - 2, E - 1]
    idx = torch.tensor(pick, device=_dev())
    ok1, T1, info1, tr1 = gmf_amd.rgbd_odometry(pyr, pair_source=[src[e] for e in pick], pair_target=[tgt[e] for e in pick], intrinsic=Kc,
                                                odo_init=init_dev[idx], iterations=(3,), return_trace=True)
    cmap1 = gmf_amd.rgbd_correspondence_map(pyr, [src[e] for e in pick], [tgt[e] for e in pick], init_dev[idx], Kc)
    assert torch.equal(cmap[idx], cmap1) and (cmap1 >= 0).sum(dim=(1, 2)).min() > 50
    assert (tr1["n"][:, 0] > 50).all()                                        # the iterations ran
    assert torch.equal(ok[idx], ok1)
    for a, b in ((T, T1), (info, info1)) + tuple((tr[k], tr1[k]) for k in tr):
        assert same_bits(a[idx].cpu().numpy(), b.cpu().numpy())


# ---- the C entries ------------------------------------------------------------------------------------------------------------

def test_c_entries_with_nan_filled_outputs(pyr, batch):
    """gmf_rgbd_pyramids, gmf_rgbd_correspondences and gmf_rgbd_odometry called directly: what the header names is written, and
    nothing else."""
    from gmf_amd._util import handle_and_stream
    dev = _dev()
    gray, depth = extra_frames()
    F, H, W, L = 8, R.H, R.W, 3
    total = sum(F * 6 * (H >> l) * (W >> l) for l in range(L))
    col, dep = _g(gray), _g(depth)
    h, st = handle_and_stream(dep)
    buf = torch.full((total + 6 * 12 * 16,), float("nan"), device=dev)
    h.call("gmf_rgbd_pyramids", col.data_ptr(), 0, dep.data_ptr(), 1, F, H, W, 1000.0, 3.0, 0.0, 4.0, L, buf.data_ptr(), st)
    assert same_planes(buf[:total].cpu().numpy(), pyr._buffer.cpu().numpy()) and torch.isnan(buf[total:]).all()
    E = 2
    src, tgt = _g([1, 0], torch.int32), _g([2, 5], torch.int32)
    poses = _g(np.stack([np.eye(4), np.eye(4)]), torch.float64)
    for l in range(L):
        hw = (H >> l) * (W >> l)
        cmap = torch.full((E + 1, hw), -77, dtype=torch.int32, device=dev)
        h.call("gmf_rgbd_correspondences", buf.data_ptr(), F, H, W, L, l, src.data_ptr(), tgt.data_ptr(), E, poses.data_ptr(), *K, 0.03,
               cmap.data_ptr(), st)
        ref = R.fixture_pyramid()[l]
        want = R.correspondence_map(R.level_intrinsic(K, l), np.eye(4), ref[1, 1], ref[2, 1], 0.03)
        assert np.array_equal(cmap[0].cpu().numpy(), want.ravel()) and (cmap[1] == -1).all() and (cmap[2] == -77).all()
    its = (20, 10, 5)
    N = sum(its)
    ok = torch.full((E + 1,), 7, dtype=torch.uint8, device=dev)
    T = torch.full((E + 1, 16), float("nan"), dtype=torch.float64, device=dev)
    info = torch.full((E + 1, 36), float("nan"), dtype=torch.float64, device=dev)
    scales = torch.full((E + 1, 2), float("nan"), dtype=torch.float64, device=dev)
    tn = torch.full((E + 1, N), -77, dtype=torch.int32, device=dev)
    td = torch.full((E + 1, N, 65), float("nan"), dtype=torch.float64, device=dev)
    h.call("gmf_rgbd_odometry", buf.data_ptr(), F, H, W, L, src.data_ptr(), tgt.data_ptr(), E, None, *K, 0.03, (C.c_int * 3)(*its),
           ok.data_ptr(), T.data_ptr(), info.data_ptr(), scales.data_ptr(), tn.data_ptr(), td.data_ptr(), st)
    assert ok.tolist() == [1, 0, 7]
    assert same_bits(T[0].cpu().numpy().reshape(4, 4), batch["T"][1]) and same_bits(info[0].cpu().numpy().reshape(6, 6), batch["information"][1])
    assert np.array_equal(T[1].cpu().numpy().reshape(4, 4), np.eye(4)) and np.array_equal(info[1].cpu().numpy().reshape(6, 6), np.eye(6))
    assert torch.isnan(T[2]).all() and torch.isnan(info[2]).all() and torch.isnan(scales[1:]).all()
    assert same_bits(scales[0].cpu().numpy(), batch["scales"][1])
    assert tn[0].cpu().numpy().tolist() == batch["n"][1].tolist() and (tn[1:] == -77).all()
    assert not torch.isnan(td[0]).any() and torch.isnan(td[1:]).all()
    assert same_bits(td[0, :, 49:].cpu().numpy().reshape(N, 4, 4), batch["pose"][1])
    # without the optional outputs
    ok.fill_(7)
    h.call("gmf_rgbd_odometry", buf.data_ptr(), F, H, W, L, src.data_ptr(), tgt.data_ptr(), E, None, *K, 0.03, (C.c_int * 3)(*its),
           ok.data_ptr(), T.data_ptr(), info.data_ptr(), None, None, None, st)
    assert ok.tolist() == [1, 0, 7] and same_bits(T[0].cpu().numpy().reshape(4, 4), batch["T"][1])


# ---- fragments ----------------------------------------------------------------------------------------------------------------

def test_rgbd_fragments():
    import gmf_amd
    import tsdf_reference as TR
    gray, depth, poses_gt = R.fixture()
    off = [0, 3, 3, 5]
    args = dict(TR.fixture_args())
    col, dep = _g(gray), _g(depth)
    pts, poff, poses, ok = gmf_amd.rgbd_fragments(col, dep, K, frame_offsets=off, optimize=False, **args)
    assert ok.tolist() == [True, True, True] and poses.shape == (5, 4, 4) and poses.dtype == torch.float64
    pairs = [(0, 1), (1, 2), (3, 4)]
    o = R.OPTIONS_B
    ok2, X, info = gmf_amd.rgbd_odometry(col, dep, pair_source=[p[0] for p in pairs], pair_target=[p[1] for p in pairs], intrinsic=K,
                                         max_depth_diff=o["max_depth_diff"], min_depth=o["min_depth"], max_depth=o["max_depth"])
    chain = torch.cat([gmf_amd.odometry_poses(X[:2]), gmf_amd.odometry_poses(X[2:])])
    assert same_bits(poses.cpu().numpy(), chain.cpu().numpy())
    want_pts, want_off = gmf_amd.tsdf_fragments(dep, chain, K, frame_offsets=off, depth_trunc=3.0, **args)
    assert poff.tolist() == want_off.tolist() and poff[1] == poff[2] and 0 < poff[1] < poff[3]
    assert same_bits(pts.cpu().numpy(), want_pts.cpu().numpy())
    opt = gmf_amd.rgbd_fragments(col, dep, K, frame_offsets=off, **args)
    d = float((opt[2] - chain).abs().max())
    print(f"optimised chain: max|dP| = {d:.3e} (tol {POSE_TOL_POSEGRAPH:.3e})")
    assert d <= POSE_TOL_POSEGRAPH and opt[3].tolist() == [True, True, True]
    # the points lie on the plane and the sphere: test_fragments_host.py's bound plus the drift of the odometry chain, which is
    # the restatement's measured pose error summed along the chain (the rotation acting over the scene's depth, 1.7 m at most)
    drift = {0: 0.0, 3: 0.0}
    for (s, t), first in zip(pairs, (0, 0, 3)):
        rot, tr = R.pose_error(R.fixture_odometry(s, t, None, "B")["T"], R.ground_truth(s, t))
        drift[first] += tr + np.radians(rot) * 1.7
    for g, first in ((0, 0), (2, 3)):
        p = pts[int(poff[g]):int(poff[g + 1])].cpu().numpy().astype(np.float64)
        world = p @ poses_gt[first][:3, :3].T + poses_gt[first][:3, 3]
        dist = np.minimum(np.abs(world[:, 2] - TR.PLANE_Z), np.abs(np.linalg.norm(world - TR.SPHERE_C, axis=1) - TR.SPHERE_R))
        bound = min(2 * 0.010727, TR.VOXEL) + drift[first]
        print(f"fragment {g}: {len(p)} points, largest distance {dist.max():.5f} (bound {bound:.5f})")
        assert len(p) > 1000 and dist.max() <= bound
    # fragments of one frame: no pair, the identity pose, and nothing for the optimiser to do
    off1 = [0, 2, 3, 4, 5]
    for optimize in (False, True):
        out = gmf_amd.rgbd_fragments(col, dep, K, frame_offsets=off1, optimize=optimize, **args)
        assert out[3].tolist() == [True] and out[2].shape == (5, 4, 4)
        eye = torch.eye(4, dtype=torch.float64, device=out[2].device)
        assert all(torch.equal(out[2][f], eye) for f in (0, 2, 3, 4)) and float((out[2][1] - chain[1]).abs().max()) <= POSE_TOL_POSEGRAPH
        alone = gmf_amd.tsdf_fragments(dep[2:3], eye[None], K, depth_trunc=3.0, **args)
        assert same_bits(out[0][int(out[1][1]):int(out[1][2])].cpu().numpy(), alone[0].cpu().numpy()) and alone[0].shape[0] > 1000
    # a failed pair raises and names it
    blank = depth.copy()
    blank[4] = 0
    with pytest.raises(RuntimeError, match=r"rgbd_fragments: the odometry of frames 3 -> 4 \(fragment 2\) failed"):
        gmf_amd.rgbd_fragments(col, _g(blank), K, frame_offsets=off, **args)
