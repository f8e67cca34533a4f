"""CPU-side checks of the RGB-D odometry (gmf_amd/rgbd.py): the restatement tests/rgbd_reference.py that tests/test_gpu_rgbd.py
holds the device to, on the fixture both share - its figures, the margins that make the pose bound sound, its error against the
analytic ground truth, its failure cases, odd sizes, the tie rule - the C ABI entries, and every argument error.

The figures are those of the committed restatement.  The issue's CPU prototype gave slightly different ones (information[5,5]
2772 / 2801 / 2770 / 2788, errors 0.18 / 0.13 / 0.37 / 0.27 deg); the counts at the first coarse iteration (157 / 157 / 157 /
154) and the largest condition number (779) agree.  The restatement follows the contract, so its figures stand here."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import rgbd_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = R.INTRINSIC
CASES_A = [(0, 1, None), (1, 2, None), (2, 3, None), (3, 4, None), (0, 2, None), (0, 2, (0, 1))]
CASES_B = [(0, 1, None), (2, 3, None), (3, 4, None)]


def test_public_names_exported():
    import gmf_amd
    want = {
        "rgbd_pyramids": (["color", "depth", "depth_scale", "depth_trunc", "min_depth", "max_depth", "levels"],
                          dict(depth_scale=1000.0, depth_trunc=3.0, min_depth=0.0, max_depth=4.0, levels=3)),
        "rgbd_correspondence_map": (["pyr", "pair_source", "pair_target", "transformation", "intrinsic", "level", "max_depth_diff"],
                                    dict(level=0, max_depth_diff=0.03)),
        "rgbd_odometry": (["pyr_or_color", "depth", "pair_source", "pair_target", "intrinsic", "odo_init", "max_depth_diff", "iterations",
                           "return_trace", "pyramid_args"],
                          dict(depth=None, odo_init=None, max_depth_diff=0.03, iterations=(20, 10, 5), return_trace=False)),
        "rgbd_fragments": (["color", "depth", "intrinsic", "frame_offsets", "max_depth_diff", "min_depth", "max_depth", "optimize",
                            "preference_loop_closure", "tsdf_args"],
                           dict(frame_offsets=None, max_depth_diff=0.07, min_depth=0.3, max_depth=3.0, optimize=True,
                                preference_loop_closure=0.1)),
    }
    for name, (params, defaults) in want.items():
        assert hasattr(gmf_amd, name) and name in gmf_amd.__all__
        sig = inspect.signature(getattr(gmf_amd, name))
        assert list(sig.parameters) == params, name
        for k, v in defaults.items():
            assert sig.parameters[k].default == v, (name, k)
    assert "jacobian" not in inspect.signature(gmf_amd.rgbd_odometry).parameters      # the hybrid term only


def test_fixture_figures():
    gray, depth, poses = R.fixture()
    assert gray.shape == depth.shape == (5, 48, 64) and gray.dtype == np.uint8 and depth.dtype == np.uint16 and poses.shape == (5, 4, 4)
    assert (depth > 0).all() and 0 < gray.min() and gray.max() < 255           # every ray hits, the texture is not clipped
    for s, t in ((0, 1), (3, 4)):
        rot, tr = R.pose_error(np.eye(4), R.ground_truth(s, t))
        assert abs(rot - 1.146) < 1e-3 and abs(tr - 0.0136) < 1e-4
    rot, tr = R.pose_error(np.eye(4), R.ground_truth(0, 2))
    assert abs(rot - 2.292) < 1e-3 and abs(tr - 0.0272) < 1e-4
    runs = [R.fixture_odometry(*c) for c in CASES_A]
    assert all(r["success"] and len(r["trace"]) == 35 for r in runs)
    assert [r["trace"][0]["n"] for r in runs] == [157, 157, 157, 154, 116, 145]
    assert [int(r["information"][5, 5]) for r in runs] == [2694, 2795, 2786, 2789, 2595, 2599]
    assert [r["trace"][0]["level"] for r in runs] == [2] * 6 and [it["level"] for it in runs[0]["trace"]] == [2] * 20 + [1] * 10 + [0] * 5
    cond = [max(it["cond"] for it in r["trace"]) for r in runs]
    assert np.allclose(cond, [398.35, 594.09, 545.61, 778.49, 537.76, 529.62], rtol=1e-4)
    assert np.allclose([r["tol"] for r in runs], [1.7047e-9, 2.4642e-9, 2.5832e-9, 3.1441e-9, 2.0583e-9, 1.9299e-9], rtol=1e-4)
    assert [r["ties"] for r in runs] == [1161, 237, 309, 272, 1307, 1370]            # equal-d_s ties met under a solved pose
    assert runs[5]["given"]["ties"] == 48 and runs[0]["given"]["ties"] == 0             # and under the input pose
    for r in runs:
        assert np.allclose(r["information"], r["information"].T) and r["information"][3, 3] == r["information"][5, 5]
        assert 0.9 < r["scales"][0] < 1.0 and 0.9 < r["scales"][1] < 1.0


MEETS_TEN_FOLD = {("A", (2, 3, None)), ("A", (3, 4, None)), ("B", (0, 1, None)), ("B", (3, 4, None))}


def test_margins_carry_the_pose_bound():
    """The pose bound tol is first order in a changed summation order and holds only while no discrete decision flips.  A pose
    within tol of the restatement's moves fu, fv by at most tol (fx + 1) and z by at most 2 tol; the decisions are fu, fv against
    the integers and |z - d_t| against max_depth_diff.  The restatement reports the smallest distance of either over a pair's
    whole run, and the condition is ten times that movement.

    With the committed restatement four of the nine cases meet it (the issue's prototype had 6.3e-6 px and 9.7e-7 m as its smallest
    margins; the restatement is the contract, so its figures stand).  The other five come to, against the ten-fold movement:
    pair 0 -> 1, pixel 9.56e-7 against 1.04e-6; pair 1 -> 2, depth 3.10e-8 against 4.93e-8; pair 0 -> 2, depth 2.86e-8 against
    4.12e-8; pair 0 -> 2 from the ground truth of 0 -> 1, pixel 2.99e-7 against 1.18e-6; pair 2 -> 3 with the second option set,
    depth 7.15e-9 against 6.17e-8 (the three depth figures are decisions under the input pose, between float32 depths).  For those
    tol, a worst case, is replaced by a measurement that is asserted here: the restatement is run again with every sum taken from
    the last correspondence to the first, every count of every iteration must be unchanged, and both margins must exceed ten
    times the movement of the largest pose difference between the two runs over all 35 iterations (4e-16 to 1.4e-15).  The device
    test asserts the same of the device's own difference from the restatement."""
    fx1 = K[0] + 1
    for options, cases in (("A", CASES_A), ("B", CASES_B)):
        for c in cases:
            r = R.fixture_odometry(*c, options)
            tol = r["tol"]
            print(f"{c} {options}: pixel margin {r['pixel_margin']:.3e} (10 x movement {10 * tol * fx1:.3e}), depth margin "
                  f"{r['depth_margin']:.3e} ({10 * tol * 2:.3e}); under a solved pose {r['solved']['pixel_margin']:.3e}, "
                  f"{r['solved']['depth_margin']:.3e}")
            ten_fold = r["pixel_margin"] > 10 * tol * fx1 and r["depth_margin"] > 10 * tol * 2
            assert ten_fold == ((options, c) in MEETS_TEN_FOLD), c
            if ten_fold:
                continue
            other = R.fixture_odometry(*c, options, reverse_sums=True)
            assert other["success"] and [it["n"] for it in other["trace"]] == [it["n"] for it in r["trace"]], c
            assert int(other["information"][5, 5]) == int(r["information"][5, 5])
            moved = max(float(np.abs(x["T"] - y["T"]).max()) for x, y in zip(r["trace"], other["trace"]))
            print(f"    summed in reverse: the pose moves by at most {moved:.3e} (tol {tol:.3e})")
            assert 0 < moved <= tol                              # another order is another result, within the bound
            assert r["pixel_margin"] > 10 * moved * fx1 and r["depth_margin"] > 10 * moved * 2, c
    # the second option set is not used on pair 1 -> 2: 4.5e-7 px under a solved pose there
    r = R.fixture_odometry(1, 2, None, "B")
    assert r["pixel_margin"] < 10 * r["tol"] * fx1


def test_restatement_against_the_analytic_ground_truth():
    """Measured (degrees, millimetres): 0.199 / 7.80, 0.254 / 2.29, 0.352 / 0.86, 0.252 / 2.23 on the four consecutive pairs,
    0.242 / 6.96 on 0 -> 2 from the identity (2.29 deg, 27.2 mm to start with), 0.232 / 6.84 from the ground truth of 0 -> 1.  The
    floor is millimetre depth and 8-bit intensity at 48 x 64.  Held to twice the measured error."""
    measured = [(0.199, 7.80e-3), (0.254, 2.29e-3), (0.352, 0.863e-3), (0.252, 2.23e-3), (0.242, 6.96e-3), (0.232, 6.84e-3)]
    for c, (rot_m, tr_m) in zip(CASES_A, measured):
        rot, tr = R.pose_error(R.fixture_odometry(*c)["T"], R.ground_truth(c[0], c[1]))
        print(f"{c}: {rot:.4f} deg, {1000 * tr:.3f} mm")
        assert rot <= 2 * rot_m and tr <= 2 * tr_m
        assert abs(rot - rot_m) < 1e-3 and abs(tr - tr_m) < 1e-5         # and the figures above are the restatement's


def test_restatement_failures():
    gray, depth, _ = R.fixture()
    pyr = R.fixture_pyramid()
    blank = R.pyramid(gray[:1], np.zeros_like(depth[:1]))
    assert np.isnan(blank[0][0, 1]).all()
    for src, tgt in (([p[0] for p in pyr], [p[0] for p in blank]), ([p[0] for p in blank], [p[0] for p in pyr])):
        r = R.odometry(src, tgt, K)
        assert not r["success"] and len(r["trace"]) == 0 and r["scales"] is None
        assert np.array_equal(r["T"], np.eye(4)) and np.array_equal(r["information"], np.eye(6))
    flat = R.pyramid(np.full((2, 48, 64), 128, np.uint8), np.full((2, 48, 64), 1500, np.uint16))
    r = R.odometry([p[0] for p in flat], [p[1] for p in flat], K)
    assert not r["success"] and len(r["trace"]) == 1 and r["trace"][0]["n"] == 12 * 16      # the determinant, at the first iteration
    assert abs(np.linalg.det(r["trace"][0]["A"])) < 1e-6 and np.array_equal(r["T"], np.eye(4))


def test_odd_sizes_and_clamped_borders():
    pyr = R.fixture_pyramid(crop=True)
    assert [p.shape for p in pyr] == [(5, 6, 47, 61), (5, 6, 23, 30), (5, 6, 11, 15)]
    full = R.fixture_pyramid()
    # away from the cut edges the crop's level 0 is the full frame's; at them the clamped taps differ
    assert np.array_equal(pyr[0][:, :2, :46, :60], full[0][:, :2, :46, :60]) and not np.array_equal(pyr[0][:, 0, 46], full[0][:, 0, 46, :61])
    assert np.array_equal(pyr[0][:, 2:, :45, :59], full[0][:, 2:, :45, :59]) and not np.array_equal(pyr[0][:, 2, :, 59], full[0][:, 2, :47, 59])
    # a constant image stays constant under the Gaussian up to its border and has no gradient there
    c = np.full((1, 7, 9), 0.3, np.float32)
    assert np.array_equal(R.filter3(c, R.GAUSS, R.GAUSS), c)
    assert not R.filter3(c, R.SOBEL_D, R.SOBEL_S).any() and not R.filter3(c, R.SOBEL_S, R.SOBEL_D).any()
    ramp = np.tile(np.arange(9, dtype=np.float32), (1, 7, 1))
    gx = R.filter3(ramp, R.SOBEL_D, R.SOBEL_S)
    assert (gx[0, :, 1:-1] == 8).all() and (gx[0, :, 0] == 4).all() and (gx[0, :, -1] == 4).all()      # clamped: half a step
    assert R.down(np.arange(35, dtype=np.float32).reshape(1, 5, 7)).shape == (1, 2, 3)
    nan = c.copy()
    nan[0, 3, 4] = np.nan
    assert np.isnan(R.filter3(nan, R.SOBEL_D, R.SOBEL_S)[0, 2:5, 3:6]).all()                 # 0 * NaN spreads too
    for (s, t), (rot_m, tr_m, n0, count) in {(0, 1): (0.0886, 7.58e-3, 130, 2504), (2, 3): (0.3587, 2.32e-3, 130, 2577)}.items():
        r = R.odometry([p[s] for p in pyr], [p[t] for p in pyr], K)
        rot, tr = R.pose_error(r["T"], R.ground_truth(s, t))
        assert r["success"] and r["trace"][0]["n"] == n0 and int(r["information"][5, 5]) == count
        assert abs(rot - rot_m) < 1e-3 and abs(tr - tr_m) < 1e-5


def test_tie_rule_and_column_zero():
    ref = R.fixture_pyramid()
    Ds, Dt = ref[0][0, 1], ref[0][1, 1]
    gt = R.ground_truth(0, 1)
    a, b = R.correspondence_map(K, gt, Ds, Dt), R.correspondence_map(K, gt, Ds, Dt, tie_largest=True)
    assert int((a != b).sum()) == 48 and ((a >= 0) == (b >= 0)).all() and (a <= b).all()
    # the winner has the smallest depth among the candidates of its pixel
    stats = {}
    R.correspondence_map(K, gt, Ds, Dt, stats=stats)
    assert stats["ties"] == 48
    # under the push pose pixels leave the image and, at every level, some land on column 0 from fu in (-1, 0)
    for l, (inside, left) in enumerate([(48, 96), (24, 24), (12, 0)]):
        Kl = R.level_intrinsic(K, l)
        fu, fv = R.projections(Kl, R.PUSH_POSE, ref[l][0, 1])
        assert int(((fu > -1) & (fu < 0)).sum()) == inside and int((fu <= -1).sum()) == left
        cmap = R.correspondence_map(Kl, R.PUSH_POSE, ref[l][0, 1], ref[l][1, 1])
        w = R.W >> l
        sources_of_column_0 = cmap[:, 0][cmap[:, 0] >= 0]
        assert len(sources_of_column_0) > 5 and (sources_of_column_0 % w <= 3).all()
    assert R.level_intrinsic(K, 2) == (15.0, 15.0, 7.875, 5.875)


def test_c_abi_declares_the_entries():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    assert "#define GMF_ABI_VERSION 5" in text
    camera = ["fx", "fy", "cx", "cy", "max_depth_diff"]
    want = {
        "gmf_rgbd_pyramids": ["h", "color", "color_kind", "depth", "depth_is_u16", "F", "H", "W", "depth_scale", "depth_trunc", "min_depth",
                              "max_depth", "levels", "planes_out", "stream"],
        "gmf_rgbd_correspondences": ["h", "planes", "F", "H", "W", "levels", "level", "pair_source", "pair_target", "E", "transformation"]
        + camera + ["map_out", "stream"],
        "gmf_rgbd_odometry": ["h", "planes", "F", "H", "W", "levels", "pair_source", "pair_target", "E", "odo_init"] + camera + [
            "iterations", "success_out", "transformation_out", "information_out", "scales_out", "trace_n_out", "trace_out", "stream"],
    }
    source = open(os.path.join(ROOT, "gmf_amd", "csrc", "gmf_api.cpp")).read()
    lib = _lib.load_library()
    for name, params in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*)\)\s*;", text)
        assert m, name
        assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == params
        d = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*)\)\s*\{", source)
        assert d and " ".join(d.group(1).split()) == " ".join(m.group(1).split())      # the definition repeats the declaration
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(params)
        assert hasattr(lib, name)
    assert lib.gmf_abi_version() == 5


def _raises(fn, msg, name):
    with pytest.raises(RuntimeError, match=msg) as e:
        fn()
    assert f"gmf_amd.{name}:" in str(e.value), (msg, str(e.value))


def test_pyramid_argument_errors():
    import gmf_amd
    F, H, W = 3, 8, 12
    color = torch.zeros(F, H, W, dtype=torch.uint8)
    depth = torch.zeros(F, H, W, dtype=torch.uint16)
    cases = [
        (dict(color=color.numpy()), "torch tensor"), (dict(depth=depth.numpy()), "torch tensor"),
        (dict(depth=depth.to(torch.int32)), "uint16"), (dict(depth=depth.double()), "uint16"),
        (dict(depth=depth[0]), r"\[F,H,W\]"), (dict(depth=depth[:0], color=color[:0]), r"\[F,H,W\]"),
        (dict(color=color[:2]), "`color` must be"), (dict(color=color.double()), "`color` must be"),
        (dict(color=torch.zeros(F, H, W, 4, dtype=torch.uint8)), "`color` must be"),
        (dict(color=torch.zeros(F, H, W, 3)), "`color` must be"), (dict(color=color[:, :, :11]), "`color` must be"),
        (dict(depth_scale=0.0), "depth_scale"), (dict(depth_scale=float("inf")), "depth_scale"), (dict(depth_scale="x"), "depth_scale"),
        (dict(depth_trunc=0.0), "depth_trunc"), (dict(depth_trunc=float("nan")), "depth_trunc"),
        (dict(min_depth=-0.1), "min_depth"), (dict(min_depth=float("nan")), "min_depth"), (dict(min_depth="x"), "min_depth"),
        (dict(min_depth=1.0, max_depth=1.0), "max_depth"), (dict(max_depth=float("nan")), "max_depth"),
        (dict(levels=0), "levels"), (dict(levels=9), "levels"), (dict(levels=2.0), "levels"), (dict(levels=5), "levels"),
        # and a valid call on CPU tensors is refused, in every input form
        (dict(), "no CPU fallback"), (dict(color=torch.zeros(F, H, W, 3, dtype=torch.uint8)), "no CPU fallback"),
        (dict(color=color.float(), depth=depth.float()), "no CPU fallback"), (dict(levels=4, max_depth=float("inf")), "no CPU fallback"),
    ]
    for kw, msg in cases:
        args = dict(color=color, depth=depth)
        args.update(kw)
        _raises(lambda: gmf_amd.rgbd_pyramids(args.pop("color"), args.pop("depth"), **args), msg, "rgbd_pyramids")


def test_odometry_and_map_argument_errors():
    import gmf_amd
    F, H, W, L = 3, 8, 12, 3
    n = sum(F * 6 * (H >> l) * (W >> l) for l in range(L))
    pyr = gmf_amd.RGBDPyramids(torch.zeros(n), F, H, W, L)                   # on the host: good for every check but the last
    assert pyr.planes(2).shape == (F, 6, 2, 3)
    _raises(lambda: pyr.planes(3), "level", "rgbd_pyramids")
    Kc = (10.0, 10.0, 5.5, 3.5)
    eye = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    shared = [
        (dict(pair_source=[0]), "same length"), (dict(pair_source=[0, 3]), "pair 1 names a frame"), (dict(pair_target=[-1, 1]), "pair 0 names"),
        (dict(pair_source=[0, 1.5]), "pair_source"), (dict(pair_target="ab"), "pair_target"), (dict(pair_source=7), "pair_source"),
        (dict(intrinsic=(10.0, 10.0, 5.5)), "intrinsic"), (dict(intrinsic=(0.0, 10.0, 5, 3)), "intrinsic"),
        (dict(intrinsic=(10.0, 10.0, float("nan"), 3)), "intrinsic"), (dict(intrinsic=None), "intrinsic"),
        (dict(max_depth_diff=-0.01), "max_depth_diff"), (dict(max_depth_diff=float("inf")), "max_depth_diff"), (dict(max_depth_diff="x"), "max_depth_diff"),
    ]
    for kw, msg in shared + [
        (dict(pyr=None), "rgbd_pyramids returned"), (dict(level=3), "level"), (dict(level=-1), "level"), (dict(level=1.0), "level"),
        (dict(transformation=eye.float()), "float64"), (dict(transformation=eye[:1]), r"\[2, 4, 4\]"), (dict(transformation=eye.numpy()), "float64"),
        (dict(), "no CPU fallback"),
    ]:
        args = dict(pyr=pyr, pair_source=[0, 1], pair_target=[1, 2], transformation=eye, intrinsic=Kc)
        args.update(kw)
        _raises(lambda: gmf_amd.rgbd_correspondence_map(**args), msg, "rgbd_correspondence_map")
    color, depth = torch.zeros(F, H, W, dtype=torch.uint8), torch.zeros(F, H, W, dtype=torch.uint16)
    for kw, msg in shared + [
        (dict(iterations=(20, 10)), "one entry per level"), (dict(iterations=(20, 10, -1)), "iterations"), (dict(iterations=(1.5, 1, 1)), "iterations"),
        (dict(iterations=5), "iterations"), (dict(iterations=()), "iterations"),
        (dict(odo_init=eye.float()), "float64"), (dict(odo_init=eye[:1]), r"\[2, 4, 4\]"), (dict(odo_init=eye), "no CPU fallback"),
        (dict(depth=depth), "not taken"), (dict(levels=3), "not taken"),
        (dict(pyr_or_color=color), "colour frames and `depth`"), (dict(pyr_or_color=color, depth=depth, jacobian="color"), "unknown argument 'jacobian'"),
        (dict(pyr_or_color=color, depth=depth.to(torch.int32)), "uint16"), (dict(pyr_or_color=color, depth=depth, levels=9), "levels"),
        (dict(pyr_or_color=color, depth=depth, min_depth=-1.0), "min_depth"),
        (dict(pyr_or_color=color, depth=depth), "no CPU fallback"), (dict(pyr_or_color=color, depth=depth, iterations=(3, 3)), "no CPU fallback"),
        (dict(), "no CPU fallback"), (dict(return_trace=True, pair_source=[], pair_target=[]), "no CPU fallback"),
    ]:
        args = dict(pyr_or_color=pyr, pair_source=[0, 1], pair_target=[1, 2], intrinsic=Kc)
        args.update(kw)
        _raises(lambda: gmf_amd.rgbd_odometry(args.pop("pyr_or_color"), **args), msg, "rgbd_odometry")


def test_fragments_argument_errors():
    import gmf_amd
    F, H, W = 3, 8, 12
    color, depth = torch.zeros(F, H, W, dtype=torch.uint8), torch.zeros(F, H, W, dtype=torch.uint16)
    Kc = (10.0, 10.0, 5.5, 3.5)
    cases = [
        (dict(depth=depth.numpy()), "`depth`"), (dict(depth=depth[0]), "`depth`"),
        (dict(frame_offsets=[0]), "frame_offsets"), (dict(frame_offsets=[1, 3]), "frame_offsets"), (dict(frame_offsets=[0, 2, 1, 3]), "frame_offsets"),
        (dict(frame_offsets=[0, 1.5, 3]), "frame_offsets"), (dict(frame_offsets=7), "frame_offsets"),
        (dict(preference_loop_closure=0.0), "preference_loop_closure"), (dict(preference_loop_closure="x"), "preference_loop_closure"),
        (dict(intrinsic=(10.0, 10.0)), "intrinsic"), (dict(intrinsic=(10.0, -10.0, 1, 1)), "intrinsic"),
        (dict(voxel_size=0.01), "unknown argument 'voxel_size'"),
        (dict(max_depth_diff=-1.0), "max_depth_diff"), (dict(min_depth=-1.0), "min_depth"), (dict(max_depth=0.2), "max_depth"),
        (dict(color=color[:2]), "`color` must be"), (dict(depth_scale=0.0), "depth_scale"),
        (dict(), "no CPU fallback"), (dict(frame_offsets=[0, 2, 2, 3], optimize=False, voxel_length=0.02), "no CPU fallback"),
        (dict(color=color[:0], depth=depth[:0]), "no CPU fallback"),
    ]
    for kw, msg in cases:
        args = dict(color=color, depth=depth, intrinsic=Kc)
        args.update(kw)
        _raises(lambda: gmf_amd.rgbd_fragments(args.pop("color"), args.pop("depth"), args.pop("intrinsic"), **args), msg, "rgbd_fragments")
