"""CPU-side checks of the coloured fragment builder (gmf_amd/fragments.py: tsdf_fragments_colored; rgbd_fragments(colors=True)): the
restatement tests/tsdf_color_reference.py that tests/test_gpu_fragments_color.py holds the device to - its geometry against
tests/tsdf_reference.py, the colour volume and the vertex colours on the shared fixture, float32 against float64 accumulators, the
ramp volumes against colours worked out by hand - the C ABI entries, and every argument error that is new."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import tsdf_color_reference as CR
import tsdf_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# n = 5 updates at most, three float32 roundings each on values up to 255: see test_blue_channel_is_the_running_mean
ROUNDING_BOUND = 5 * 3 * 2.0 ** -24 * 255


def test_public_name_exported_and_signatures():
    import gmf_amd
    assert hasattr(gmf_amd, "tsdf_fragments_colored") and "tsdf_fragments_colored" in gmf_amd.__all__
    plain = inspect.signature(gmf_amd.tsdf_fragments)
    colored = inspect.signature(gmf_amd.tsdf_fragments_colored)
    assert list(colored.parameters) == ["color"] + list(plain.parameters)
    assert colored.parameters["color"].default is inspect.Parameter.empty
    assert all(colored.parameters[k].default == v.default and colored.parameters[k].kind == v.kind for k, v in plain.parameters.items())
    # the two existing signatures are what they were
    assert list(plain.parameters) == ["depth", "poses", "intrinsic", "frame_offsets", "voxel_length", "sdf_trunc", "depth_scale",
                                      "depth_trunc", "depth_sampling_stride", "max_units", "return_volume"]
    d = {k: v.default for k, v in plain.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(frame_offsets=None, voxel_length=0.008, sdf_trunc=0.04, depth_scale=1000.0, depth_trunc=4.5,
                     depth_sampling_stride=4, max_units=1 << 18, return_volume=False)
    whole = inspect.signature(gmf_amd.rgbd_fragments)
    assert list(whole.parameters) == ["color", "depth", "intrinsic", "frame_offsets", "max_depth_diff", "min_depth", "max_depth",
                                      "optimize", "preference_loop_closure", "tsdf_args"]
    assert whole.parameters["tsdf_args"].kind is inspect.Parameter.VAR_KEYWORD
    d = {k: v.default for k, v in whole.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(frame_offsets=None, max_depth_diff=0.07, min_depth=0.3, max_depth=3.0, optimize=True, preference_loop_closure=0.1)


def test_c_abi_declares_the_colour_entries():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    assert "#define GMF_ABI_VERSION 5" in text
    camera = ["G", "F", "H", "W", "fx", "fy", "cx", "cy", "voxel_length", "sdf_trunc", "depth_scale", "depth_trunc"]
    want = {
        "gmf_tsdf_integrate_color": ["h", "depth", "depth_is_u16", "color", "poses_inv", "frame_offsets"] + camera + [
            "unit_keys", "unit_offsets", "birth", "num_units", "tsdf_out", "weight_out", "color_out", "stream"],
        "gmf_tsdf_extract_color": ["h", "unit_keys", "unit_offsets", "G", "num_units", "tsdf", "weight", "color", "voxel_length",
                                   "points_out", "colors_out", "max_points", "point_offsets_out", "num_points", "stream"],
    }
    source = open(os.path.join(ROOT, "gmf_amd", "csrc", "gmf_api.cpp")).read()
    lib = _lib.load_library()

    def names(params):
        return [p.split()[-1].lstrip("*") for p in params.split(",")]

    for name, params in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*)\)\s*;", text)
        assert m, name
        assert names(m.group(1)) == params
        # the neighbouring entry's parameters, with the two new ones put in
        plain = re.search(r"\bint\s+" + name[:-len("_color")] + r"\s*\(([^;{]*)\)\s*;", text)
        added = {"gmf_tsdf_integrate_color": ("color", "color_out"), "gmf_tsdf_extract_color": ("color", "colors_out")}[name]
        assert [p for p in params if p not in added] == names(plain.group(1))
        d = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*)\)\s*\{", source)
        assert d and " ".join(d.group(1).split()) == " ".join(m.group(1).split())      # the definition repeats the declaration
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(params)
        assert hasattr(lib, name)
    assert lib.gmf_abi_version() == 5


def test_colour_fixture():
    color = CR.color_fixture()
    depth, _ = R.fixture()
    assert color.shape == (5, R.H, R.W, 3) and color.dtype == np.uint8
    nothing = depth == 0
    assert nothing[(slice(None),) + R.HOLE].all() and nothing.sum() == 5 * 16           # the hole: every other ray hits a surface
    assert (color[nothing] == CR.MAGENTA).all()
    assert not (color[~nothing] == CR.MAGENTA).all(-1).any()
    for k in range(5):
        assert (color[k][~nothing[k]][:, 2] == 40 * k + 20).all()


def test_restatement_on_the_fixture():
    """Measured on the restatement: the smallest G of an observed voxel is 37.0 and of a vertex 37.0 (magenta has G = 0), the
    largest B of either is 180 (magenta has 255)."""
    r, ref = CR.color_fixture_reference(), R.fixture_reference()
    assert all(r[k].dtype == ref[k].dtype and r[k].tobytes() == ref[k].tobytes() for k in ref)      # the geometry, bitwise
    cv, col = r["color_volume"], r["colors"]
    assert cv.shape == (81, 16, 16, 16, 3) and cv.dtype == np.float32
    observed = r["weight"] > 0
    assert (cv[~observed] == 0).all()
    assert cv[observed].min() >= 0 and cv[observed].max() <= 255
    assert col.shape == (12991, 3) and col.dtype == np.float32 and col.min() >= 0 and col.max() <= 1
    print(f"smallest G: voxels {cv[observed][:, 1].min()}, vertices {col[:, 1].min() * 255}; largest B: {cv[..., 2].max()}")
    assert cv[observed][:, 1].min() > 36.9 and col[:, 1].min() * 255 > 36.9
    assert cv[..., 2].max() <= 180 and col[:, 2].max() * 255 <= 180 + 1e-4


def test_blue_channel_is_the_running_mean():
    """B is 40 k + 20 over a whole frame, so a voxel's B is the mean of those over the frames that updated it - not the first,
    not the last.  The bound: one update is c' = fl(fl(fl(c w) + x) / (w + 1)), three roundings, each a relative 2^-24 of a value
    that is at most 255 (w + 1) before the division, so the new c' is off by at most 3 * 2^-24 * 255 of its own, to first order;
    the error c carried before comes through times w / (w + 1) < 1.  After n <= 5 updates: at most n * 3 * 2^-24 * 255 = 2.3e-4.
    Measured: 2.5e-6."""
    depth, poses = R.fixture()
    updates = []
    r = CR.fragment_color(depth, CR.color_fixture(), poses, R.INTRINSIC, updates=updates, **R.fixture_args())
    total = np.zeros(r["weight"].size, np.float64)
    count = np.zeros(r["weight"].size, np.float64)
    for k, flat in enumerate(updates):
        total[flat] += CR.frame_blue(k)
        count[flat] += 1
    assert np.array_equal(count.reshape(r["weight"].shape), r["weight"]) and count.max() == 5
    mean = np.where(count > 0, total / np.maximum(count, 1), 0.0)
    blue = r["color_volume"][..., 2].reshape(-1).astype(np.float64)
    err = np.abs(blue - mean).max()
    print(f"largest |B - mean| {err:.3e} (bound {ROUNDING_BOUND:.3e})")
    assert err <= ROUNDING_BOUND
    several = count >= 2
    first = np.full(count.shape, -1.0)
    for k, flat in reversed(list(enumerate(updates))):
        first[flat] = CR.frame_blue(k)
    assert several.sum() > 50000 and (np.abs(blue[several] - first[several]) > 1).all()      # the mean is not the first frame's


def test_float32_against_float64_accumulators():
    """The stated deviation: open3d keeps a voxel's colour as doubles, the contract as float32.  Held to the bound of
    test_blue_channel_is_the_running_mean (over 255 for the vertex colours).  Measured: 6.1e-6 of 255 over the volume, 6.0e-8 of 1
    over the vertex colours (one float32 step of the output)."""
    a, b = CR.color_fixture_reference(), CR.color_fixture_reference(dtype=np.float64)
    assert b["color_volume"].dtype == np.float64 and a["points"].tobytes() == b["points"].tobytes()
    dv = np.abs(a["color_volume"].astype(np.float64) - b["color_volume"]).max()
    dc = np.abs(a["colors"].astype(np.float64) - b["colors"].astype(np.float64)).max()
    print(f"float32 against float64 accumulators: volume {dv:.3e}, vertex colours {dc:.3e}")
    assert 0 < dv <= ROUNDING_BOUND
    assert dc <= ROUNDING_BOUND / 255


def test_red_and_green_against_the_analytic_colour_at_the_vertex():
    """R and G are functions of the world point, so a vertex's colour is near the function at the vertex.  Not exactly: the pixel
    that coloured a voxel hit the surface up to sdf_trunc and a pixel's footprint away from the vertex, and the frames' values are
    rounded to bytes.  Measured on the restatement, in units of 0..255: R largest 18.123 (mean 0.839), G largest 16.717 (mean
    0.896) - the far ones at the sphere's silhouette, where neighbouring pixels see the plane 0.4 behind it.  Bounds: twice the
    measured largest, and the mean below a quarter of that."""
    r = CR.color_fixture_reference()
    want = CR.analytic_rg(r["points"].astype(np.float64))
    for ch, name, largest in ((0, "R", 18.123), (1, "G", 16.717)):
        err = np.abs(r["colors"][:, ch].astype(np.float64) * 255.0 - want[ch])
        print(f"{name}: largest {err.max():.3f}, mean {err.mean():.3f}")
        assert err.max() <= 2 * largest
        assert err.mean() < 2 * largest / 4


@pytest.mark.parametrize("axis,units", CR.RAMP_CASES)
def test_ramp_volumes_by_hand(axis, units):
    v = CR.ramp_volume(axis, units)
    pts, col = CR.extract_color(v["unit_keys"], v["tsdf"], v["weight"], v["color_volume"], R.VOXEL)
    assert pts.shape == (256, 3) and col.dtype == np.float32
    assert (pts[:, axis] == np.float32((v["cross"] + 0.5) * R.VOXEL + (0.25 / 16 * R.VOXEL) / (1.0 / 16))).all()      # a quarter along
    assert col.tobytes() == v["expected"].tobytes()
    # b's colour has the weight ta: the other way round is another colour at every vertex
    _, swapped = CR.extract_color(v["unit_keys"], v["tsdf"], v["weight"], v["color_volume"], R.VOXEL, swapped=True)
    assert (swapped != col).any(1).all()


def test_argument_errors():
    import gmf_amd
    F = 3
    depth = torch.zeros(F, 8, 12, dtype=torch.float32)
    color = torch.zeros(F, 8, 12, 3, dtype=torch.uint8)
    poses = torch.eye(4, dtype=torch.float64).repeat(F, 1, 1)
    K = (10.0, 10.0, 5.5, 3.5)
    cases = [
        (dict(color=color.numpy()), "`color` must be a torch tensor"), (dict(color=None), "`color` must be a torch tensor"),
        (dict(color=color.float()), "uint8"), (dict(color=color.to(torch.int16)), "uint8"),
        (dict(color=color[..., 0]), r"\[F,H,W,3\]"), (dict(color=torch.zeros(F, 8, 12, 4, dtype=torch.uint8)), r"\[F,H,W,3\]"),
        (dict(color=color[:2]), r"\[F,H,W,3\]"), (dict(color=color[:, :7]), r"\[F,H,W,3\]"), (dict(color=color[:, :, :11]), r"\[F,H,W,3\]"),
        (dict(color=torch.zeros(F, 8, 12, 3, dtype=torch.uint8, device="meta")), "depth's device"),
        # the checks it shares with tsdf_fragments are raised under its own name
        (dict(depth=depth.double()), "uint16"), (dict(poses=poses[:2]), r"\[F,4,4\]"), (dict(voxel_length=0.0), "voxel_length"),
        (dict(frame_offsets=[0, 2]), "frame_offsets"), (dict(max_units=0), "max_units"),
        # and a valid call on CPU tensors is refused as well
        (dict(), "no CPU fallback"), (dict(frame_offsets=[0, 0, 2, 3], return_volume=True), "no CPU fallback"),
        (dict(color=color[:0], depth=depth[:0], poses=poses[:0]), "no CPU fallback"),
    ]
    for kw, msg in cases:
        args = dict(color=color, depth=depth, poses=poses, intrinsic=K)
        args.update(kw)
        with pytest.raises(RuntimeError, match=msg) as e:
            gmf_amd.tsdf_fragments_colored(args.pop("color"), args.pop("depth"), args.pop("poses"), args.pop("intrinsic"), **args)
        assert "gmf_amd.tsdf_fragments_colored:" in str(e.value), kw
    # the same check under the other name
    with pytest.raises(RuntimeError, match="voxel_length") as e:
        gmf_amd.tsdf_fragments(depth, poses, K, voxel_length=0.0)
    assert "gmf_amd.tsdf_fragments:" in str(e.value)


def test_rgbd_fragments_colors_argument_errors():
    import gmf_amd
    F = 3
    depth = torch.zeros(F, 8, 12, dtype=torch.float32)
    color = torch.zeros(F, 8, 12, 3, dtype=torch.uint8)
    K = (10.0, 10.0, 5.5, 3.5)
    cases = [
        (color[..., 0], dict(colors=True), "no R, G, B"), (color[..., 0].float(), dict(colors=True), "no R, G, B"),
        (color.numpy(), dict(colors=True), "no R, G, B"),
        (color, dict(colors=1.5), "colors must be True or False"), (color, dict(colors=1), "colors must be True or False"),
        (color, dict(colors="yes"), "colors must be True or False"), (color, dict(colours=True), "unknown argument 'colours'"),
        (color, dict(colors=True), "no CPU fallback"), (color, dict(colors=False), "no CPU fallback"),
        (color[:0], dict(colors=True, depth=depth[:0]), "no CPU fallback"),
    ]
    for col, kw, msg in cases:
        kw = dict(kw)
        with pytest.raises(RuntimeError, match=msg) as e:
            gmf_amd.rgbd_fragments(col, kw.pop("depth", depth), K, **kw)
        assert "gmf_amd.rgbd_fragments:" in str(e.value) and "tsdf_fragments" not in str(e.value).split(":")[0], (kw, msg)
