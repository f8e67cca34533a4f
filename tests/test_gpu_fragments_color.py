"""The coloured fragment builder on the device (gmf_amd.tsdf_fragments_colored, rgbd_fragments(colors=True); csrc/tsdf_kernels.hip:
the colour forms of k_tsdf_integrate and k_tsdf_extract) against its numpy restatement (tests/tsdf_color_reference.py), bit for bit:
the colour volume and the vertex colours, beside the geometry of tests/test_gpu_fragments.py, on that file's fixture (81 units,
12991 vertices) with the colour frames of the restatement, and on one- and two-unit ramp volumes given to gmf_tsdf_extract_color
directly."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_color_reference as CR
import tsdf_reference as R

pytestmark = pytest.mark.gpu

GEOMETRY = ("points", "point_offsets", "unit_keys", "unit_offsets", "birth", "tsdf", "weight")
NAMES = GEOMETRY + ("colors", "color_volume")


def _dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _g(x):
    return torch.from_numpy(np.array(x)).to(_dev())          # a copy: the fixtures are read-only


def run(depth, color, poses, frame_offsets=None, **kw):
    """tsdf_fragments_colored(return_volume=True) on numpy inputs -> dict of numpy arrays."""
    import gmf_amd
    args = dict(R.fixture_args())
    args.update(kw)
    out = gmf_amd.tsdf_fragments_colored(_g(color), _g(depth), torch.from_numpy(np.array(poses)), R.INTRINSIC,
                                         frame_offsets=frame_offsets, return_volume=True, **args)
    assert len(out) == len(NAMES)
    return {k: v.cpu().numpy() for k, v in zip(NAMES, out)}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equals_reference(got, ref, where=""):
    U, M = len(ref["unit_keys"]), len(ref["points"])
    assert got["unit_offsets"].tolist() == [0, U] and got["point_offsets"].tolist() == [0, M], where
    for k in ("unit_keys", "birth", "weight", "tsdf", "points"):
        assert same_bits(got[k], ref[k]), f"{where}: {k}"
    differ = (got["color_volume"].view(np.int32) != ref["color_volume"].view(np.int32)).sum()
    assert same_bits(got["color_volume"], ref["color_volume"]), f"{where}: {differ} colour values of the volume differ"
    differ = (got["colors"].view(np.int32) != ref["colors"].view(np.int32)).sum()
    assert same_bits(got["colors"], ref["colors"]), f"{where}: {differ} vertex colour values differ"


@pytest.fixture(scope="module")
def device_result():
    depth, poses = R.fixture()
    return run(depth, CR.color_fixture(), poses)


def test_fixture_bitwise(device_result):
    ref = CR.color_fixture_reference()
    assert device_result["color_volume"].shape == (81, 16, 16, 16, 3) and device_result["colors"].shape == (12991, 3)
    assert_equals_reference(device_result, ref, "fixture")


def test_geometry_has_the_bits_of_the_colour_free_call(device_result):
    import gmf_amd
    depth, poses = R.fixture()
    plain = gmf_amd.tsdf_fragments(_g(depth), torch.from_numpy(np.array(poses)), R.INTRINSIC, return_volume=True, **R.fixture_args())
    assert len(plain) == len(GEOMETRY)
    for k, v in zip(GEOMETRY, plain):
        assert same_bits(device_result[k], v.cpu().numpy()), k
    # and without the volume: points, offsets, colours
    pts, off, col = gmf_amd.tsdf_fragments_colored(_g(CR.color_fixture()), _g(depth), torch.from_numpy(np.array(poses)), R.INTRINSIC,
                                                   **R.fixture_args())
    assert same_bits(pts.cpu().numpy(), device_result["points"]) and same_bits(col.cpu().numpy(), device_result["colors"])
    assert off.tolist() == [0, 12991]


def test_float_depth_in_metres(device_result):
    depth, poses = R.fixture()
    got = run(depth.astype(np.float32) / np.float32(1000.0), CR.color_fixture(), poses)
    assert all(same_bits(got[k], device_result[k]) for k in NAMES)


def test_ragged_batch_equals_fragments_alone(device_result):
    depth, poses = R.fixture()
    color = CR.color_fixture()
    order = [0, 1, 2] + [0, 1, 2, 3, 4]
    got = run(depth[order], color[order], poses[order], frame_offsets=[0, 3, 3, 8])
    first = run(depth[:3], color[:3], poses[:3])
    assert_equals_reference(first, CR.color_fixture_reference(frames=(0, 1, 2)), "three frames")
    uo, po = got["unit_offsets"], got["point_offsets"]
    assert uo.tolist() == [0, len(first["unit_keys"]), len(first["unit_keys"]), len(first["unit_keys"]) + 81]
    assert po.tolist() == [0, len(first["points"]), len(first["points"]), len(first["points"]) + 12991]      # the empty one: nothing
    assert len(got["colors"]) == po[3] and len(got["color_volume"]) == uo[3]
    for g, alone in ((0, first), (2, device_result)):
        for k in ("tsdf", "weight", "color_volume"):
            assert same_bits(got[k][uo[g]:uo[g + 1]], alone[k]), (g, k)
        for k in ("points", "colors"):
            assert same_bits(got[k][po[g]:po[g + 1]], alone[k]), (g, k)


def test_all_zero_depth_and_one_blank_frame():
    depth, poses = R.fixture()
    color = CR.color_fixture()
    nothing = run(np.zeros_like(depth), color, poses, frame_offsets=[0, 2, 5])
    assert nothing["colors"].shape == (0, 3) and nothing["colors"].dtype == np.float32
    assert nothing["color_volume"].shape == (0, 16, 16, 16, 3) and nothing["points"].shape == (0, 3)
    assert nothing["point_offsets"].tolist() == [0, 0, 0]
    blank = np.array(depth)
    blank[2] = 0                                   # its colour frame stays: nothing of it may be read
    got = run(blank, color, poses)
    ref = CR.fragment_color(blank, color, poses, R.INTRINSIC, **R.fixture_args())
    assert_equals_reference(got, ref, "one blank frame")
    assert not np.isin(CR.frame_blue(2), np.unique(ref["color_volume"][..., 2][ref["weight"] == 1]))


def test_two_runs_bitwise_equal(device_result):
    depth, poses = R.fixture()
    again = run(depth, CR.color_fixture(), poses)
    assert all(same_bits(again[k], device_result[k]) for k in NAMES)


def test_c_entries_with_nan_filled_outputs():
    """gmf_tsdf_integrate_color and gmf_tsdf_extract_color called directly: every output is written where the header says, and
    nothing else."""
    from gmf_amd._util import handle_and_stream
    dev = _dev()
    depth, poses = R.fixture()
    ref = CR.color_fixture_reference()
    U, M = 81, 12991
    D, Cf = _g(depth), _g(CR.color_fixture())
    Pinv = torch.from_numpy(np.linalg.inv(poses)).to(dev)
    off = torch.tensor([0, 5], dtype=torch.int32, device=dev)
    h, st = handle_and_stream(D)
    fx, fy, cx, cy = R.INTRINSIC
    camera = (1, 5, R.H, R.W, fx, fy, cx, cy, R.VOXEL, R.TRUNC, 1000.0, 4.5)
    keys, birth = _g(ref["unit_keys"]), _g(ref["birth"])
    uoff = torch.tensor([0, U], dtype=torch.int32, device=dev)
    nan = float("nan")
    tsdf = torch.full((U + 1, 16, 16, 16), nan, device=dev)
    weight = torch.full((U + 1, 16, 16, 16), nan, device=dev)
    cvol = torch.full((U + 1, 16, 16, 16, 3), nan, device=dev)
    h.call("gmf_tsdf_integrate_color", D.data_ptr(), 1, Cf.data_ptr(), Pinv.data_ptr(), off.data_ptr(), *camera, keys.data_ptr(),
           uoff.data_ptr(), birth.data_ptr(), U, tsdf.data_ptr(), weight.data_ptr(), cvol.data_ptr(), st)
    assert same_bits(tsdf[:U].cpu().numpy(), ref["tsdf"]) and same_bits(weight[:U].cpu().numpy(), ref["weight"])
    assert same_bits(cvol[:U].cpu().numpy(), ref["color_volume"])
    assert torch.isnan(tsdf[U]).all() and torch.isnan(weight[U]).all() and torch.isnan(cvol[U]).all()
    volume = (keys.data_ptr(), uoff.data_ptr(), 1, U, tsdf.data_ptr(), weight.data_ptr(), cvol.data_ptr(), R.VOXEL)
    poff = torch.full((2,), -77, dtype=torch.int32, device=dev)
    pts = torch.full((M + 1, 3), nan, device=dev)
    col = torch.full((M + 1, 3), nan, device=dev)
    n = C.c_longlong(-1)
    h.call("gmf_tsdf_extract_color", *volume, None, col.data_ptr(), M, poff.data_ptr(), C.byref(n), st)      # counts only
    assert n.value == M and poff.tolist() == [0, M]
    assert torch.isnan(pts).all() and torch.isnan(col).all()
    poff.fill_(-77)
    n.value = -5
    h.call("gmf_tsdf_extract_color", *volume, pts.data_ptr(), col.data_ptr(), M, poff.data_ptr(), C.byref(n), st)
    assert n.value == -5 and poff.tolist() == [0, M]
    assert same_bits(pts[:M].cpu().numpy(), ref["points"]) and torch.isnan(pts[M]).all()
    assert same_bits(col[:M].cpu().numpy(), ref["colors"]) and torch.isnan(col[M]).all()
    short_p = torch.full((M, 3), nan, device=dev)                                         # short buffers are not overrun
    short_c = torch.full((M, 3), nan, device=dev)
    h.call("gmf_tsdf_extract_color", *volume, short_p.data_ptr(), short_c.data_ptr(), M - 100, poff.data_ptr(), None, st)
    assert same_bits(short_p[:M - 100].cpu().numpy(), ref["points"][:M - 100]) and torch.isnan(short_p[M - 100:]).all()
    assert same_bits(short_c[:M - 100].cpu().numpy(), ref["colors"][:M - 100]) and torch.isnan(short_c[M - 100:]).all()


@pytest.mark.parametrize("axis,units", CR.RAMP_CASES)
def test_ramp_volumes_through_the_c_entry(axis, units):
    """One unit, and two with the crossing edges' far ends in the second: the smallest shape at which fetching the far end's
    colour from the neighbouring unit can go wrong."""
    from gmf_amd._util import handle_and_stream
    dev = _dev()
    v = CR.ramp_volume(axis, units)
    want_p, want_c = CR.extract_color(v["unit_keys"], v["tsdf"], v["weight"], v["color_volume"], R.VOXEL)
    assert same_bits(want_c, v["expected"])
    keys, tsdf, weight, cvol = (_g(v[k]) for k in ("unit_keys", "tsdf", "weight", "color_volume"))
    uoff = torch.tensor([0, units], dtype=torch.int32, device=dev)
    poff = torch.full((2,), -77, dtype=torch.int32, device=dev)
    h, st = handle_and_stream(tsdf)
    volume = (keys.data_ptr(), uoff.data_ptr(), 1, units, tsdf.data_ptr(), weight.data_ptr(), cvol.data_ptr(), R.VOXEL)
    n = C.c_longlong(-1)
    h.call("gmf_tsdf_extract_color", *volume, None, None, 0, poff.data_ptr(), C.byref(n), st)
    assert n.value == 256 and poff.tolist() == [0, 256]
    pts = torch.full((257, 3), float("nan"), device=dev)
    col = torch.full((257, 3), float("nan"), device=dev)
    h.call("gmf_tsdf_extract_color", *volume, pts.data_ptr(), col.data_ptr(), 256, poff.data_ptr(), None, st)
    assert same_bits(pts[:256].cpu().numpy(), want_p) and torch.isnan(pts[256]).all()
    assert same_bits(col[:256].cpu().numpy(), want_c) and torch.isnan(col[256]).all()


def test_rgbd_fragments_with_colors():
    """On the frames of tests/test_gpu_rgbd.py's test_rgbd_fragments, as colour: R = G = the grey value, B half of it."""
    import gmf_amd
    import rgbd_reference as O
    gray, depth, _ = O.fixture()
    rgb = np.stack([gray, gray, gray // 2], -1)
    off = [0, 3, 3, 5]
    args = dict(R.fixture_args())
    col, dep = _g(rgb), _g(depth)
    plain = gmf_amd.rgbd_fragments(col, dep, O.INTRINSIC, frame_offsets=off, optimize=False, colors=False, **args)
    default = gmf_amd.rgbd_fragments(col, dep, O.INTRINSIC, frame_offsets=off, optimize=False, **args)
    got = gmf_amd.rgbd_fragments(col, dep, O.INTRINSIC, frame_offsets=off, optimize=False, colors=True, **args)
    assert len(plain) == len(default) == 4 and len(got) == 5
    pts, poff, colors, poses, ok = got
    for a, b, c in zip((pts, poff, poses, ok), plain, default):
        assert same_bits(a.cpu().numpy(), b.cpu().numpy()) and same_bits(b.cpu().numpy(), c.cpu().numpy())
    assert ok.tolist() == [True, True, True] and poff[1] == poff[2] and 0 < poff[1] < poff[3]
    want = gmf_amd.tsdf_fragments_colored(col, dep, poses, O.INTRINSIC, frame_offsets=off, depth_trunc=3.0, **args)
    assert same_bits(pts.cpu().numpy(), want[0].cpu().numpy()) and same_bits(colors.cpu().numpy(), want[2].cpu().numpy())
    c = colors.cpu().numpy()
    assert c.shape == (pts.shape[0], 3) and c.min() >= 0 and c.max() <= 1 and (c[:, 0] == c[:, 1]).all() and (c[:, 2] <= c[:, 0]).all()
    # with the volume: the colour outputs come after the volume's, the poses last
    full = gmf_amd.rgbd_fragments(col, dep, O.INTRINSIC, frame_offsets=off, optimize=False, colors=True, return_volume=True, **args)
    assert len(full) == 11 and same_bits(full[7].cpu().numpy(), c) and full[8].shape == (full[2].shape[0], 16, 16, 16, 3)
    assert same_bits(full[9].cpu().numpy(), poses.cpu().numpy())
