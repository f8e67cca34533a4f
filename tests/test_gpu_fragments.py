"""The fragment builder on the device (gmf_amd.tsdf_fragments; csrc/tsdf_kernels.hip) against its numpy restatement
(tests/tsdf_reference.py), bit for bit: units, births, the volume, the vertices and their order, on the fixture of
tests/test_fragments_host.py (a plane, a sphere, five poses, a hole; 81 units, 12991 vertices) and on the one-frame volume where the
cube rule removes 790 crossings."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_reference as R

pytestmark = pytest.mark.gpu

VOLUME = ("unit_keys", "unit_offsets", "birth", "tsdf", "weight")


def _dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def run(depth, poses, frame_offsets=None, **kw):
    """tsdf_fragments(return_volume=True) on numpy inputs -> dict of numpy arrays."""
    import gmf_amd
    args = dict(R.fixture_args())
    args.update(kw)
    out = gmf_amd.tsdf_fragments(torch.from_numpy(np.array(depth)).to(_dev()), torch.from_numpy(np.array(poses)), R.INTRINSIC,
                                 frame_offsets=frame_offsets, return_volume=True, **args)
    return {k: v.cpu().numpy() for k, v in zip(("points", "point_offsets") + VOLUME, out)}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equals_reference(got, ref, where=""):
    U, M = len(ref["unit_keys"]), len(ref["points"])
    assert got["unit_offsets"].tolist() == [0, U], where
    assert got["point_offsets"].tolist() == [0, M], where
    assert np.array_equal(got["unit_keys"], ref["unit_keys"]) and got["unit_keys"].dtype == np.int32, where
    assert np.array_equal(got["birth"], ref["birth"]) and got["birth"].dtype == np.int32, where
    assert same_bits(got["weight"], ref["weight"]), f"{where}: {(got['weight'] != ref['weight']).sum()} weights differ"
    assert same_bits(got["tsdf"], ref["tsdf"]), f"{where}: {(got['tsdf'].view(np.int32) != ref['tsdf'].view(np.int32)).sum()} tsdf differ"
    assert same_bits(got["points"], ref["points"]), where          # the same vertices, in the same order


@pytest.fixture(scope="module")
def device_result():
    depth, poses = R.fixture()
    return run(depth, poses)


def test_units_births_and_volume_bitwise(device_result):
    ref = R.fixture_reference()
    assert device_result["unit_keys"].shape == (81, 3) and device_result["tsdf"].shape == (81, 16, 16, 16)
    assert np.bincount(device_result["birth"], minlength=5).tolist() == [34, 18, 10, 7, 12]
    assert_equals_reference(device_result, ref, "fixture")
    # the other rule (every frame into every unit) is another volume: the comparison above tells them apart
    assert not same_bits(device_result["weight"], R.fixture_reference(from_birth=False)["weight"])


def test_points_bitwise_and_in_order(device_result):
    ref = R.fixture_reference()
    assert device_result["points"].shape == (12991, 3)
    assert same_bits(device_result["points"], ref["points"])
    assert not same_bits(device_result["points"], R.fixture_reference(cube_rule=False)["points"])


def test_cube_rule_volume_bitwise():
    depth, poses = R.pinhole_fixture()
    got = run(depth, poses)
    assert len(got["points"]) == 3906                              # 4696 crossings, 790 of them in no fully observed cube
    assert_equals_reference(got, R.pinhole_reference(), "pinholes")


def test_float_depth_in_metres(device_result):
    depth, poses = R.fixture()
    metres = depth.astype(np.float32) / np.float32(1000.0)
    metres[2, 0, 0], metres[2, 0, 4], metres[2, 4, 0] = np.nan, -1.0, np.inf      # sampled pixels: no measurement
    ref = R.fragment(metres, poses, R.INTRINSIC, **R.fixture_args())
    got = run(metres, poses)
    assert_equals_reference(got, ref, "float32 depth")
    clean = run(depth.astype(np.float32) / np.float32(1000.0), poses)
    assert all(same_bits(clean[k], device_result[k]) for k in clean)


def test_ragged_batch_equals_fragments_alone(device_result):
    depth, poses = R.fixture()
    order = [0, 1, 2] + [0, 1, 2, 3, 4]
    got = run(depth[order], poses[order], frame_offsets=[0, 3, 3, 8])
    first = run(depth[:3], poses[:3])
    assert_equals_reference(first, R.fixture_reference(frames=(0, 1, 2)), "three frames")
    uo, po = got["unit_offsets"], got["point_offsets"]
    assert uo.tolist() == [0, len(first["unit_keys"]), len(first["unit_keys"]), len(first["unit_keys"]) + 81]
    assert po.tolist() == [0, len(first["points"]), len(first["points"]), len(first["points"]) + 12991]      # the empty one: no points
    for g, alone in ((0, first), (2, device_result)):
        for k in ("unit_keys", "birth", "tsdf", "weight"):
            assert same_bits(got[k][uo[g]:uo[g + 1]], alone[k]), (g, k)
        assert same_bits(got["points"][po[g]:po[g + 1]], alone["points"]), g


def test_depth_trunc_cuts_the_plane_away():
    depth, poses = R.fixture()
    got = run(depth, poses, depth_trunc=1.4)
    assert_equals_reference(got, R.fixture_reference(depth_trunc=1.4), "depth_trunc")
    assert 0 < len(got["points"]) < 4000 and (got["points"][:, 2] < 1.45).all()


def test_all_zero_frames(device_result):
    depth, poses = R.fixture()
    blank = np.array(depth)
    blank[1] = 0
    got = run(blank, poses)
    assert_equals_reference(got, R.fragment(blank, poses, R.INTRINSIC, **R.fixture_args()), "one blank frame")
    nothing = run(np.zeros_like(blank), poses, frame_offsets=[0, 2, 5])
    assert nothing["points"].shape == (0, 3) and nothing["point_offsets"].tolist() == [0, 0, 0]
    assert nothing["unit_keys"].shape == (0, 3) and nothing["unit_offsets"].tolist() == [0, 0, 0]
    assert nothing["tsdf"].shape == (0, 16, 16, 16)


def test_max_units_overflow_and_index_range_raise():
    depth, poses = R.fixture()
    with pytest.raises(RuntimeError, match="raise max_units"):
        run(depth, poses, max_units=80)
    assert len(run(depth, poses, max_units=81)["unit_keys"]) == 81
    with pytest.raises(RuntimeError, match="raise voxel_length"):
        run(depth, poses, voxel_length=1e-7, sdf_trunc=1e-7)


def test_two_runs_bitwise_equal(device_result):
    depth, poses = R.fixture()
    again = run(depth, poses)
    assert all(same_bits(again[k], device_result[k]) for k in again)


def test_c_entries_with_nan_filled_outputs(device_result):
    """gmf_tsdf_allocate, gmf_tsdf_integrate and gmf_tsdf_extract called directly: every output is written where the header says,
    and nothing else."""
    from gmf_amd._util import handle_and_stream
    dev = _dev()
    depth, poses = R.fixture()
    ref = R.fixture_reference()
    U, M, cap = 81, 12991, 100
    D = torch.from_numpy(np.array(depth)).to(dev)
    P = torch.from_numpy(np.stack([poses, np.linalg.inv(poses)])).to(dev)
    off = torch.tensor([0, 5], dtype=torch.int32, device=dev)
    h, st = handle_and_stream(D)
    fx, fy, cx, cy = R.INTRINSIC
    camera = (1, 5, R.H, R.W, fx, fy, cx, cy, R.VOXEL, R.TRUNC, 1000.0, 4.5)
    keys = torch.full((cap, 3), -77, dtype=torch.int32, device=dev)
    birth = torch.full((cap,), -77, dtype=torch.int32, device=dev)
    uoff = torch.full((2,), -77, dtype=torch.int32, device=dev)
    n = C.c_longlong(-1)
    h.call("gmf_tsdf_allocate", D.data_ptr(), 1, P[0].data_ptr(), off.data_ptr(), *camera, R.STRIDE, cap, keys.data_ptr(), birth.data_ptr(),
           uoff.data_ptr(), C.byref(n), st)
    assert n.value == U and uoff.tolist() == [0, U]
    assert np.array_equal(keys[:U].cpu().numpy(), ref["unit_keys"]) and (keys[U:] == -77).all()
    assert np.array_equal(birth[:U].cpu().numpy(), ref["birth"]) and (birth[U:] == -77).all()
    tsdf = torch.full((U + 1, 16, 16, 16), float("nan"), device=dev)
    weight = torch.full((U + 1, 16, 16, 16), float("nan"), device=dev)
    h.call("gmf_tsdf_integrate", D.data_ptr(), 1, P[1].data_ptr(), off.data_ptr(), *camera, keys.data_ptr(), uoff.data_ptr(),
           birth.data_ptr(), U, tsdf.data_ptr(), weight.data_ptr(), st)
    assert same_bits(tsdf[:U].cpu().numpy(), ref["tsdf"]) and same_bits(weight[:U].cpu().numpy(), ref["weight"])
    assert torch.isnan(tsdf[U]).all() and torch.isnan(weight[U]).all()
    volume = (keys.data_ptr(), uoff.data_ptr(), 1, U, tsdf.data_ptr(), weight.data_ptr(), R.VOXEL)
    poff = torch.full((2,), -77, dtype=torch.int32, device=dev)
    h.call("gmf_tsdf_extract", *volume, None, 0, poff.data_ptr(), C.byref(n), st)       # counts only
    assert n.value == M and poff.tolist() == [0, M]
    pts = torch.full((M + 1, 3), float("nan"), device=dev)
    poff.fill_(-77)
    n.value = -5
    h.call("gmf_tsdf_extract", *volume, pts.data_ptr(), M, poff.data_ptr(), C.byref(n), st)
    assert n.value == -5 and poff.tolist() == [0, M]
    assert same_bits(pts[:M].cpu().numpy(), ref["points"]) and torch.isnan(pts[M]).all()
    short = torch.full((M, 3), float("nan"), device=dev)                                  # a short buffer is not overrun
    h.call("gmf_tsdf_extract", *volume, short.data_ptr(), M - 100, poff.data_ptr(), None, st)
    assert same_bits(short[:M - 100].cpu().numpy(), ref["points"][:M - 100]) and torch.isnan(short[M - 100:]).all()


def test_points_compose_with_the_descriptor_front_end(device_result):
    import gmf_amd
    dev = _dev()
    pts = torch.from_numpy(device_result["points"]).to(dev)
    off = torch.from_numpy(device_result["point_offsets"]).to(dev)
    down, down_off = gmf_amd.voxel_down_sample_batched(pts, off, 0.05)            # the device offsets, as they come
    assert 0 < down.shape[0] < pts.shape[0] and down.shape[1] == 3
    normals = gmf_amd.estimate_normals_batched(down, down_off, 0.1, 30)
    torch.cuda.synchronize()
    assert normals.shape == down.shape and torch.isfinite(normals).all()
