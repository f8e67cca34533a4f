"""The fragment meshes on the device (gmf_amd.tsdf_fragment_meshes, gmf_amd.tsdf_extract_mesh; csrc/tsdf_kernels.hip:
k_tsdf_mesh_count, k_tsdf_mesh_vertices, k_tsdf_mesh_triangles) against the numpy restatement tests/tsdf_mesh_reference.py, bit
for bit: triangles, both offset vectors and normals, on the two fixtures of tests/tsdf_reference.py and on the random volume
(every case of the table, every neighbour direction, unobserved voxels, tsdf exactly 0, a zero normal sum); the vertices and
colours against tsdf_fragments and tsdf_fragments_colored, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_color_reference as CR
import tsdf_mesh_reference as M
import tsdf_reference as R

pytestmark = pytest.mark.gpu

FIELDS = ("points", "point_offsets", "triangles", "triangle_offsets", "normals", "colors")
VOLUME = ("unit_keys", "unit_offsets", "birth", "tsdf", "weight", "color_volume")


def _dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _g(x):
    return torch.from_numpy(np.array(x)).to(_dev())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def as_numpy(meshes):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in zip(FIELDS, meshes)}


def run(depth, poses, frame_offsets=None, color=None, **kw):
    """tsdf_fragment_meshes(return_volume=True) on numpy inputs -> dict of numpy arrays, the volume included."""
    import gmf_amd
    args = dict(R.fixture_args())
    args.update(kw)
    meshes, volume = gmf_amd.tsdf_fragment_meshes(_g(depth), torch.from_numpy(np.array(poses)), R.INTRINSIC, frame_offsets=frame_offsets,
                                                  color=None if color is None else _g(color), return_volume=True, **args)
    assert type(meshes).__name__ == "TsdfMeshes" and meshes._fields == FIELDS
    out = as_numpy(meshes)
    out.update({k: v.cpu().numpy() for k, v in zip(VOLUME, volume)})
    return out


def extract(keys, off, tsdf, weight, voxel, color_volume=None):
    import gmf_amd
    return as_numpy(gmf_amd.tsdf_extract_mesh(_g(keys), off, _g(tsdf), _g(weight), voxel,
                                              None if color_volume is None else _g(color_volume)))


def assert_mesh_equals(got, ref, where=""):
    """`got` (one fragment) against a dict of the restatement: triangles, normals and points bit for bit."""
    assert got["point_offsets"].dtype == np.int32 and got["triangle_offsets"].dtype == np.int32, where
    assert got["point_offsets"].tolist() == [0, len(ref["points"])], where
    assert got["triangle_offsets"].tolist() == [0, len(ref["triangles"])], where
    assert same_bits(got["points"], ref["points"]), where
    assert same_bits(got["triangles"], ref["triangles"]), f"{where}: {(got['triangles'] != ref['triangles']).any(1).sum()} triangles differ"
    differ = (got["normals"].view(np.int32) != ref["normals"].view(np.int32)).any(1).sum() if got["normals"].shape == ref["normals"].shape else -1
    assert same_bits(got["normals"], ref["normals"]), f"{where}: {differ} normals differ"


@pytest.fixture(scope="module")
def device_result():
    depth, poses = R.fixture()
    return run(depth, poses)


def test_fixture_bitwise(device_result):
    import gmf_amd
    assert device_result["triangles"].shape == (24747, 3) and device_result["normals"].shape == (12991, 3)
    assert device_result["colors"] is None
    assert_mesh_equals(device_result, M.fixture_mesh(), "fixture")
    depth, poses = R.fixture()
    pts, off = gmf_amd.tsdf_fragments(_g(depth), torch.from_numpy(np.array(poses)), R.INTRINSIC, **R.fixture_args())
    assert same_bits(device_result["points"], pts.cpu().numpy()) and device_result["point_offsets"].tolist() == off.tolist()
    # the volume that came back, through tsdf_extract_mesh with its device offsets: the same mesh
    import gmf_amd as G
    again = as_numpy(G.tsdf_extract_mesh(_g(device_result["unit_keys"]), _g(device_result["unit_offsets"]), _g(device_result["tsdf"]),
                                         _g(device_result["weight"]), R.VOXEL))
    assert all(again[k] is None if device_result[k] is None else same_bits(again[k], device_result[k]) for k in FIELDS)


def test_fixture_with_colours_bitwise(device_result):
    import gmf_amd
    depth, poses = R.fixture()
    color = CR.color_fixture()
    got = run(depth, poses, color=color)
    assert all(same_bits(got[k], device_result[k]) for k in FIELDS[:5])            # colour changes nothing else
    out = gmf_amd.tsdf_fragments_colored(_g(color), _g(depth), torch.from_numpy(np.array(poses)), R.INTRINSIC, **R.fixture_args())
    assert same_bits(got["points"], out[0].cpu().numpy()) and same_bits(got["colors"], out[2].cpu().numpy())
    assert got["color_volume"].shape == (81, 16, 16, 16, 3)


def test_cube_rule_volume_bitwise():
    depth, poses = R.pinhole_fixture()
    got = run(depth, poses)
    assert got["triangles"].shape == (6468, 3)
    assert_mesh_equals(got, M.pinhole_mesh(), "pinholes")


def test_random_volume_bitwise():
    keys, off, tsdf, weight = M.random_volume()
    ref = M.random_meshes()
    cvol = (np.random.default_rng(5).random(tsdf.shape + (3,)) * 255).astype(np.float32)
    got = extract(keys, off.tolist(), tsdf, weight, M.RANDOM_VOXEL, cvol)
    assert got["point_offsets"].tolist() == ref["point_offsets"].tolist() == [0, 38271, 82391]
    assert got["triangle_offsets"].tolist() == ref["triangle_offsets"].tolist() == [0, 64023, 139540]
    for k in ("points", "triangles", "normals"):
        differ = (got[k] != ref[k]).any(1).sum() if got[k].shape == ref[k].shape else -1
        assert same_bits(got[k], ref[k]), f"{k}: {differ} rows differ"
    assert (got["normals"] == np.array([0, 0, 1], np.float32)).all(1).sum() >= 1               # the fallback occurs
    for g in range(2):
        a, b = off[g], off[g + 1]
        _, colors = CR.extract_color(keys[a:b], tsdf[a:b], weight[a:b], cvol[a:b], M.RANDOM_VOXEL)
        assert same_bits(got["colors"][got["point_offsets"][g]:got["point_offsets"][g + 1]], colors), g
    # a fragment alone has the bits it has in the batch, local indices included
    a, b = off[1], off[2]
    alone = extract(keys[a:b], [0, b - a], tsdf[a:b], weight[a:b], M.RANDOM_VOXEL)
    po, to = got["point_offsets"], got["triangle_offsets"]
    assert same_bits(alone["points"], got["points"][po[1]:]) and same_bits(alone["normals"], got["normals"][po[1]:])
    assert same_bits(alone["triangles"], got["triangles"][to[1]:]) and alone["colors"] is None


def test_ragged_batch_equals_fragments_alone(device_result):
    depth, poses = R.fixture()
    order = [0, 1, 2] + [0, 1, 2, 3, 4]
    got = run(depth[order], poses[order], frame_offsets=[0, 3, 3, 8])
    first = run(depth[:3], poses[:3])
    assert_mesh_equals(first, M.fixture_mesh(frames=(0, 1, 2)), "three frames")
    po, to = got["point_offsets"], got["triangle_offsets"]
    M0, K0 = len(first["points"]), len(first["triangles"])
    assert po.tolist() == [0, M0, M0, M0 + 12991] and to.tolist() == [0, K0, K0, K0 + 24747]      # the empty one: nothing
    for g, alone in ((0, first), (2, device_result)):
        for k, o in (("points", po), ("normals", po), ("triangles", to)):
            assert same_bits(got[k][o[g]:o[g + 1]], alone[k]), (g, k)                              # (triangles: local indices)


def test_two_runs_bitwise_equal(device_result):
    depth, poses = R.fixture()
    again = run(depth, poses)
    assert all(again[k] is None if device_result[k] is None else same_bits(again[k], device_result[k]) for k in again)


def test_all_zero_frames():
    depth, poses = R.fixture()
    nothing = run(np.zeros_like(depth), poses, frame_offsets=[0, 2, 5])
    assert nothing["points"].shape == (0, 3) and nothing["normals"].shape == (0, 3) and nothing["triangles"].shape == (0, 3)
    assert nothing["triangles"].dtype == np.int32 and nothing["colors"] is None
    assert nothing["point_offsets"].tolist() == [0, 0, 0] and nothing["triangle_offsets"].tolist() == [0, 0, 0]
    assert nothing["unit_keys"].shape == (0, 3)
    coloured = run(np.zeros_like(depth), poses, color=CR.color_fixture())
    assert coloured["colors"].shape == (0, 3) and coloured["triangle_offsets"].tolist() == [0, 0]


def test_c_entry_with_filled_outputs_and_short_caps():
    """gmf_tsdf_extract_mesh called directly on the random volume: counts only touch the offsets and the two counts; with max_points
    and max_triangles one short nothing is written beyond the caps, and the counting call is still right."""
    from gmf_amd._util import handle_and_stream
    dev = _dev()
    keys, off, tsdf, weight = M.random_volume()
    ref = M.random_meshes()
    Mv, K = len(ref["points"]), len(ref["triangles"])
    kd, od, td, wd = _g(keys), _g(off), _g(tsdf), _g(weight)
    h, st = handle_and_stream(td)
    volume = (kd.data_ptr(), od.data_ptr(), 2, len(keys), td.data_ptr(), wd.data_ptr(), None, M.RANDOM_VOXEL)
    poff = torch.full((3,), -77, dtype=torch.int32, device=dev)
    toff = torch.full((3,), -77, dtype=torch.int32, device=dev)
    n, m = C.c_longlong(-1), C.c_longlong(-1)
    h.call("gmf_tsdf_extract_mesh", *volume, None, None, None, 0, None, 0, poff.data_ptr(), toff.data_ptr(), C.byref(n), C.byref(m), st)
    assert (n.value, m.value) == (Mv, K)
    assert poff.tolist() == ref["point_offsets"].tolist() and toff.tolist() == ref["triangle_offsets"].tolist()
    pts = torch.full((Mv + 1, 3), float("nan"), device=dev)
    nrm = torch.full((Mv + 1, 3), float("nan"), device=dev)
    tri = torch.full((K + 1, 3), -1, dtype=torch.int32, device=dev)
    n.value, m.value = -5, -6
    poff.fill_(-77)
    toff.fill_(-77)
    h.call("gmf_tsdf_extract_mesh", *volume, pts.data_ptr(), nrm.data_ptr(), None, Mv - 1, tri.data_ptr(), K - 1, poff.data_ptr(),
           toff.data_ptr(), C.byref(n), C.byref(m), st)
    assert (n.value, m.value) == (-5, -6)                                   # an emitting call reads nothing back
    assert poff.tolist() == ref["point_offsets"].tolist() and toff.tolist() == ref["triangle_offsets"].tolist()
    assert same_bits(pts[:Mv - 1].cpu().numpy(), ref["points"][:Mv - 1]) and torch.isnan(pts[Mv - 1:]).all()
    assert same_bits(nrm[:Mv - 1].cpu().numpy(), ref["normals"][:Mv - 1]) and torch.isnan(nrm[Mv - 1:]).all()
    assert same_bits(tri[:K - 1].cpu().numpy(), ref["triangles"][:K - 1]) and (tri[K - 1:] == -1).all()
    h.call("gmf_tsdf_extract_mesh", *volume, None, None, None, 0, None, 0, poff.data_ptr(), toff.data_ptr(), C.byref(n), C.byref(m), st)
    assert (n.value, m.value) == (Mv, K)


def test_mesh_normals_compose_with_point_to_plane_icp():
    """The fixture's frames {0,1,2} and {2,3,4} as two fragments of one call; the first, moved by the inverse of a known small pose
    (1 degree about (1, 0.5, 0.2), 7 mm), is registered to the second by icp_point_to_plane_batched at the distance
    tests/icp_plane_reference.py uses (0.07), once with the mesh normals as target normals and once with
    estimate_normals_batched's (radius two voxels: a neighbourhood that does not reach across the edge between the sphere and the
    plane).  Both must recover the pose to the gates of tests/test_gpu_icp_plane.py (0.1 degree, 0.01).  The scene - a plane and a
    sphere - is symmetric about the plane's normal through the sphere's centre, so the rotation about that axis is held only by
    the fragments' outlines and carries nearly all of the error.  The float64 restatements of both steps (icp_plane_np on the
    restatement's meshes, fpfh_reference.estimate_normals) give 0.069 degree / 0.0008 with the mesh normals and 0.036 degree /
    0.0008 with the estimated ones; the device gave 0.0681 / 0.00081 and 0.0346 / 0.00083 on an MI355X."""
    import gmf_amd
    import icp_plane_reference as I
    depth, poses = R.fixture()
    order = [0, 1, 2, 2, 3, 4]
    meshes = gmf_amd.tsdf_fragment_meshes(_g(depth[order]), torch.from_numpy(np.array(poses[order])), R.INTRINSIC, frame_offsets=[0, 3, 6],
                                          **R.fixture_args())
    po = meshes.point_offsets.tolist()
    Tg = np.eye(4)
    Tg[:3, :3] = I.rotation((1.0, 0.5, 0.2), 1.0)
    Tg[:3, 3] = (0.004, -0.003, 0.005)
    src = _g(I.transform_rows(np.linalg.inv(Tg), meshes.points[:po[1]].cpu().numpy()).astype(np.float32))
    tgt, tgt_off = meshes.points[po[1]:].contiguous(), [0, po[2] - po[1]]
    estimated = gmf_amd.estimate_normals_batched(tgt, tgt_off, 2 * R.VOXEL, 30)
    eye = torch.eye(4, device=_dev())[None]
    for name, normals in (("mesh", meshes.normals[po[1]:].contiguous()), ("estimated", estimated)):
        T = gmf_amd.icp_point_to_plane_batched(src, tgt, normals, eye, I.TAU, source_offsets=[0, po[1]], target_offsets=tgt_off)[0]
        T = T[0].cpu().numpy().astype(np.float64)
        rot, trans = I.rotation_error_deg(T, Tg), np.linalg.norm(T[:3, 3] - Tg[:3, 3])
        print(f"{name} normals: rotation error {rot:.4f} degree, translation error {trans:.5f}")
        assert rot < 0.1 and trans < 0.01, (name, rot, trans)
