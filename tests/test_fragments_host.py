"""CPU-side checks of the fragment builder (gmf_amd/fragments.py: tsdf_fragments): the restatement tests/tsdf_reference.py that
tests/test_gpu_fragments.py holds the device to, on the fixture both share - its figures, and that the fixture exercises late
births, negative unit indices, the hole and (a second volume) the cube rule - the extracted points against the analytic surfaces,
the C ABI entries, and every argument error."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import tsdf_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_name_exported():
    import gmf_amd
    assert hasattr(gmf_amd, "tsdf_fragments") and "tsdf_fragments" in gmf_amd.__all__
    sig = inspect.signature(gmf_amd.tsdf_fragments)
    assert list(sig.parameters) == ["depth", "poses", "intrinsic", "frame_offsets", "voxel_length", "sdf_trunc", "depth_scale",
                                    "depth_trunc", "depth_sampling_stride", "max_units", "return_volume"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(frame_offsets=None, voxel_length=0.008, sdf_trunc=0.04, depth_scale=1000.0, depth_trunc=4.5,
                     depth_sampling_stride=4, max_units=1 << 18, return_volume=False)


def test_fixture_figures():
    """The figures of the issue's CPU prototype, re-established with the committed restatement (they agree exactly)."""
    depth, poses = R.fixture()
    assert depth.shape == (5, R.H, R.W) and depth.dtype == np.uint16 and poses.shape == (5, 4, 4)
    r = R.fixture_reference()
    keys, birth = r["unit_keys"], r["birth"]
    assert len(keys) == 81
    assert int((keys < 0).any(1).sum()) == 54
    assert np.bincount(birth, minlength=5).tolist() == [34, 18, 10, 7, 12]
    assert [tuple(k) for k in keys] == sorted(tuple(k) for k in keys)              # ascending (x, y, z)
    assert int((r["weight"] > 0).sum()) == 185503
    assert len(r["points"]) == 12991
    assert len(np.unique(r["points"], axis=0)) == 12991                            # each vertex once
    assert r["tsdf"].dtype == r["weight"].dtype == r["points"].dtype == np.float32


def test_fixture_exercises_late_births_negative_indices_and_the_hole():
    r = R.fixture_reference()
    # late births: integrating every frame into every unit changes weights, so the birth rule is visible in this scene
    every = R.fixture_reference(from_birth=False)
    changed = int((every["weight"] != r["weight"]).sum())
    assert changed == 13354
    assert (r["birth"] > 0).sum() == 47 and (every["weight"] >= r["weight"]).all()
    # negative unit indices along x and y, with units on both sides of zero (the scene lies in front of z = 0)
    assert (r["unit_keys"].min(0)[:2] < 0).all() and (r["unit_keys"].max(0) > 0).all()
    # the hole: its pixels are zero in every frame, carry a measurement without it, and filling it changes the volume
    depth, poses = R.fixture()
    assert (depth[(slice(None),) + R.HOLE] == 0).all()
    filled = np.stack([np.round(R.raycast(P) * 1000.0) for P in poses]).astype(np.uint16)
    assert (filled[(slice(None),) + R.HOLE] > 0).all()
    assert ((filled == 0) == (np.array(depth) == 0)).sum() == depth.size - 5 * 16      # the hole is the only difference
    whole = R.fragment(filled, poses, R.INTRINSIC, **R.fixture_args())
    assert int((whole["weight"] > 0).sum()) == 185568 and len(whole["points"]) == 13001
    # the cube rule removes one crossing here; test_cube_rule_volume has a volume where it removes many
    assert len(R.fixture_reference(cube_rule=False)["points"]) == 12992


def test_cube_rule_volume():
    """One frame of the plane with isolated zero pixels: 4696 crossings between observed voxels, of which 790 lie in no fully
    observed cube."""
    depth, _ = R.pinhole_fixture()
    assert int((depth == 0).sum()) == 15 * 24
    r, loose = R.pinhole_reference(), R.pinhole_reference(cube_rule=False)
    assert len(r["unit_keys"]) == 30
    assert len(loose["points"]) == 4696
    assert len(r["points"]) == 3906
    kept = {p.tobytes() for p in r["points"]}
    assert len(kept) == 3906 and kept < {p.tobytes() for p in loose["points"]}     # the rule only removes


def test_points_lie_on_the_analytic_surfaces():
    """Distance of every extracted vertex to the nearer of the plane z = 1.5 and the sphere.  Measured on the restatement: largest
    0.010727 (the 99th percentile is 0.0073, the mean 0.0013): the far ones sit where the sphere's silhouette meets the plane
    behind it and the projective distance of one surface is averaged with the other's.  The bound is twice the measured value,
    and in any case no more than voxel_length: 0.02."""
    p = R.fixture_reference()["points"].astype(np.float64)
    dist = np.minimum(np.abs(p[:, 2] - R.PLANE_Z), np.abs(np.linalg.norm(p - R.SPHERE_C, axis=1) - R.SPHERE_R))
    print(f"largest distance {dist.max():.6f}, mean {dist.mean():.6f}")
    assert dist.max() <= min(2 * 0.010727, R.VOXEL)
    # both surfaces are there
    assert (np.abs(p[:, 2] - R.PLANE_Z) < 0.005).sum() > 5000
    assert (np.abs(np.linalg.norm(p - R.SPHERE_C, axis=1) - R.SPHERE_R) < 0.005).sum() > 1000
    # the flat volume of test_cube_rule_volume is the plane alone
    q = R.pinhole_reference()["points"].astype(np.float64)
    assert np.abs(q[:, 2] - R.PLANE_Z).max() < 1e-3


def test_float_depth_and_truncation_in_the_restatement():
    depth, poses = R.fixture()
    metres = depth.astype(np.float32) / np.float32(1000.0)
    a = R.fragment(metres, poses, R.INTRINSIC, **R.fixture_args())
    r = R.fixture_reference()
    assert all(np.array_equal(a[k], r[k]) for k in r)
    bad = metres.copy()
    bad[0, 0, :4] = [np.nan, np.inf, -1.0, -np.inf]
    d = R.depth_values(bad)
    assert (d[0, 0, :4] == 0).all() and np.array_equal(d[1:], R.depth_values(metres)[1:])
    near = R.fixture_reference(depth_trunc=1.4)                  # every depth of the plane is 1.417 or more: cut away
    p = near["points"].astype(np.float64)
    assert 0 < len(p) < 4000 and (p[:, 2] < 1.45).all()


def test_c_abi_declares_the_entries():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    assert "#define GMF_ABI_VERSION 5" in text
    camera = ["G", "F", "H", "W", "fx", "fy", "cx", "cy", "voxel_length", "sdf_trunc", "depth_scale", "depth_trunc"]
    want = {
        "gmf_tsdf_allocate": ["h", "depth", "depth_is_u16", "poses", "frame_offsets"] + camera + [
            "stride", "max_units", "unit_keys_out", "birth_out", "unit_offsets_out", "num_units", "stream"],
        "gmf_tsdf_integrate": ["h", "depth", "depth_is_u16", "poses_inv", "frame_offsets"] + camera + [
            "unit_keys", "unit_offsets", "birth", "num_units", "tsdf_out", "weight_out", "stream"],
        "gmf_tsdf_extract": ["h", "unit_keys", "unit_offsets", "G", "num_units", "tsdf", "weight", "voxel_length", "points_out",
                             "max_points", "point_offsets_out", "num_points", "stream"],
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


def test_argument_errors():
    import gmf_amd
    F = 3
    depth = torch.zeros(F, 8, 12, dtype=torch.float32)
    poses = torch.eye(4, dtype=torch.float64).repeat(F, 1, 1)
    K = (10.0, 10.0, 5.5, 3.5)
    singular = poses.clone()
    singular[1] = 0
    nan_pose = poses.clone()
    nan_pose[2, 0, 3] = float("nan")
    cases = [
        (dict(depth=depth.numpy()), "torch tensor"), (dict(depth=depth.double()), "uint16"), (dict(depth=depth.to(torch.int32)), "uint16"),
        (dict(depth=depth[0]), r"\[F,H,W\]"), (dict(depth=depth[None]), r"\[F,H,W\]"), (dict(depth=torch.zeros(F, 0, 12)), r"\[F,H,W\]"),
        (dict(poses=poses.numpy()), "torch tensor"), (dict(poses=poses.float()), "float64"), (dict(poses=poses[:2]), r"\[F,4,4\]"),
        (dict(poses=poses[:, :3]), r"\[F,4,4\]"), (dict(poses=singular), "invertible"), (dict(poses=nan_pose), "finite"),
        (dict(intrinsic=(10.0, 10.0, 5.5)), "intrinsic"), (dict(intrinsic=5.0), "intrinsic"), (dict(intrinsic=(0.0, 10.0, 5, 3)), "intrinsic"),
        (dict(intrinsic=(10.0, -1.0, 5, 3)), "intrinsic"), (dict(intrinsic=(10.0, 10.0, float("nan"), 3)), "intrinsic"),
        (dict(intrinsic=("a", 1, 2, 3)), "intrinsic"),
        (dict(frame_offsets=[0]), "frame_offsets"), (dict(frame_offsets=[1, 3]), "frame_offsets"), (dict(frame_offsets=[0, 2]), "frame_offsets"),
        (dict(frame_offsets=[0, 2, 1, 3]), "frame_offsets"), (dict(frame_offsets=[0, "a", 3]), "frame_offsets"),
        (dict(frame_offsets=[0, 1.5, 3]), "frame_offsets"), (dict(frame_offsets=7), "frame_offsets"),
        (dict(frame_offsets=[0] * 65536 + [3]), "65535 fragments"),
        (dict(voxel_length=0.0), "voxel_length"), (dict(voxel_length=float("inf")), "voxel_length"), (dict(voxel_length="x"), "voxel_length"),
        (dict(sdf_trunc=-0.04), "sdf_trunc"), (dict(sdf_trunc=float("nan")), "sdf_trunc"),
        (dict(depth_scale=0.0), "depth_scale"), (dict(depth_scale=float("inf")), "depth_scale"),
        (dict(depth_trunc=0.0), "depth_trunc"), (dict(depth_trunc=float("nan")), "depth_trunc"),
        (dict(depth_sampling_stride=0), "depth_sampling_stride"), (dict(depth_sampling_stride=2.0), "depth_sampling_stride"),
        (dict(max_units=0), "max_units"), (dict(max_units=(1 << 22) + 1), "max_units"), (dict(max_units=10.5), "max_units"),
        # and a valid call on CPU tensors, ragged or not, is refused as well
        (dict(), "no CPU fallback"), (dict(depth=depth.to(torch.uint16)), "no CPU fallback"),
        (dict(frame_offsets=[0, 0, 2, 3], return_volume=True), "no CPU fallback"), (dict(depth_trunc=float("inf")), "no CPU fallback"),
        (dict(depth=depth[:0], poses=poses[:0]), "no CPU fallback"),
    ]
    for kw, msg in cases:
        args = dict(depth=depth, poses=poses, intrinsic=K)
        args.update(kw)
        with pytest.raises(RuntimeError, match=msg) as e:
            gmf_amd.tsdf_fragments(args.pop("depth"), args.pop("poses"), args.pop("intrinsic"), **args)
        assert "tsdf_fragments" in str(e.value), kw
    big = torch.zeros(1, dtype=torch.float32).expand(65536, 1, 1)                      # too many frames for one fragment
    with pytest.raises(RuntimeError, match="65535 frames"):
        gmf_amd.tsdf_fragments(big, torch.eye(4, dtype=torch.float64).expand(65536, 4, 4), K)
