"""CPU-side checks of the fragment meshes (gmf_amd.tsdf_extract_mesh, gmf_amd.tsdf_fragment_meshes): the case table
gmf_amd/_mc_table.py against the properties that pin it (it was written from memory: there is no copy to compare it with) and the
kernels' copy against it; the restatement tests/tsdf_mesh_reference.py, which tests/test_gpu_fragments_mesh.py holds the device to,
on the two fixtures of tests/tsdf_reference.py and on a random volume; the normals against the analytic scene; the C ABI entry; and
every argument error."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import tsdf_mesh_reference as M
import tsdf_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def directed_edges(tri):
    """[3K] codes of the directed edges (i -> j), (j -> l), (l -> i) of triangles [K,3], and the codes of their reverses."""
    t = tri.astype(np.int64)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    return (a << 32) | b, (b << 32) | a


# ---- the table ----------------------------------------------------------------------------------------------------------------

def test_table_rows_use_exactly_the_crossing_edges():
    assert M.TABLE.shape == (256, 16) and M.TABLE.dtype == np.int8
    total = 0
    for case in range(256):
        row = M.TABLE[case]
        n = int((row >= 0).sum())
        assert (row[:n] >= 0).all() and (row[n:] == -1).all(), case            # entries, then the terminator and padding
        assert n % 3 == 0 and n // 3 <= 5, case
        crossing = {e for e, (a, b) in enumerate(M.EDGE_TO_VERT) if ((case >> a) & 1) != ((case >> b) & 1)}
        assert set(row[:n].tolist()) == crossing, case
        total += n // 3
    assert total == 820
    assert M.TABLE[1, :4].tolist() == [0, 8, 3, -1] and M.TABLE[3, :7].tolist() == [1, 8, 3, 9, 8, 1, -1]
    assert M.TABLE[254, :4].tolist() == [0, 3, 8, -1]
    # the numbering the table is read with: an edge joins the corners its shift says
    for e, (a, b) in enumerate(M.EDGE_TO_VERT):
        axis = M.EDGE_SHIFT[e, 3]
        assert (M.SHIFT[a] == M.EDGE_SHIFT[e, :3]).all() and (M.SHIFT[b] - M.SHIFT[a]).tolist() == [int(axis == i) for i in range(3)]


def test_kernel_copy_of_the_table_equals_the_module():
    """csrc/tsdf_mc_table.inc is checked against gmf_amd/_mc_table.py here (tools/gen_mc_table.py writes it from there)."""
    text = open(os.path.join(ROOT, "gmf_amd", "csrc", "tsdf_mc_table.inc")).read()
    rows = re.findall(r"^\{([^}]*)\},$", text, re.M)
    assert len(rows) == 256
    assert np.array_equal(np.array([[int(v) for v in r.split(",")] for r in rows], np.int8), M.TABLE)
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.text() == text
    assert '#include "tsdf_mc_table.inc"' in open(os.path.join(ROOT, "gmf_amd", "csrc", "tsdf_kernels.hip")).read()


def _one_unit_mesh(field):
    """The restatement on a field that fits one unit (values on a sub-grid, everything else unobserved)."""
    n = field.shape[0]
    tsdf = np.zeros((1, 16, 16, 16), np.float32)
    weight = np.zeros((1, 16, 16, 16), np.float32)
    tsdf[0, :n, :n, :n] = field
    weight[0, :n, :n, :n] = 1
    return M.mesh(np.zeros((1, 3), np.int32), tsdf, weight, 1.0)


def test_random_fields_give_closed_consistently_wound_surfaces():
    """Standard normal values on a 7^3 grid inside a positive shell (9^3 with the shell), 40 seeds: every directed edge occurs
    exactly once and its reverse exactly once - closed, crack-free and consistently wound, ambiguous faces included."""
    for seed in range(40):
        field = np.ones((9, 9, 9), np.float32)
        field[1:8, 1:8, 1:8] = np.random.default_rng(seed).standard_normal((7, 7, 7)).astype(np.float32)
        m = _one_unit_mesh(field)
        code, rev = directed_edges(m["triangles"])
        assert len(code) > 300, seed
        assert len(np.unique(code)) == len(code), seed
        assert np.array_equal(np.sort(code), np.sort(rev)), seed


def test_sampled_sphere_is_a_sphere_wound_outwards():
    g = np.arange(12) - 5.5
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    m = _one_unit_mesh((np.sqrt(x * x + y * y + z * z) - 3.7).astype(np.float32))
    tri, p = m["triangles"], m["points"].astype(np.float64)
    code, rev = directed_edges(tri)
    assert len(np.unique(code)) == len(code) and np.array_equal(np.sort(code), np.sort(rev))
    V, E, F = len(p), len(code) // 2, len(tri)
    assert V - E + F == 2 and F == 524                             # Euler characteristic 2 (radius 3.7 on a 12^3 grid: 524 triangles)
    n = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    centre = (p[tri].mean(1)) - (0.5 + 5.5)                      # voxel i has its centre at i + 0.5
    assert ((n * centre).sum(1) > 0).all()
    assert ((m["normals"].astype(np.float64) * (p - 6.0)).sum(1) > 0).all()


# ---- the restatement on the two fixtures ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,vertices,triangles,boundary", [("fixture", 12991, 24747, 1269), ("pinhole", 3906, 6468, 1422)])
def test_restatement_figures(name, vertices, triangles, boundary):
    """The figures of the issue's prototype, confirmed by the committed restatement (they agree exactly)."""
    ref = R.fixture_reference() if name == "fixture" else R.pinhole_reference()
    m = M.fixture_mesh() if name == "fixture" else M.pinhole_mesh()
    assert m["points"].dtype == np.float32 and m["points"].tobytes() == ref["points"].tobytes()      # bit for bit, in order
    assert m["points"].shape == (vertices, 3)
    tri = m["triangles"]
    assert tri.dtype == np.int32 and tri.shape == (triangles, 3) and tri.min() == 0 and tri.max() == vertices - 1
    assert len(np.unique(tri)) == vertices                                  # every vertex is in a triangle
    code, rev = directed_edges(tri)
    assert len(np.unique(code)) == len(code)                                # no directed edge twice
    assert int((~np.isin(code, rev)).sum()) == boundary
    p = m["points"].astype(np.float64)
    n = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    assert (np.abs(n).sum(1) > 0).all()                                     # no degenerate triangle
    assert (np.abs(m["sums"]).sum(1) > 0).all()                             # no zero sum
    length = np.linalg.norm(m["normals"].astype(np.float64), axis=1)
    assert m["normals"].dtype == np.float32 and np.abs(length - 1).max() < 2e-7


def test_normals_against_the_scene():
    """Over vertices within a quarter voxel of one analytic surface and three voxels from the other.  Measured on the restatement:
    plane (10428 vertices) n . (0,0,-1) at least 0.886926, mean 0.995552; sphere (1617 vertices) n . radial mean 0.990145, 1st
    percentile 0.902309, smallest 0.337420 (silhouette vertices, where the mesh joins the sphere to the plane behind it), 0.99 %
    below 0.9.  The restatement is deterministic, so the margins only leave room for another libm's last bits in the fixture's
    ray casting: 0.005 on each figure, and 2 % for the share."""
    m = M.fixture_mesh()
    p, n = m["points"].astype(np.float64), m["normals"].astype(np.float64)
    rad = p - R.SPHERE_C
    d_plane, d_sphere = np.abs(p[:, 2] - R.PLANE_Z), np.abs(np.linalg.norm(rad, axis=1) - R.SPHERE_R)
    plane = (d_plane < R.VOXEL / 4) & (d_sphere > 3 * R.VOXEL)
    sphere = (d_sphere < R.VOXEL / 4) & (d_plane > 3 * R.VOXEL)
    a = -n[plane, 2]
    b = (n[sphere] * rad[sphere]).sum(1) / np.linalg.norm(rad[sphere], axis=1)
    print(f"plane {plane.sum()}: min {a.min():.6f} mean {a.mean():.6f}; sphere {sphere.sum()}: mean {b.mean():.6f} "
          f"p1 {np.percentile(b, 1):.6f} min {b.min():.6f} below 0.9: {(b < 0.9).mean():.4f}")
    assert plane.sum() > 10000 and sphere.sum() > 1500
    assert a.min() >= 0.8869 - 0.005 and a.mean() >= 0.9956 - 0.005
    assert b.mean() >= 0.9901 - 0.005
    assert (b < 0.9).mean() <= 0.02
    # the flat volume: every normal looks at the camera
    q = M.pinhole_mesh()["normals"]
    assert (-q[:, 2]).min() > 0.9999


# ---- the random volume ----------------------------------------------------------------------------------------------------------

def test_random_volume_reaches_every_case_and_every_neighbour():
    keys, off, tsdf, weight = M.random_volume()
    assert off.tolist() == [0, 7, 15] and (keys < 0).any() and len({tuple(k) for k in keys[:7]}) == 7
    assert 0.02 < (weight == 0).mean() < 0.04 and int((tsdf == 0).sum()) >= 20
    for a, b in zip(off[:-1], off[1:]):
        assert [tuple(k) for k in keys[a:b]] == sorted(tuple(k) for k in keys[a:b])
    r = M.random_meshes()
    assert r["point_offsets"].tolist() == [0, 38271, 82391] and r["triangle_offsets"].tolist() == [0, 64023, 139540]
    cases = np.concatenate([p["cases"] for p in r["parts"]])
    assert len(np.unique(cases)) == 254                                     # every case but 0 and 255
    # A cube's corners reach into each of the seven positive neighbour units, and its edges START in each of the six an edge can
    # start in: no cube edge starts at the corner (1, 1, 1), so (+x, +y, +z) holds a corner (number 6) and never an edge's start.
    corner_dirs, start_dirs = set(), set()
    for part in r["parts"]:
        local = part["origins"] % 16
        for i in range(8):
            corner_dirs |= {tuple(v) for v in np.unique((local + M.SHIFT[i]) >> 4, axis=0)}
        rows = M.TABLE[part["cases"]]
        for e in range(12):
            used = (rows == e).any(1)
            start_dirs |= {tuple(v) for v in np.unique((local[used] + M.EDGE_SHIFT[e, :3]) >> 4, axis=0)}
    seven = {(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)} - {(0, 0, 0)}
    assert corner_dirs - {(0, 0, 0)} == seven
    assert start_dirs - {(0, 0, 0)} == seven - {(1, 1, 1)}
    for g, part in enumerate(r["parts"]):
        a, b = off[g], off[g + 1]
        assert part["points"].tobytes() == R.extract(keys[a:b], tsdf[a:b], weight[a:b], M.RANDOM_VOXEL).tobytes()
        code, _ = directed_edges(part["triangles"])
        assert len(np.unique(code)) == len(code) and len(np.unique(part["triangles"])) == len(part["points"])
    # the volume also has what the fixtures lack: degenerate triangles and a vertex whose sum is zero, so the (0, 0, 1) fallback
    sums = np.concatenate([p["sums"] for p in r["parts"]])
    zero = np.abs(sums).sum(1) == 0
    assert zero.sum() == 1 and r["normals"][zero].tolist() == [[0.0, 0.0, 1.0]]
    assert np.isfinite(r["normals"]).all()


# ---- the interface --------------------------------------------------------------------------------------------------------------

def test_public_names_exported():
    import gmf_amd
    for name in ("tsdf_extract_mesh", "tsdf_fragment_meshes", "TsdfMeshes"):
        assert hasattr(gmf_amd, name) and name in gmf_amd.__all__
    assert gmf_amd.TsdfMeshes._fields == ("points", "point_offsets", "triangles", "triangle_offsets", "normals", "colors")
    assert list(inspect.signature(gmf_amd.tsdf_extract_mesh).parameters) == ["unit_keys", "unit_offsets", "tsdf", "weight", "voxel_length",
                                                                             "color_volume"]
    sig = inspect.signature(gmf_amd.tsdf_fragment_meshes)
    base = inspect.signature(gmf_amd.tsdf_fragments)
    assert list(sig.parameters) == list(base.parameters)[:-1] + ["color", "return_volume"]
    assert all(sig.parameters[k].default == v.default for k, v in base.parameters.items())
    assert sig.parameters["color"].default is None
    doc = gmf_amd.tsdf_extract_mesh.__doc__
    assert "only through weight > 0" in doc and "ascending in (x, y, z) and distinct" in doc


def test_c_abi_declares_the_entry():
    from gmf_amd import _lib
    text = open(os.path.join(ROOT, "include", "gmf_hip.h")).read()
    assert "#define GMF_ABI_VERSION 5" in text
    name = "gmf_tsdf_extract_mesh"
    params = ["h", "unit_keys", "unit_offsets", "G", "num_units", "tsdf", "weight", "color", "voxel_length", "points_out", "normals_out",
              "colors_out", "max_points", "triangles_out", "max_triangles", "point_offsets_out", "triangle_offsets_out", "num_points",
              "num_triangles", "stream"]
    source = open(os.path.join(ROOT, "gmf_amd", "csrc", "gmf_api.cpp")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*)\)\s*;", text)
    assert m
    assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == params
    d = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*)\)\s*\{", source)
    assert d and " ".join(d.group(1).split()) == " ".join(m.group(1).split())          # the definition repeats the declaration
    assert len(_lib.SIGNATURES[name][1]) == len(params)
    lib = _lib.load_library()
    assert hasattr(lib, name) and lib.gmf_abi_version() == 5


def test_argument_errors():
    import gmf_amd
    U = 2
    keys = torch.zeros(U, 3, dtype=torch.int32)
    vol = torch.zeros(U, 16, 16, 16)
    cvol = torch.zeros(U, 16, 16, 16, 3)
    cases = [
        (dict(unit_keys=keys.numpy()), "`unit_keys` must be a torch tensor"), (dict(unit_keys=keys.long()), "`unit_keys` must be int32"),
        (dict(unit_keys=keys[:, :2]), r"\[U,3\]"), (dict(unit_keys=keys[0]), r"\[U,3\]"),
        (dict(tsdf=None), "`tsdf` must be a torch tensor"), (dict(tsdf=vol.double()), "`tsdf` must be float32"),
        (dict(tsdf=vol[:1]), r"`tsdf` must be \[U,16,16,16\] with unit_keys' U = 2"), (dict(tsdf=vol.reshape(U, 4096)), r"`tsdf` must be \[U,16,16,16\]"),
        (dict(weight=vol.numpy()), "`weight` must be a torch tensor"), (dict(weight=vol.half()), "`weight` must be float32"),
        (dict(weight=vol[:, :8]), r"`weight` must be \[U,16,16,16\]"),
        (dict(color_volume=cvol.numpy()), "`color_volume` must be a torch tensor"), (dict(color_volume=cvol.to(torch.uint8)), "`color_volume` must be float32"),
        (dict(color_volume=vol), r"`color_volume` must be \[U,16,16,16,3\]"),
        (dict(color_volume=torch.zeros(U, 16, 16, 16, 3, device="meta")), "must live on the same device"),
        (dict(voxel_length=0.0), "voxel_length"), (dict(voxel_length=float("nan")), "voxel_length"), (dict(voxel_length="x"), "voxel_length must be a number"),
        (dict(unit_offsets=[0]), "unit_offsets"), (dict(unit_offsets=[0, 1]), "unit_offsets must ascend from 0 to the row count 2"),
        (dict(unit_offsets=[0, 2, 1, 2]), "unit_offsets"), (dict(unit_offsets=[0, "a", 2]), "unit_offsets must be B \\+ 1 integers"),
        (dict(unit_offsets=[0] * 65536 + [2]), "65535 fragments"),
        # and a valid call on CPU tensors, ragged or not, is refused as well
        (dict(), "no CPU fallback"), (dict(unit_offsets=[0, 0, 1, 2], color_volume=cvol), "no CPU fallback"),
        (dict(unit_offsets=torch.tensor([0, 2], dtype=torch.int32)), "no CPU fallback"),
        (dict(unit_keys=keys[:0], tsdf=vol[:0], weight=vol[:0], unit_offsets=[0, 0]), "no CPU fallback"),
    ]
    for kw, msg in cases:
        args = dict(unit_keys=keys, unit_offsets=[0, U], tsdf=vol, weight=vol, voxel_length=0.01)
        args.update(kw)
        with pytest.raises(RuntimeError, match=msg) as e:
            gmf_amd.tsdf_extract_mesh(**args)
        assert "gmf_amd.tsdf_extract_mesh: " in str(e.value), kw
    # tsdf_fragment_meshes checks as tsdf_fragments and tsdf_fragments_colored do, under its own name
    F = 3
    depth = torch.zeros(F, 8, 12, dtype=torch.float32)
    poses = torch.eye(4, dtype=torch.float64).repeat(F, 1, 1)
    K = (10.0, 10.0, 5.5, 3.5)
    color = torch.zeros(F, 8, 12, 3, dtype=torch.uint8)
    for kw, msg in [(dict(depth=depth.double()), "uint16"), (dict(poses=poses[:2]), r"\[F,4,4\]"), (dict(intrinsic=5.0), "intrinsic"),
                    (dict(frame_offsets=[0, 2]), "frame_offsets"), (dict(voxel_length=0.0), "voxel_length"), (dict(max_units=0), "max_units"),
                    (dict(color=color.float()), "`color` must be uint8"), (dict(color=color[:2]), r"`color` must be \[F,H,W,3\]"),
                    (dict(color=color.numpy()), "`color` must be a torch tensor"),
                    (dict(), "no CPU fallback"), (dict(color=color, return_volume=True), "no CPU fallback")]:
        args = dict(depth=depth, poses=poses, intrinsic=K)
        args.update(kw)
        with pytest.raises(RuntimeError, match=msg) as e:
            gmf_amd.tsdf_fragment_meshes(args.pop("depth"), args.pop("poses"), args.pop("intrinsic"), **args)
        assert "gmf_amd.tsdf_fragment_meshes: " in str(e.value), kw
