"""A numpy restatement of steps 5 and 6 of DESIGN.md section 4o (gmf_amd.tsdf_extract_mesh, gmf_amd.tsdf_fragment_meshes;
csrc/tsdf_kernels.hip), operation for operation: a cube walk over the volume with the case table gmf_amd/_mc_table.py gives the
triangles, and with them the vertex set of step 4 (tests/test_fragments_mesh_host.py holds the walk's vertices to
tsdf_reference.extract bit for bit and in order); the vertex normals are float64 sums of triangle cross products over the
returned float32 positions.  tests/test_gpu_fragments_mesh.py holds the kernels to it bit for bit.  One fragment per call.

Also here: the random volume both test files share, and every result cached, so that the restatement runs once per process."""
import functools

import numpy as np

import tsdf_reference as R
from gmf_amd._mc_table import TRI_TABLE

RES = R.RES
f32 = np.float32

SHIFT = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)
EDGE_SHIFT = np.array([(0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 1, 1), (0, 1, 1, 0), (0, 0, 1, 1),
                       (0, 0, 0, 2), (1, 0, 0, 2), (1, 1, 0, 2), (0, 1, 0, 2)], np.int64)
EDGE_TO_VERT = np.array([(0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7)], np.int64)
TABLE = np.array(TRI_TABLE, np.int8)
assert TABLE.shape == (256, 16)
TRIANGLES_OF = (TABLE >= 0).sum(1) // 3


def cube_walk(keys, tsdf, weight):
    """Step 5 up to the vertex numbering.  -> dict: tri_edges [K,3] (each entry an edge id `cell * 3 + axis` of the dense grid, in
    the output order of the triangles and already in (e0, e2, e1) order), edge_ids [M] (the edges that carry a vertex, in step 4's
    order), cases [C] and origins [C,3] (global voxel coordinates) of the cubes that yield triangles, in walk order, and the dense
    grid's `val`, `dims`, `kmin`."""
    k = keys.astype(np.int64)
    kmin = k.min(0)
    dims = (k.max(0) - kmin + 1) * RES + 2              # one empty voxel around
    val = np.full(dims, np.nan, np.float64)
    unit = np.full(dims, -1, np.int64)
    for i in range(len(k)):
        o = (k[i] - kmin) * RES + 1
        sl = tuple(slice(o[a], o[a] + RES) for a in range(3))
        val[sl] = np.where(weight[i] > 0, tsdf[i].astype(np.float64), np.nan)
        unit[sl] = i
    obs = ~np.isnan(val)
    neg = val < 0
    inner = tuple(s - 1 for s in dims)
    observed = np.ones(inner, bool)
    case = np.zeros(inner, np.int64)
    for i, s in enumerate(SHIFT):
        sl = tuple(slice(s[a], s[a] + inner[a]) for a in range(3))
        observed &= obs[sl]
        case |= neg[sl].astype(np.int64) << i
    o = np.argwhere(observed & (case != 0) & (case != 255))           # coordinates in `val`
    local = (o - 1) % RES
    rank = np.lexsort((local[:, 0] * 256 + local[:, 1] * 16 + local[:, 2], unit[tuple(o.T)]))
    o = o[rank]
    cases = case[tuple(o.T)]
    count = TRIANGLES_OF[cases]
    first = np.concatenate([[0], np.cumsum(count)])
    tri_edges = np.zeros((first[-1], 3), np.int64)

    def edge_id(origin, e):
        a = origin + EDGE_SHIFT[e, :3]
        return ((a[:, 0] * dims[1] + a[:, 1]) * dims[2] + a[:, 2]) * 3 + EDGE_SHIFT[e, 3]

    for t in range(5):
        sel = np.flatnonzero(count > t)
        row = TABLE[cases[sel]].astype(np.int64)
        for slot, col in enumerate((3 * t, 3 * t + 2, 3 * t + 1)):     # (v(e0), v(e2), v(e1))
            tri_edges[first[sel] + t, slot] = edge_id(o[sel], row[:, col])
    ids = np.unique(tri_edges)
    cell, axis = ids // 3, ids % 3
    a = np.stack(np.unravel_index(cell, dims), 1)
    la = (a - 1) % RES
    rank = np.lexsort((axis, la[:, 0] * 256 + la[:, 1] * 16 + la[:, 2], unit[tuple(a.T)]))
    return dict(tri_edges=tri_edges, edge_ids=ids[rank], cases=cases, origins=o - 1 + kmin * RES, val=val, dims=dims, kmin=kmin)


def vertex_normals(points, triangles):
    """Step 6: [M,3] float32.  fp64 over the float32 positions, every operation rounded on its own, a vertex's triangles added in
    ascending triangle index."""
    p = points.astype(np.float64)
    i, j, l = triangles[:, 0], triangles[:, 1], triangles[:, 2]
    a, b = p[j] - p[i], p[l] - p[i]
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    s = np.zeros_like(p)
    vert = triangles.reshape(-1)                                       # triangle-major: a stable sort keeps triangle order
    tri = np.repeat(np.arange(len(triangles)), 3)
    order = np.argsort(vert, kind="stable")
    vert, tri = vert[order], tri[order]
    nth = np.arange(len(vert)) - np.searchsorted(vert, vert, side="left")      # 0 for a vertex's first triangle, 1 for its second
    for r in range(int(nth.max()) + 1 if len(nth) else 0):
        sel = nth == r
        s[vert[sel]] = s[vert[sel]] + n[tri[sel]]
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    good = np.isfinite(length) & (length > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (s / length[:, None]).astype(f32)
    out[~good] = (0, 0, 1)
    return out, s


def mesh(keys, tsdf, weight, voxel_length):
    """One fragment -> dict(points [M,3] float32, triangles [K,3] int32, normals [M,3] float32) and, for the tests, `sums` (the
    float64 normal sums), `cases`, `origins`."""
    if len(keys) == 0:
        return dict(points=np.zeros((0, 3), f32), triangles=np.zeros((0, 3), np.int32), normals=np.zeros((0, 3), f32),
                    sums=np.zeros((0, 3)), cases=np.zeros(0, np.int64), origins=np.zeros((0, 3), np.int64))
    w = cube_walk(keys, tsdf, weight)
    ids, dims, val = w["edge_ids"], w["dims"], w["val"]
    triangles = np.searchsorted(np.sort(ids), w["tri_edges"])
    back = np.argsort(ids)                                             # position in sorted ids -> vertex index
    triangles = back[triangles].astype(np.int32).reshape(-1, 3)
    # the positions of step 4, for the walk's vertices
    a = np.stack(np.unravel_index(ids // 3, dims), 1)
    axis = ids % 3
    b = a.copy()
    b[np.arange(len(a)), axis] += 1
    ta, tb = np.abs(val[tuple(a.T)]), np.abs(val[tuple(b.T)])
    vl = float(voxel_length)
    pos = ((a - 1 + w["kmin"] * RES) + 0.5) * vl
    pos[np.arange(len(a)), axis] = pos[np.arange(len(a)), axis] + (ta * vl) / (ta + tb)
    points = pos.astype(f32)
    normals, sums = vertex_normals(points, triangles)
    return dict(points=points, triangles=triangles, normals=normals, sums=sums, cases=w["cases"], origins=w["origins"])


def meshes(unit_keys, unit_offsets, tsdf, weight, voxel_length):
    """G fragments of one volume -> dict(points, point_offsets, triangles, triangle_offsets, normals) as the device returns them."""
    parts = [mesh(unit_keys[a:b], tsdf[a:b], weight[a:b], voxel_length) for a, b in zip(unit_offsets[:-1], unit_offsets[1:])]
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("points", "triangles", "normals")}
    out["point_offsets"] = np.cumsum([0] + [len(p["points"]) for p in parts]).astype(np.int32)
    out["triangle_offsets"] = np.cumsum([0] + [len(p["triangles"]) for p in parts]).astype(np.int32)
    out["parts"] = parts
    return out


@functools.lru_cache(maxsize=None)
def fixture_mesh(frames=(0, 1, 2, 3, 4)):
    r = R.fixture_reference(frames=frames)
    return mesh(r["unit_keys"], r["tsdf"], r["weight"], R.VOXEL)


@functools.lru_cache(maxsize=None)
def pinhole_mesh():
    r = R.pinhole_reference()
    return mesh(r["unit_keys"], r["tsdf"], r["weight"], R.VOXEL)


# ---- the random volume --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_volume():
    """A volume no camera could produce: 2 fragments on the 2x2x2 block of keys -1..0, the first without (0, -1, 0), the second
    whole (only there do cubes reach across the block's centre, into the +x+y+z neighbour); tsdf standard normal, about 3 % of
    the weights 0 and twenty tsdf exactly 0.
    -> unit_keys [15,3] int32, unit_offsets [3] int32, tsdf, weight [15,16,16,16] float32, read-only."""
    rng = np.random.default_rng(20240521)
    block = [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)]
    first = [k for k in block if k != (0, -1, 0)]
    second = list(block)
    keys = np.array(first + second, np.int32)
    off = np.array([0, len(first), len(first) + len(second)], np.int32)
    U = len(keys)
    tsdf = rng.standard_normal((U, RES, RES, RES)).astype(f32)
    weight = np.where(rng.random((U, RES, RES, RES)) < 0.03, 0, rng.integers(1, 6, (U, RES, RES, RES))).astype(f32)
    flat = tsdf.reshape(-1)
    flat[rng.choice(flat.size, 20, replace=False)] = 0
    for a in (keys, off, tsdf, weight):
        a.setflags(write=False)
    return keys, off, tsdf, weight


RANDOM_VOXEL = 0.0125


@functools.lru_cache(maxsize=None)
def random_meshes():
    keys, off, tsdf, weight = random_volume()
    return meshes(keys, off, tsdf, weight, RANDOM_VOXEL)
