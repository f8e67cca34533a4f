"""A numpy restatement of the colours of gmf_amd.tsdf_fragments_colored (gmf_amd/fragments.py, csrc/tsdf_kernels.hip): steps 3c and
4c of DESIGN.md section 4o, on top of tests/tsdf_reference.py, which it imports and does not repeat - the geometry it computes
beside the colours is asserted bitwise equal to that module's.  tests/test_gpu_fragments_color.py holds the kernels to it bit for
bit.  One fragment per call.

Also here: the colour frames of tsdf_reference's fixture (rendered from the world point each pixel hits, magenta where there is no
depth), and hand-made ramp volumes on which the colour of every vertex follows from 4c by hand."""
import functools

import numpy as np

import tsdf_reference as R

RES = R.RES
f32 = np.float32


def integrate_color(d, color, poses, intrinsic, voxel_length, sdf_trunc, keys, birth, dtype=f32, updates=None):
    """Steps 3 and 3c: tsdf, weight [U,16,16,16] float32 (asserted bitwise R.integrate's) and color_volume [U,16,16,16,3].  dtype is
    the type of the colour accumulators and of their arithmetic: float32 is the contract, float64 is what open3d keeps.  updates:
    a list that receives, per frame, the flat indices of the voxels the frame updated."""
    F, H, W = d.shape
    U = len(keys)
    fx, fy, cx, cy = (f32(v) for v in intrinsic)
    m = R.pixel_scale(intrinsic, H, W)
    c = R.voxel_centres(keys, voxel_length)
    shape = (U, RES, RES, RES)
    x = np.broadcast_to(c[0][:, :, None, None], shape).reshape(-1)
    y = np.broadcast_to(c[1][:, None, :, None], shape).reshape(-1)
    z = np.broadcast_to(c[2][:, None, None, :], shape).reshape(-1)
    T = np.zeros(U * RES ** 3, f32)
    Wt = np.zeros(U * RES ** 3, f32)
    Cv = np.zeros((U * RES ** 3, 3), dtype)
    trunc = f32(sdf_trunc)
    inv_trunc = f32(1.0 / float(trunc))
    eps = f32(1e-4)
    u_hi, v_hi = f32(W) - eps, f32(H) - eps
    born = np.repeat(birth, RES ** 3)
    for f in range(F):
        E = np.linalg.inv(np.asarray(poses[f], np.float64)).astype(f32)
        flat = np.flatnonzero(born <= f)
        q = [((E[r, 0] * x[flat] + E[r, 1] * y[flat]) + E[r, 2] * z[flat]) + E[r, 3] for r in range(3)]
        keep = q[2] > 0
        flat, qx, qy, qz = flat[keep], q[0][keep], q[1][keep], q[2][keep]
        uf = ((qx * fx) / qz + cx) + f32(0.5)
        vf = ((qy * fy) / qz + cy) + f32(0.5)
        keep = (uf >= eps) & (uf < u_hi) & (vf >= eps) & (vf < v_hi)
        flat, qz, uf, vf = flat[keep], qz[keep], uf[keep], vf[keep]
        u, v = uf.astype(np.int32), vf.astype(np.int32)
        dd = d[f][v, u]
        keep = dd > 0
        flat, qz, u, v, dd = flat[keep], qz[keep], u[keep], v[keep], dd[keep]
        sdf = (dd - qz) * m[v, u]
        keep = sdf > -trunc
        flat, sdf, u, v = flat[keep], sdf[keep], u[keep], v[keep]
        t = np.minimum(f32(1), sdf * inv_trunc)
        # 3c: the same voxels, the same pixel, the weight before the update; every operation rounded in `dtype`
        w = Wt[flat].astype(dtype)[:, None]
        px = color[f][v, u].astype(dtype)
        Cv[flat] = (Cv[flat] * w + px) / (w + dtype(1))
        assert Cv.dtype == dtype
        T[flat] = (T[flat] * Wt[flat] + t) / (Wt[flat] + f32(1))
        Wt[flat] = Wt[flat] + f32(1)
        if updates is not None:
            updates.append(flat)
    T, Wt = T.reshape(shape), Wt.reshape(shape)
    T0, W0 = R.integrate(d, poses, intrinsic, voxel_length, sdf_trunc, keys, birth)
    assert T.tobytes() == T0.tobytes() and Wt.tobytes() == W0.tobytes()
    return T, Wt, Cv.reshape(shape + (3,))


def vertex_edges(keys, tsdf, weight, cube_rule=True):
    """The edge of every vertex of R.extract, in its order: a [M,3] int64, the global index 16 k + local of the edge's first voxel,
    and axis [M].  R.extract itself says so: which edges yield a vertex, and their order, depend on the signs and the weights alone,
    so on a volume of -1 / +1 with voxel_length 1 it puts each vertex at a + 0.5 with the axis component at a + 1, all exact."""
    sign = np.where(tsdf < 0, f32(-1), f32(1))
    p = R.extract(keys, sign, weight, 1.0, cube_rule).astype(np.float64)
    whole = p == np.floor(p)
    assert (whole.sum(1) == 1).all()
    axis = whole.argmax(1)
    a = np.floor(p).astype(np.int64)
    a[np.arange(len(a)), axis] -= 1
    return a, axis


def extract_color(keys, tsdf, weight, color_volume, voxel_length, cube_rule=True, swapped=False):
    """Steps 4 and 4c: points [M,3] float32 (R.extract's) and colors [M,3] float32 in 0..1.  swapped=True gives a's colour the
    weight ta and b's tb (not the contract: it exists so that a test can show that the ramp volumes tell the two apart)."""
    pts = R.extract(keys, tsdf, weight, voxel_length, cube_rule)
    if not len(pts):
        return pts, np.zeros((0, 3), f32)
    a, axis = vertex_edges(keys, tsdf, weight, cube_rule)
    assert len(a) == len(pts)
    unit_of = {tuple(int(v) for v in k): i for i, k in enumerate(keys)}

    def at(g):
        unit = np.array([unit_of[tuple(k)] for k in (g >> 4).tolist()])
        loc = g & 15
        return unit, loc[:, 0], loc[:, 1], loc[:, 2]

    b = a.copy()
    b[np.arange(len(b)), axis] += 1
    ia, ib = at(a), at(b)
    assert (weight[ia] > 0).all() and (weight[ib] > 0).all()
    ta = np.abs(tsdf[ia].astype(np.float64))[:, None]
    tb = np.abs(tsdf[ib].astype(np.float64))[:, None]
    ca, cb = color_volume[ia].astype(np.float64), color_volume[ib].astype(np.float64)
    # the positions once more from the edges, to hold the edges themselves to R.extract
    pos = (a + 0.5) * float(voxel_length)
    pos[np.arange(len(a)), axis] = pos[np.arange(len(a)), axis] + (ta[:, 0] * float(voxel_length)) / (ta[:, 0] + tb[:, 0])
    assert pos.astype(f32).tobytes() == pts.tobytes()
    if swapped:
        ta, tb = tb, ta
    col = (((tb * ca) + (ta * cb)) / (ta + tb)) / 255.0
    return pts, col.astype(f32)


def fragment_color(depth, color, poses, intrinsic, voxel_length=0.008, sdf_trunc=0.04, depth_scale=1000.0, depth_trunc=4.5,
                   depth_sampling_stride=4, dtype=f32, updates=None):
    """One fragment, every step -> dict(points, colors, unit_keys, birth, tsdf, weight, color_volume)."""
    d = R.depth_values(depth, depth_scale, depth_trunc)
    keys, birth = R.allocate(d, poses, intrinsic, voxel_length, sdf_trunc, depth_sampling_stride)
    T, Wt, Cv = integrate_color(d, color, poses, intrinsic, voxel_length, sdf_trunc, keys, birth, dtype, updates)
    pts, col = extract_color(keys, T, Wt, Cv, voxel_length)
    return dict(points=pts, colors=col, unit_keys=keys, birth=birth, tsdf=T, weight=Wt, color_volume=Cv)


# ---- the colour fixture -------------------------------------------------------------------------------------------------------

MAGENTA = (255, 0, 255)


def analytic_rg(p):
    """R and G (0..255, not rounded) of world points p [...,3]."""
    return 127.5 + 127.5 * np.sin(2 * p[..., 0]), 127.5 + 127.5 * np.sin(2 * p[..., 1] + 1)


def frame_blue(k):
    return 40 * k + 20


@functools.lru_cache(maxsize=None)
def color_fixture():
    """color [5,48,64,3] uint8 for R.fixture(): with p the world point the pixel's ray hits (R.raycast), R = round(127.5 + 127.5
    sin(2 p_x)), G = round(127.5 + 127.5 sin(2 p_y + 1)), B = 40 k + 20 in frame k - so that keeping the first or the last frame's
    colour is not the running mean - and magenta wherever the depth is 0, the hole included: a colour nothing may ever read."""
    depth, poses = R.fixture()
    fx, fy, cx, cy = R.INTRINSIC
    i, j = np.meshgrid(np.arange(R.H), np.arange(R.W), indexing="ij")
    color = np.zeros((5, R.H, R.W, 3), np.uint8)
    for k, P in enumerate(poses):
        s = R.raycast(P)
        cam = np.stack([(j - cx) / fx * s, (i - cy) / fy * s, s], -1)
        p = cam @ P[:3, :3].T + P[:3, 3]
        r, g = analytic_rg(p)
        color[k, ..., 0] = np.round(r)
        color[k, ..., 1] = np.round(g)
        color[k, ..., 2] = frame_blue(k)
        color[k][depth[k] == 0] = MAGENTA
    color.setflags(write=False)
    return color


@functools.lru_cache(maxsize=None)
def color_fixture_reference(frames=(0, 1, 2, 3, 4), dtype=f32):
    depth, poses = R.fixture()
    sel = list(frames)
    out = fragment_color(depth[sel], color_fixture()[sel], poses[sel], R.INTRINSIC, dtype=dtype, **R.fixture_args())
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- hand-made ramp volumes ---------------------------------------------------------------------------------------------------

RAMP_CASES = tuple((axis, units) for axis in range(3) for units in (1, 2))


@functools.lru_cache(maxsize=None)
def ramp_volume(axis, units):
    """One unit (0, 0, 0), or two with the second next to it along `axis`, every voxel of weight 1; tsdf = (X_axis - (cross +
    0.25)) / 16 in global voxel coordinates X, with cross = 7 (one unit) or 15 (two: the edge's far end is the next unit's voxel 0),
    so that exactly the 256 edges along `axis` from X_axis = cross change sign, with ta : tb = 1 : 3; colours are the small integers
    ((x + 2 y) % 256, (y + 3 z) % 256, (z + 5 x) % 256).  -> dict(unit_keys, tsdf, weight, color_volume, cross, expected), expected
    [256,3] float32 being 4c by hand: ta = 1/64, tb = 3/64, so ((tb c_a + ta c_b) / (ta + tb)) / 255 = ((3 c_a + c_b) / 4) / 255
    with every step before the last division exact."""
    cross = 7 if units == 1 else 15
    keys = np.zeros((units, 3), np.int32)
    keys[1:, axis] = 1
    loc = np.stack(np.meshgrid(*([np.arange(RES)] * 3), indexing="ij"), -1)              # [16,16,16,3]
    X = loc[None] + RES * keys[:, None, None, None, :].astype(np.int64)                   # [units,16,16,16,3]
    tsdf = ((X[..., axis] - (cross + 0.25)) / 16).astype(f32)
    weight = np.ones(tsdf.shape, f32)

    def colour(g):
        x, y, z = g[..., 0], g[..., 1], g[..., 2]
        return np.stack([(x + 2 * y) % 256, (y + 3 * z) % 256, (z + 5 * x) % 256], -1).astype(np.float64)

    p, q = [i for i in range(3) if i != axis]
    a = np.zeros((RES, RES, 3), np.int64)                                                 # the edges' first voxels, in local-index order
    a[..., axis] = cross
    a[..., p], a[..., q] = np.meshgrid(np.arange(RES), np.arange(RES), indexing="ij")
    b = a.copy()
    b[..., axis] += 1
    expected = (((3 * colour(a) + colour(b)) / 4) / 255.0).astype(f32).reshape(-1, 3)
    out = dict(unit_keys=keys, tsdf=tsdf, weight=weight, color_volume=colour(X).astype(f32), cross=cross, expected=expected)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
