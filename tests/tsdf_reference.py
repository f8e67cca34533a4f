"""A numpy restatement of gmf_amd.tsdf_fragments (gmf_amd/fragments.py, csrc/tsdf_kernels.hip), operation for operation: the
contract of DESIGN.md section 4o.  Allocation and the vertex positions are float64, the integration is np.float32 with every
operation rounded on its own; tests/test_gpu_fragments.py holds the kernels to it bit for bit.  One fragment per call.

Also here: the fixture both test files share (a plane and a sphere ray-cast analytically, five poses, a hole), a second hand-made
volume on which the cube rule removes many crossings, and both results cached, so that the reference runs once per process."""
import functools

import numpy as np

RES = 16
f32 = np.float32


def depth_values(depth, depth_scale=1000.0, depth_trunc=4.5):
    """Step 1: [F,H,W] uint16 (sensor values) or float32 (metres) -> float32 metres, 0 = no measurement."""
    if depth.dtype == np.uint16:
        d = depth.astype(f32) / f32(depth_scale)
    else:
        d = depth.astype(f32).copy()
        d[~np.isfinite(d) | (d < 0)] = 0
    d[d >= f32(depth_trunc)] = 0
    return d


def allocate(d, poses, intrinsic, voxel_length, sdf_trunc, stride):
    """Step 2: unit keys [U,3] int32 in ascending (x, y, z) order and the frame that first touches each, birth [U] int32."""
    fx, fy, cx, cy = (float(v) for v in intrinsic)
    ul = RES * float(voxel_length)
    trunc = float(sdf_trunc)
    F, H, W = d.shape
    ii, jj = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    birth = {}
    for f in range(F):
        z = d[f][ii, jj].astype(np.float64)
        ok = z > 0
        if not ok.any():
            continue
        z = z[ok]
        x = (jj[ok] - cx) * z / fx
        y = (ii[ok] - cy) * z / fy
        P = np.asarray(poses[f], np.float64)
        p = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]
        lo = np.stack([np.floor((p[r] - trunc) / ul) for r in range(3)], 1).astype(np.int64)
        hi = np.stack([np.floor((p[r] + trunc) / ul) for r in range(3)], 1).astype(np.int64)
        if lo.min() < -32767 or hi.max() > 32767:
            raise ValueError("a unit index outside +-32767")
        span = (hi - lo).max(0)
        for dx in range(span[0] + 1):
            for dy in range(span[1] + 1):
                for dz in range(span[2] + 1):
                    k = lo + np.array([dx, dy, dz])
                    for key in np.unique(k[(k <= hi).all(1)], axis=0):
                        birth.setdefault(tuple(int(v) for v in key), f)
    keys = sorted(birth)
    return np.array(keys, np.int32).reshape(-1, 3), np.array([birth[k] for k in keys], np.int32)


def pixel_scale(intrinsic, H, W):
    """m[v,u] of step 3: the length of the ray through pixel (v, u) at z = 1, float64 rounded to float32."""
    fx, fy, cx, cy = (float(v) for v in intrinsic)
    a = (np.arange(W, dtype=np.float64)[None, :] - cx) / fx
    b = (np.arange(H, dtype=np.float64)[:, None] - cy) / fy
    return np.sqrt((a * a + b * b) + 1.0).astype(f32)


def voxel_centres(keys, voxel_length):
    """c_a of step 3 for the 16 positions of every unit along each axis: three [U,16] float32 arrays."""
    loc = np.arange(RES, dtype=np.int64)[None, :]
    return [(((RES * keys[:, a].astype(np.int64)[:, None] + loc) + 0.5) * float(voxel_length)).astype(f32) for a in range(3)]


def integrate(d, poses, intrinsic, voxel_length, sdf_trunc, keys, birth, from_birth=True):
    """Step 3: tsdf, weight [U,16,16,16] float32.  from_birth=False integrates every frame into every unit (not the contract: it
    exists so that a test can show that the fixture tells the two rules apart)."""
    F, H, W = d.shape
    U = len(keys)
    fx, fy, cx, cy = (f32(v) for v in intrinsic)
    m = pixel_scale(intrinsic, H, W)
    c = voxel_centres(keys, voxel_length)
    shape = (U, RES, RES, RES)
    X = np.broadcast_to(c[0][:, :, None, None], shape)
    Y = np.broadcast_to(c[1][:, None, :, None], shape)
    Z = np.broadcast_to(c[2][:, None, None, :], shape)
    T = np.zeros(shape, f32)
    Wt = np.zeros(shape, f32)
    trunc = f32(sdf_trunc)
    inv_trunc = f32(1.0 / float(trunc))
    eps = f32(1e-4)
    u_hi, v_hi = f32(W) - eps, f32(H) - eps
    for f in range(F):
        E = np.linalg.inv(np.asarray(poses[f], np.float64)).astype(f32)
        sel = np.flatnonzero(birth <= f) if from_birth else np.arange(U)
        if not len(sel):
            continue
        x, y, z = X[sel].ravel(), Y[sel].ravel(), Z[sel].ravel()
        q = [((E[r, 0] * x + E[r, 1] * y) + E[r, 2] * z) + E[r, 3] for r in range(3)]
        flat = (sel[:, None] * RES ** 3 + np.arange(RES ** 3)[None, :]).ravel()
        keep = q[2] > 0
        flat, qx, qy, qz = flat[keep], q[0][keep], q[1][keep], q[2][keep]
        uf = ((qx * fx) / qz + cx) + f32(0.5)
        vf = ((qy * fy) / qz + cy) + f32(0.5)
        assert uf.dtype == f32 and vf.dtype == f32
        keep = (uf >= eps) & (uf < u_hi) & (vf >= eps) & (vf < v_hi)
        flat, qz, uf, vf = flat[keep], qz[keep], uf[keep], vf[keep]
        u, v = uf.astype(np.int32), vf.astype(np.int32)
        dd = d[f][v, u]
        keep = dd > 0
        flat, qz, u, v, dd = flat[keep], qz[keep], u[keep], v[keep], dd[keep]
        sdf = (dd - qz) * m[v, u]
        keep = sdf > -trunc
        flat, sdf = flat[keep], sdf[keep]
        t = np.minimum(f32(1), sdf * inv_trunc)
        assert t.dtype == f32
        Tf, Wf = T.reshape(-1), Wt.reshape(-1)
        Tf[flat] = (Tf[flat] * Wf[flat] + t) / (Wf[flat] + f32(1))
        Wf[flat] = Wf[flat] + f32(1)
    return T, Wt


def extract(keys, tsdf, weight, voxel_length, cube_rule=True):
    """Step 4: the vertices [M,3] float32 in the contract's order.  cube_rule=False keeps every crossing (not the contract: it
    counts what the rule removes)."""
    U = len(keys)
    if U == 0:
        return np.zeros((0, 3), f32)
    vl = float(voxel_length)
    k = keys.astype(np.int64)
    kmin = k.min(0)
    dims = (k.max(0) - kmin + 1) * RES + 2              # one empty voxel around: every shifted slice stays inside
    val = np.full(dims, np.nan, np.float64)
    unit = np.full(dims, -1, np.int64)
    for i in range(U):
        o = (k[i] - kmin) * RES + 1
        sl = tuple(slice(o[a], o[a] + RES) for a in range(3))
        val[sl] = np.where(weight[i] > 0, tsdf[i].astype(np.float64), np.nan)
        unit[sl] = i
    obs = ~np.isnan(val)
    neg = val < 0

    def shifted(a, off):
        return a[tuple(slice(1 + off[i], a.shape[i] - 1 + off[i]) for i in range(3))]

    # cube[o] (o in the inner block's coordinates, shifted by -1..0): all eight corners observed
    cube = np.ones(tuple(s - 1 for s in dims), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cube &= obs[dx:dims[0] - 1 + dx, dy:dims[1] - 1 + dy, dz:dims[2] - 1 + dz]
    out = []
    for axis in range(3):
        e = [0, 0, 0]
        e[axis] = 1
        a_obs, b_obs = shifted(obs, (0, 0, 0)), shifted(obs, e)
        cross = a_obs & b_obs & (shifted(neg, (0, 0, 0)) != shifted(neg, e))
        if cube_rule:
            p, q = [a for a in range(3) if a != axis]
            anyc = np.zeros_like(cross)
            for dp in (0, -1):
                for dq in (0, -1):
                    off = [0, 0, 0]
                    off[p], off[q] = dp, dq
                    # cube array index i is the cube with origin i; the inner block starts at 1
                    anyc |= cube[tuple(slice(1 + off[i], dims[i] - 1 + off[i]) for i in range(3))]
            cross &= anyc
        idx = np.argwhere(cross) + 1                                     # coordinates in `val`
        if not len(idx):
            continue
        ta = np.abs(val[tuple(idx.T)])
        tb = np.abs(val[tuple((idx + e).T)])
        glob = idx - 1 + kmin * RES                                      # 16 k + local
        pos = (glob + 0.5) * vl
        pos[:, axis] = pos[:, axis] + (ta * vl) / (ta + tb)
        local = (idx - 1) % RES
        order = np.stack([unit[tuple(idx.T)], local[:, 0] * 256 + local[:, 1] * 16 + local[:, 2], np.full(len(idx), axis)], 1)
        out.append((order, pos.astype(f32)))
    if not out:
        return np.zeros((0, 3), f32)
    order = np.concatenate([o for o, _ in out])
    pts = np.concatenate([p for _, p in out])
    assert (order[:, 0] >= 0).all()
    rank = np.lexsort((order[:, 2], order[:, 1], order[:, 0]))
    return pts[rank]


def fragment(depth, poses, intrinsic, voxel_length=0.008, sdf_trunc=0.04, depth_scale=1000.0, depth_trunc=4.5,
             depth_sampling_stride=4, from_birth=True, cube_rule=True):
    """One fragment, every step -> dict(points, unit_keys, birth, tsdf, weight)."""
    d = depth_values(depth, depth_scale, depth_trunc)
    keys, birth = allocate(d, poses, intrinsic, voxel_length, sdf_trunc, depth_sampling_stride)
    T, Wt = integrate(d, poses, intrinsic, voxel_length, sdf_trunc, keys, birth, from_birth)
    pts = extract(keys, T, Wt, voxel_length, cube_rule)
    return dict(points=pts, unit_keys=keys, birth=birth, tsdf=T, weight=Wt)


# ---- the fixture --------------------------------------------------------------------------------------------------------------

H, W = 48, 64
INTRINSIC = (60.0, 60.0, 31.5, 23.5)
VOXEL, TRUNC, STRIDE = 0.02, 0.06, 4
PLANE_Z = 1.5
SPHERE_C, SPHERE_R = np.array([0.1, 0.0, 1.1]), 0.3
HOLE = (slice(5, 9), slice(10, 14))             # rows 5..8 x columns 10..13, zero in every frame


def fixture_pose(k):
    a = 0.12 * k
    P = np.eye(4)
    P[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    P[:3, 3] = [0.05 * k - 0.3, 0.02 * k, -0.1]
    return P


def raycast(P):
    """Depth (metres, float64; 0 = nothing hit) of the plane and the sphere seen from camera-to-world pose P."""
    fx, fy, cx, cy = INTRINSIC
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dirs = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones_like(i, float)], -1) @ P[:3, :3].T
    o = P[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        s_plane = np.where(dirs[..., 2] > 0, (PLANE_Z - o[2]) / dirs[..., 2], np.inf)
        oc = o - SPHERE_C
        a = (dirs * dirs).sum(-1)
        b = 2 * (dirs * oc).sum(-1)
        c = (oc * oc).sum() - SPHERE_R ** 2
        disc = b * b - 4 * a * c
        s_sphere = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    s_sphere = np.where(s_sphere > 0, s_sphere, np.inf)
    s_plane = np.where(s_plane > 0, s_plane, np.inf)
    s = np.minimum(s_plane, s_sphere)
    return np.where(np.isfinite(s), s, 0.0)


@functools.lru_cache(maxsize=None)
def fixture():
    """depth [5,48,64] uint16 (millimetres), poses [5,4,4] float64.  Treat both as read-only."""
    poses = np.stack([fixture_pose(k) for k in range(5)])
    depth = np.stack([np.round(raycast(P) * 1000.0) for P in poses]).astype(np.uint16)
    depth[(slice(None),) + HOLE] = 0
    depth.setflags(write=False)
    poses.setflags(write=False)
    return depth, poses


def fixture_args():
    return dict(voxel_length=VOXEL, sdf_trunc=TRUNC, depth_sampling_stride=STRIDE)


@functools.lru_cache(maxsize=None)
def fixture_reference(frames=(0, 1, 2, 3, 4), from_birth=True, cube_rule=True, depth_trunc=4.5):
    depth, poses = fixture()
    sel = list(frames)
    return fragment(depth[sel], poses[sel], INTRINSIC, depth_trunc=depth_trunc, from_birth=from_birth, cube_rule=cube_rule,
                    **fixture_args())


# ---- a volume on which the cube rule matters ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pinhole_fixture():
    """One frame of the plane alone seen from the first pose, with isolated single zero pixels (odd row, odd column) inside rows
    10..39 x columns 8..55: the voxels behind such a pixel stay unobserved along the whole ray, so between them the sign change
    has crossings whose four cubes all have an unobserved corner.  depth [1,48,64] uint16, poses [1,4,4]."""
    P = fixture_pose(0)
    fx, fy, cx, cy = INTRINSIC
    depth = np.full((1, H, W), 0, np.uint16)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dirs_z = ((np.stack([(j - cx) / fx, (i - cy) / fy, np.ones_like(i, float)], -1)) @ P[:3, :3].T)[..., 2]
    depth[0] = np.round((PLANE_Z - P[2, 3]) / dirs_z * 1000.0).astype(np.uint16)
    depth[0, 11:40:2, 9:56:2] = 0
    depth.setflags(write=False)
    return depth, P[None].copy()


@functools.lru_cache(maxsize=None)
def pinhole_reference(cube_rule=True):
    depth, poses = pinhole_fixture()
    return fragment(depth, poses, INTRINSIC, cube_rule=cube_rule, **fixture_args())
