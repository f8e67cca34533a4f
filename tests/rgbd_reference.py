"""A numpy restatement of gmf_amd.rgbd (gmf_amd/rgbd.py, csrc/rgbd_kernels.hip), operation for operation: the contract of
DESIGN.md section 4p (open3d 0.9's RGB-D odometry with the hybrid Jacobian, as remembered: open3d itself could not be run).
Images are np.float32 with every operation rounded on its own, geometry is float64.  tests/test_gpu_rgbd.py holds the kernels
to it: planes and correspondence maps exactly, sums and poses within the bounds worked out there.

Also here: the fixture both test files share (the plane and the sphere of tsdf_reference.py under five close poses, textured),
its pyramids and its odometry runs, cached, so that the restatement runs once per process."""
import functools

import numpy as np

import tsdf_reference as TR

f32, f64 = np.float32, np.float64
GAUSS = (0.25, 0.5, 0.25)
SOBEL_D = (-1.0, 0.0, 1.0)
SOBEL_S = (1.0, 2.0, 1.0)
LAMBDA_DEP = 0.968
SOBEL_SCALE = 0.125
NAMES = ("I", "D", "Idx", "Idy", "Ddx", "Ddy")


# ---- steps 1-3: planes ------------------------------------------------------------------------------------------------------------

def depth_plane(depth, depth_scale=1000.0, depth_trunc=3.0, min_depth=0.0, max_depth=4.0):
    """Step 1: float32 metres, NaN = no measurement."""
    d = TR.depth_values(np.asarray(depth), depth_scale, depth_trunc).copy()
    d[(d < f32(min_depth)) | (d > f32(max_depth)) | (d <= 0)] = np.nan
    return d


def intensity(color):
    color = np.asarray(color)
    if color.dtype == np.uint8 and color.ndim == 3:
        return color.astype(f32) / f32(255)
    if color.dtype == np.uint8 and color.ndim == 4:
        c = color.astype(f32)
        return ((f32(0.2990) * c[..., 0] + f32(0.5870) * c[..., 1]) + f32(0.1140) * c[..., 2]) / f32(255)
    assert color.dtype == np.float32 and color.ndim == 3
    return color.copy()


def _pass(img, k, axis):
    n = img.shape[axis]
    i = np.arange(n)
    acc = np.zeros(img.shape, f64)
    with np.errstate(invalid="ignore"):
        for tap in (-1, 0, 1):
            acc = acc + k[tap + 1] * np.take(img, np.clip(i + tap, 0, n - 1), axis=axis).astype(f64)
    return acc.astype(f32)


def filter3(img, kx, ky):
    """Step 2: Filter(kx, ky) over the last two axes of a float32 array."""
    return _pass(_pass(img, kx, -1), ky, -2)


def down(img):
    h, w = img.shape[-2] // 2, img.shape[-1] // 2
    a = img[..., :2 * h, :2 * w]
    with np.errstate(invalid="ignore"):
        return (((a[..., 0::2, 0::2] + a[..., 0::2, 1::2]) + a[..., 1::2, 0::2]) + a[..., 1::2, 1::2]) / f32(4)


def pyramid(color, depth, depth_scale=1000.0, depth_trunc=3.0, min_depth=0.0, max_depth=4.0, levels=3):
    """Steps 1-3 -> a list over levels of [F,6,h,w] float32 (I, D, Idx, Idy, Ddx, Ddy)."""
    I = filter3(intensity(color), GAUSS, GAUSS)
    D = filter3(depth_plane(depth, depth_scale, depth_trunc, min_depth, max_depth), GAUSS, GAUSS)
    out = []
    for l in range(levels):
        if l:
            I, D = down(filter3(I, GAUSS, GAUSS)), down(D)
        out.append(np.stack([I, D, filter3(I, SOBEL_D, SOBEL_S), filter3(I, SOBEL_S, SOBEL_D), filter3(D, SOBEL_D, SOBEL_S),
                             filter3(D, SOBEL_S, SOBEL_D)], 1))
    return out


def level_intrinsic(K, l):
    return tuple(float(v) * 2.0 ** -l for v in K)


# ---- step 4: correspondences ------------------------------------------------------------------------------------------------------

def geometry(K, T):
    """M = K R K^-1 (K^-1 written out) and k = K t, float64, in the order the kernel uses."""
    fx, fy, cx, cy = K
    R, t = T[:3, :3], T[:3, 3]
    KR = np.stack([fx * R[0] + cx * R[2], fy * R[1] + cy * R[2], R[2]])
    M = np.empty((3, 3))
    M[:, 0] = KR[:, 0] / fx
    M[:, 1] = KR[:, 1] / fy
    M[:, 2] = KR[:, 2] - (M[:, 0] * cx + M[:, 1] * cy)
    return M, np.array([fx * t[0] + cx * t[2], fy * t[1] + cy * t[2], t[2]])


def correspondence_map(K, T, Ds, Dt, max_depth_diff=0.03, tie_largest=False, stats=None):
    """Step 4 -> [h,w] int32: per target pixel the winning source pixel v_s*w + u_s, or -1.  stats (a dict) collects the number
    of target pixels whose two best candidates have equal d_s, and the two margins of a discrete decision."""
    h, w = Ds.shape
    M, k = geometry(K, np.asarray(T, f64))
    v, u = np.mgrid[0:h, 0:w]
    ok = ~np.isnan(Ds)
    us, vs, ds, src = u[ok].astype(f64), v[ok].astype(f64), Ds[ok].astype(f64), (v[ok] * w + u[ok]).astype(np.int64)
    p = [ds * ((M[i, 0] * us + M[i, 1] * vs) + M[i, 2]) + k[i] for i in range(3)]
    z = p[2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fu, fv = p[0] / z + 0.5, p[1] / z + 0.5
        fin = np.isfinite(fu) & np.isfinite(fv) & (np.abs(fu) < 2.0 ** 30) & (np.abs(fv) < 2.0 ** 30)
    fu, fv, z, ds, src = fu[fin], fv[fin], z[fin], ds[fin], src[fin]
    if stats is not None and len(fu):
        px = min(np.abs(fu - np.round(fu)).min(), np.abs(fv - np.round(fv)).min())
        stats["pixel_margin"] = min(stats.get("pixel_margin", np.inf), float(px))
    ut, vt = np.trunc(fu).astype(np.int64), np.trunc(fv).astype(np.int64)
    inside = (ut >= 0) & (ut < w) & (vt >= 0) & (vt < h)
    ut, vt, z, ds, src = ut[inside], vt[inside], z[inside], ds[inside], src[inside]
    dt = Dt[vt, ut].astype(f64)
    seen = ~np.isnan(dt)
    diff = np.abs(z[seen] - dt[seen])
    if stats is not None and len(diff):
        stats["depth_margin"] = min(stats.get("depth_margin", np.inf), float(np.abs(diff - max_depth_diff).min()))
    keep = diff <= max_depth_diff
    tgt, ds, src = (vt * w + ut)[seen][keep], ds[seen][keep], src[seen][keep]
    out = np.full(h * w, -1, np.int32)
    if len(tgt):
        order = np.lexsort((-src if tie_largest else src, ds, tgt))
        tgt, ds, src = tgt[order], ds[order], src[order]
        first = np.r_[True, tgt[1:] != tgt[:-1]]
        out[tgt[first]] = src[first]
        if stats is not None:
            second = np.r_[False, first[:-1]] & ~first                       # the runner-up of its target pixel
            stats["ties"] = stats.get("ties", 0) + int((ds[second] == ds[np.flatnonzero(second) - 1]).sum())
    return out.reshape(h, w)


def pairs_of(cmap):
    """The correspondence list of a map, in ascending target order: (target index, source index)."""
    tgt = np.flatnonzero(cmap.ravel() >= 0)
    return tgt, cmap.ravel()[tgt].astype(np.int64)


# ---- steps 5-7 --------------------------------------------------------------------------------------------------------------------

def scales(cmap, I_src, I_tgt, reverse=False):
    tgt, src = pairs_of(cmap)
    if reverse:
        tgt, src = tgt[::-1], src[::-1]
    if not len(tgt):
        return None
    n = len(tgt)
    return 0.5 / (I_src.ravel()[src].astype(f64).sum() / n), 0.5 / (I_tgt.ravel()[tgt].astype(f64).sum() / n)


def source_points(K, Ds, src):
    """(x, y, z) of the source pixels `src`: open3d's float32 xyz image, as float64."""
    fx, fy, cx, cy = K
    w = Ds.shape[1]
    z = Ds.ravel()[src].astype(f64)
    x = ((((src % w).astype(f64) - cx) * z) / fx).astype(f32).astype(f64)
    y = ((((src // w).astype(f64) - cy) * z) / fy).astype(f32).astype(f64)
    return x, y, z


def jacobian_rows(K, T, Ps, Pt, cmap, s_src, s_tgt):
    """The two rows [n,2,6] and residuals [n,2] of RGBDOdometryJacobianFromHybridTerm; Ps, Pt: [6,h,w] planes."""
    fx, fy = K[0], K[1]
    T = np.asarray(T, f64)
    tgt, src = pairs_of(cmap)
    x, y, z = source_points(K, Ps[1], src)
    p = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)]
    at = lambda plane: Pt[plane].ravel()[tgt].astype(f64)
    sl_img, sl_dep = np.sqrt(1.0 - LAMBDA_DEP), np.sqrt(LAMBDA_DEP)
    diff_photo = s_tgt * at(0) - s_src * Ps[0].ravel()[src].astype(f64)
    dIdx, dIdy = SOBEL_SCALE * (s_tgt * at(2)), SOBEL_SCALE * (s_tgt * at(3))
    dDdx, dDdy = SOBEL_SCALE * at(4), SOBEL_SCALE * at(5)
    dDdx[np.isnan(dDdx)] = 0
    dDdy[np.isnan(dDdy)] = 0
    diff_geo = at(1) - p[2]
    invz = 1.0 / p[2]
    c0, c1 = (dIdx * fx) * invz, (dIdy * fy) * invz
    c2 = -(c0 * p[0] + c1 * p[1]) * invz
    d0, d1 = (dDdx * fx) * invz, (dDdy * fy) * invz
    d2 = -(d0 * p[0] + d1 * p[1]) * invz
    J = np.empty((len(tgt), 2, 6))
    J[:, 0, 0] = sl_img * (-p[2] * c1 + p[1] * c2)
    J[:, 0, 1] = sl_img * (p[2] * c0 - p[0] * c2)
    J[:, 0, 2] = sl_img * (-p[1] * c0 + p[0] * c1)
    J[:, 0, 3], J[:, 0, 4], J[:, 0, 5] = sl_img * c0, sl_img * c1, sl_img * c2
    J[:, 1, 0] = sl_dep * ((-p[2] * d1 + p[1] * d2) - p[1])
    J[:, 1, 1] = sl_dep * ((p[2] * d0 - p[0] * d2) + p[0])
    J[:, 1, 2] = sl_dep * (-p[1] * d0 + p[0] * d1)
    J[:, 1, 3], J[:, 1, 4], J[:, 1, 5] = sl_dep * d0, sl_dep * d1, sl_dep * (d2 - 1.0)
    r = np.stack([sl_img * diff_photo, sl_dep * diff_geo], 1)
    return J, r


def sums(J, r, reverse=False):
    """A = sum J^T J, b = sum J^T r, r2, and the sums of the absolute terms (the bound of a different summation order).
    reverse: the same terms summed from the last correspondence to the first (another order, to measure what an order moves)."""
    if reverse:
        J, r = J[::-1], r[::-1]
    JJ = J[:, :, :, None] * J[:, :, None, :]
    Jr = J * r[:, :, None]
    return dict(n=len(J), A=JJ.sum((0, 1)), b=Jr.sum((0, 1)), r2=float((r * r).sum()), A_abs=np.abs(JJ).sum((0, 1)),
                b_abs=np.abs(Jr).sum((0, 1)), r2_abs=float((r * r).sum()))


def update_matrix(x):
    cx, sx, cy, sy, cz, sz = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rz @ Ry @ Rx
    M[:3, 3] = x[3:]
    return M


def information(K, T, D_src, D_tgt, max_depth_diff, stats=None):
    """Step 7 -> G [6,6], and the sum of the absolute terms."""
    cmap = correspondence_map(K, T, D_src, D_tgt, max_depth_diff, stats=stats)
    _, src = pairs_of(cmap)
    x, y, z = source_points(K, D_src, src)
    o, l = np.zeros_like(x), np.ones_like(x)
    rows = np.stack([np.stack([o, z, -y, l, o, o], 1), np.stack([-z, o, x, o, l, o], 1), np.stack([y, -x, o, o, o, l], 1)], 1)
    GG = rows[:, :, :, None] * rows[:, :, None, :]
    return GG.sum((0, 1)), np.abs(GG).sum((0, 1))


def odometry(pyr_src, pyr_tgt, K, odo_init=None, max_depth_diff=0.03, iterations=(20, 10, 5), reverse_sums=False):
    """Steps 4-8 for one pair; pyr_*: lists over levels of [6,h,w].  -> dict(success, T, information, information_abs, scales,
    trace: a list over iterations of dict(level, n, A, b, r2, A_abs, b_abs, r2_abs, x, T, T_in, cond), ties, pixel_margin,
    depth_margin, tol, given, solved).
    pixel_margin and depth_margin are taken over the pair's whole run.  They are also reported apart: `solved` over the
    decisions made under a pose that came out of a solve, `given` over those under the input pose (the normalisation and the
    first iteration), which are a function of the inputs alone.  `ties` counts the decisions under a solved pose.
    reverse_sums: every sum over correspondences runs from the last to the first (what another order of summation moves)."""
    L = len(pyr_src)
    assert len(iterations) == L
    T = np.eye(4) if odo_init is None else np.array(odo_init, f64)
    stats, given, trace = {}, {}, []               # `given`: decisions under the input pose, which no summation order can move
    failed = dict(success=False, T=np.eye(4), information=np.eye(6), information_abs=np.eye(6), scales=None, trace=trace)
    sc = scales(correspondence_map(K, T, pyr_src[0][1], pyr_tgt[0][1], max_depth_diff, stats=given), pyr_src[0][0], pyr_tgt[0][0],
                reverse=reverse_sums)
    if sc is None or not np.isfinite(sc).all():
        return dict(failed, **stats)
    failed["scales"] = sc
    for l in range(L - 1, -1, -1):
        Kl = level_intrinsic(K, l)
        for _ in range(iterations[L - 1 - l]):
            cmap = correspondence_map(Kl, T, pyr_src[l][1], pyr_tgt[l][1], max_depth_diff, stats=stats if trace else given)
            J, r = jacobian_rows(Kl, T, pyr_src[l], pyr_tgt[l], cmap, *sc)
            it = sums(J, r, reverse=reverse_sums)
            it.update(level=l, T_in=T.copy())
            trace.append(it)
            A, b = it["A"], it["b"]
            if not (np.isfinite(A).all() and np.isfinite(b).all() and np.isfinite(it["r2"])) or abs(np.linalg.det(A)) < 1e-6:
                return dict(failed, **stats)
            x = np.linalg.solve(A, -b)
            if not np.isfinite(x).all():
                return dict(failed, **stats)
            T = update_matrix(x) @ T
            it.update(x=x, T=T.copy(), cond=float(np.linalg.cond(A)))
    G, G_abs = information(K, T, pyr_src[0][1], pyr_tgt[0][1], max_depth_diff, stats=stats)
    tol = float(sum(it["cond"] * it["n"] for it in trace) * 2.0 ** -52)
    whole = {k: min(stats.get(k, np.inf), given.get(k, np.inf)) for k in ("pixel_margin", "depth_margin")}
    return dict(success=True, T=T, information=G, information_abs=G_abs, scales=sc, trace=trace, tol=tol, given=given, solved=stats,
                ties=stats.get("ties", 0), **whole)


def pose_error(T, gt):
    """(rotation error in degrees, translation error in metres) of T against gt."""
    d = np.linalg.inv(gt) @ T
    return float(np.degrees(np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1)))), float(np.linalg.norm(d[:3, 3]))


# ---- the fixture ------------------------------------------------------------------------------------------------------------------

H, W = TR.H, TR.W
INTRINSIC = TR.INTRINSIC
FRAMES = 5
OPTIONS_A = dict(max_depth_diff=0.03, min_depth=0.0, max_depth=4.0)          # the defaults
OPTIONS_B = dict(max_depth_diff=0.07, min_depth=0.3, max_depth=3.0)          # make_fragments.py's; used on pairs 0-2


def fixture_pose(k):
    a = 0.02 * k
    P = np.eye(4)
    P[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    P[:3, 3] = [0.012 * k - 0.05, 0.005 * k, -0.1 + 0.004 * k]
    return P


def _push_pose():
    """A pose that pushes source pixels off the image and, at every level, some onto column 0 from fu in (-1, 0)."""
    a = -0.03
    P = np.eye(4)
    P[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    P[:3, 3] = [-0.02, 0.03, 0.0]
    return P


PUSH_POSE = _push_pose()


def projections(K, T, Ds):
    """(fu, fv) of step 4 for every source pixel with a depth (what decides where a pixel lands)."""
    M, k = geometry(K, np.asarray(T, f64))
    v, u = np.nonzero(~np.isnan(Ds))
    ds = Ds[v, u].astype(f64)
    p = [ds * ((M[i, 0] * u + M[i, 1] * v) + M[i, 2]) + k[i] for i in range(3)]
    return p[0] / p[2] + 0.5, p[1] / p[2] + 0.5


def texture(X):
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    return 0.5 + 0.2 * np.sin(7 * x) * np.cos(5 * y) + 0.15 * np.sin(9 * y + 3 * z) + 0.1 * np.cos(11 * x + 2 * z)


@functools.lru_cache(maxsize=None)
def fixture():
    """gray [5,48,64] uint8, depth [5,48,64] uint16 (millimetres), poses [5,4,4] float64 camera-to-world.  Read-only."""
    fx, fy, cx, cy = INTRINSIC
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cam = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones_like(i, float)], -1)
    poses = np.stack([fixture_pose(k) for k in range(FRAMES)])
    gray, depth = [], []
    for P in poses:
        s = TR.raycast(P)
        X = (cam * s[..., None]) @ P[:3, :3].T + P[:3, 3]
        gray.append(np.round(255 * np.clip(texture(X), 0, 1)).astype(np.uint8))
        depth.append(np.round(1000.0 * s).astype(np.uint16))
    out = np.stack(gray), np.stack(depth), poses
    for a in out:
        a.setflags(write=False)
    return out


def ground_truth(s, t):
    poses = fixture()[2]
    return np.linalg.inv(poses[t]) @ poses[s]


def rgb_of(gray):
    """A colour image whose luma differs from channel to channel (the weights matter)."""
    g = np.asarray(gray).astype(np.int64)
    return np.stack([g, (g * 7 + 13) % 256, 255 - g], -1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def fixture_pyramid(min_depth=0.0, max_depth=4.0, crop=False):
    gray, depth, _ = fixture()
    if crop:
        gray, depth = gray[:, :47, :61], depth[:, :47, :61]
    return pyramid(gray, depth, min_depth=min_depth, max_depth=max_depth)


@functools.lru_cache(maxsize=None)
def fixture_odometry(s, t, init=None, options="A", reverse_sums=False):
    """The restatement's run of pair (s, t); init: None (identity) or a pair (a, b) whose ground truth is odo_init."""
    o = OPTIONS_A if options == "A" else OPTIONS_B
    pyr = fixture_pyramid(o["min_depth"], o["max_depth"])
    return odometry([p[s] for p in pyr], [p[t] for p in pyr], INTRINSIC, None if init is None else ground_truth(*init),
                    max_depth_diff=o["max_depth_diff"], reverse_sums=reverse_sums)
