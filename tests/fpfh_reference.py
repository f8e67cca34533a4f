"""Float64 numpy restatement of the descriptor contract (gmf_amd/features.py, csrc/pointcloud_kernels.hip): the radius-bounded
kNN search, open3d's normals (cumulant covariance + FastEigen3x3), SPFH / FPFH and the two voxel grids.  The GPU tests hold the
kernels to it; the host tests check it against numpy.linalg and geometric invariants.  scipy's cKDTree only proposes candidates;
membership and order come from the contract's own d^2 and (d^2, row) key."""
import numpy as np
from scipy.spatial import cKDTree

TWO_THIRDS_PI = 2.09439510239319549


def _segments(offsets, n):
    off = [0, n] if offsets is None else [int(o) for o in offsets]
    return list(zip(off[:-1], off[1:]))


def d2_exact(P, i, j):
    """(dx dx + dy dy) + dz dz in fp64 from fp32 coordinates, dx = p_j - p_i (no contraction: numpy never fuses)."""
    P64 = P.astype(np.float64)
    dx = P64[j, 0] - P64[i, 0]
    dy = P64[j, 1] - P64[i, 1]
    dz = P64[j, 2] - P64[i, 2]
    return dx * dx + dy * dy + dz * dz


def radius_knn(points, offsets, radius, max_nn):
    """-> idx [N, max_nn] int32 (row within the cloud, -1 padding), d2 [N, max_nn] float64 (0 padding), count [N] int32.
    Inside: d^2 < radius^2.  Order: (d^2, row)."""
    P = np.ascontiguousarray(points, np.float32)
    n = len(P)
    r2 = float(radius) * float(radius)
    idx = np.full((n, max_nn), -1, np.int32)
    d2o = np.zeros((n, max_nn), np.float64)
    cnt = np.zeros(n, np.int32)
    for lo, hi in _segments(offsets, n):
        Q = P[lo:hi]
        tree = cKDTree(Q.astype(np.float64))
        lists = tree.query_ball_point(Q.astype(np.float64), float(radius) * (1 + 1e-6) + 1e-12)
        lens = np.array([len(l) for l in lists])
        qi = np.repeat(np.arange(len(Q)), lens)
        cj = np.concatenate([np.asarray(l, np.int64) for l in lists]) if lens.sum() else np.zeros(0, np.int64)
        d = d2_exact(Q, qi, cj)
        keep = d < r2
        qi, cj, d = qi[keep], cj[keep], d[keep]
        o = np.lexsort((cj, d, qi))
        qi, cj, d = qi[o], cj[o], d[o]
        first = np.searchsorted(qi, np.arange(len(Q)))
        rank = np.arange(len(qi)) - first[qi]
        sel = rank < max_nn
        idx[lo + qi[sel], rank[sel]] = cj[sel]
        d2o[lo + qi[sel], rank[sel]] = d[sel]
        cnt[lo:hi] = np.minimum(np.bincount(qi, minlength=len(Q)), max_nn)
    return idx, d2o, cnt


def _global(idx, offsets, n):
    base = np.zeros(n, np.int64)
    for lo, hi in _segments(offsets, n):
        base[lo:hi] = lo
    return np.where(idx >= 0, idx + base[:, None], -1)


# ---------------------------------------------------------------------------------------------------------------------------
# normals
# ---------------------------------------------------------------------------------------------------------------------------

def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _sel(c, a, b):
    return np.where(c[..., None], a, b)


def _eigenvector0(A, e):
    r0 = np.stack([A[:, 0] - e, A[:, 1], A[:, 2]], -1)
    r1 = np.stack([A[:, 1], A[:, 3] - e, A[:, 4]], -1)
    r2 = np.stack([A[:, 2], A[:, 4], A[:, 5] - e], -1)
    c01, c02, c12 = _cross(r0, r1), _cross(r0, r2), _cross(r1, r2)
    d0, d1, d2 = _dot(c01, c01), _dot(c02, c02), _dot(c12, c12)
    imax = np.zeros(len(A), np.int64)
    dmax = d0.copy()
    m1 = d1 > dmax
    imax[m1], dmax[m1] = 1, d1[m1]
    imax[d2 > dmax] = 2
    return np.where((imax == 0)[:, None], c01 / np.sqrt(d0)[:, None],
                    np.where((imax == 1)[:, None], c02 / np.sqrt(d1)[:, None], c12 / np.sqrt(d2)[:, None]))


def _eigenvector1(A, e0, e):
    bx = np.abs(e0[:, 0]) > np.abs(e0[:, 1])
    il_a = 1 / np.sqrt(e0[:, 0] * e0[:, 0] + e0[:, 2] * e0[:, 2])
    il_b = 1 / np.sqrt(e0[:, 1] * e0[:, 1] + e0[:, 2] * e0[:, 2])
    z = np.zeros(len(A))
    U = _sel(bx, np.stack([-e0[:, 2] * il_a, z, e0[:, 0] * il_a], -1), np.stack([z, e0[:, 2] * il_b, -e0[:, 1] * il_b], -1))
    V = _cross(e0, U)

    def mul(X):
        return np.stack([A[:, 0] * X[:, 0] + A[:, 1] * X[:, 1] + A[:, 2] * X[:, 2],
                         A[:, 1] * X[:, 0] + A[:, 3] * X[:, 1] + A[:, 4] * X[:, 2],
                         A[:, 2] * X[:, 0] + A[:, 4] * X[:, 1] + A[:, 5] * X[:, 2]], -1)
    AU, AV = mul(U), mul(V)
    m00 = _dot(U, AU) - e
    m01 = _dot(U, AV)
    m11 = _dot(V, AV) - e
    a00, a01, a11 = np.abs(m00), np.abs(m01), np.abs(m11)
    # branch a00 >= a11
    p_a = np.maximum(a00, a01) > 0
    q1 = a00 >= a01
    x01 = m01 / m00
    x00 = 1 / np.sqrt(1 + x01 * x01)
    x01 = x01 * x00
    y00 = m00 / m01
    y01 = 1 / np.sqrt(1 + y00 * y00)
    y00 = y00 * y01
    ma01 = np.where(q1, x01, y01)
    ma00 = np.where(q1, x00, y00)
    res_a = ma01[:, None] * U - ma00[:, None] * V
    # branch a00 < a11
    p_b = np.maximum(a11, a01) > 0
    q2 = a11 >= a01
    x01b = m01 / m11
    x11 = 1 / np.sqrt(1 + x01b * x01b)
    x01b = x01b * x11
    y11 = m11 / m01
    y01b = 1 / np.sqrt(1 + y11 * y11)
    y11 = y11 * y01b
    mb11 = np.where(q2, x11, y11)
    mb01 = np.where(q2, x01b, y01b)
    res_b = mb11[:, None] * U - mb01[:, None] * V
    return _sel(a00 >= a11, _sel(p_a, res_a, U), _sel(p_b, res_b, U))


def fast_eigen3x3(A):
    """open3d's FastEigen3x3 (Eberly's robust solver), vectorised: A [M,6] = a00 a01 a02 a11 a12 a22 (fp64) -> the
    eigenvector of the smallest eigenvalue [M,3] (zero for a zero matrix), with the sign the algorithm yields."""
    A = np.asarray(A, np.float64).copy()
    with np.errstate(all="ignore"):
        full = A[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]
        mc = full.max(1)
        zero = mc == 0
        As = A / np.where(zero, 1.0, mc)[:, None]
        norm = As[:, 1] * As[:, 1] + As[:, 2] * As[:, 2] + As[:, 4] * As[:, 4]
        q = (As[:, 0] + As[:, 3] + As[:, 5]) / 3
        b00, b11, b22 = As[:, 0] - q, As[:, 3] - q, As[:, 5] - q
        p = np.sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * 2) / 6)
        c00 = b11 * b22 - As[:, 4] * As[:, 4]
        c01 = As[:, 1] * b22 - As[:, 4] * As[:, 2]
        c02 = As[:, 1] * As[:, 4] - b11 * As[:, 2]
        det = (b00 * c00 - As[:, 1] * c01 + As[:, 2] * c02) / (p * p * p)
        hd = np.minimum(np.maximum(det * 0.5, -1.0), 1.0)
        angle = np.arccos(hd) / 3.0
        beta2 = np.cos(angle) * 2
        beta0 = np.cos(angle + TWO_THIRDS_PI) * 2
        beta1 = -(beta0 + beta2)
        e0, e1, e2 = q + p * beta0, q + p * beta1, q + p * beta2
        pos = hd >= 0
        ea = np.where(pos, e2, e0)
        first = _eigenvector0(As, ea)
        cond_a = np.where(pos, (e2 < e0) & (e2 < e1), (e0 < e1) & (e0 < e2))
        v1 = _eigenvector1(As, first, e1)
        cond_1 = (e1 < e0) & (e1 < e2)
        third = _sel(pos, _cross(v1, first), _cross(first, v1))
        off_diag = _sel(cond_a, first, _sel(cond_1, v1, third))
        Ar = As * np.where(zero, 1.0, mc)[:, None]
        ex = (Ar[:, 0] < Ar[:, 3]) & (Ar[:, 0] < Ar[:, 5])
        ey = ~ex & (Ar[:, 3] < Ar[:, 0]) & (Ar[:, 3] < Ar[:, 5])
        diag = np.zeros((len(A), 3))
        diag[ex, 0] = 1
        diag[ey, 1] = 1
        diag[~ex & ~ey, 2] = 1
        out = _sel(norm > 0, off_diag, diag)
        out[zero] = 0
    return out


def covariances(points, offsets, idx, count):
    """open3d's cumulant covariance over each row's neighbour list, in list order: -> A [N,6] (a00 a01 a02 a11 a12 a22)."""
    P = np.asarray(points, np.float32).astype(np.float64)
    n = len(P)
    g = _global(idx, offsets, n)
    cu = np.zeros((n, 9))
    for t in range(idx.shape[1]):
        v = t < count
        j = np.where(v, g[:, t], 0)
        x, y, z = (np.where(v, P[j, k], 0.0) for k in range(3))
        for k, val in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            cu[:, k] = cu[:, k] + np.where(v, val, 0.0)
    cu = cu / np.maximum(count, 1)[:, None].astype(np.float64)
    return np.stack([cu[:, 3] - cu[:, 0] * cu[:, 0], cu[:, 4] - cu[:, 0] * cu[:, 1], cu[:, 5] - cu[:, 0] * cu[:, 2],
                     cu[:, 6] - cu[:, 1] * cu[:, 1], cu[:, 7] - cu[:, 1] * cu[:, 2], cu[:, 8] - cu[:, 2] * cu[:, 2]], -1)


def estimate_normals(points, offsets, radius, max_nn=30, lists=None):
    """-> normals [N,3] float64, covariance A [N,6], count [N]."""
    idx, _, count = lists if lists is not None else radius_knn(points, offsets, radius, max_nn)
    A = covariances(points, offsets, idx, count)
    n = fast_eigen3x3(A)
    n[(n * n).sum(1) == 0] = (0, 0, 1)
    n[count < 3] = (0, 0, 1)
    return n, A, count


def sym(A):
    return np.stack([A[:, [0, 1, 2]], A[:, [1, 3, 4]], A[:, [2, 4, 5]]], 1)


# ---------------------------------------------------------------------------------------------------------------------------
# FPFH
# ---------------------------------------------------------------------------------------------------------------------------

def pair_features(p1, n1, p2, n2):
    """open3d's ComputePairFeatures, vectorised, fp64 -> (phi, alpha, theta) [M,3] and a flag [M]: a swap decision within
    1e-12 of a tie."""
    with np.errstate(all="ignore"):
        dp = p2 - p1
        d = np.sqrt(dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1] + dp[:, 2] * dp[:, 2])
        a1 = _dot(n1, dp) / d
        a2 = _dot(n2, dp) / d
        c1, c2 = np.arccos(np.abs(a1)), np.arccos(np.abs(a2))
        swap = c1 > c2
        tie = np.abs(c1 - c2) < 1e-12
        ns = _sel(swap, n2, n1)
        nt = _sel(swap, n1, n2)
        dp = _sel(swap, -dp, dp)
        f2 = np.where(swap, -a2, a1)
        v = _cross(dp, ns)
        vn = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        v = v / vn[:, None]
        w = _cross(ns, v)
        f1 = _dot(v, nt)
        f0 = np.arctan2(_dot(w, nt), _dot(ns, nt))
        zero = (d == 0) | (vn == 0)
        f = np.stack([f0, f1, f2], -1)
        f[zero] = 0
    return f, tie & ~zero


def _bins(f):
    """the three bins of each pair feature and the distance of the scaled value to its nearest bin edge."""
    with np.errstate(invalid="ignore"):
        x = np.stack([11 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11 * (f[:, 1] + 1.0) * 0.5, 11 * (f[:, 2] + 1.0) * 0.5], -1)
        b = np.floor(x)
        b = np.where(np.isnan(b), 0, np.clip(b, 0, 10)).astype(np.int64)
        edge = np.abs(x - np.round(x))
        edge = np.where((x < 0.5) | (x > 10.5) | np.isnan(x), np.inf, edge)      # the clamped ends have no neighbour bin
    return b, edge


def spfh(points, normals, offsets, idx, count, edge_tol=1e-9):
    """SPFH [N,33] fp64 (each bin: pairs in the bin x 100 / (count - 1)) and, per row, the number of its pairs within
    `edge_tol` of a bin edge or of a swap tie."""
    P = np.asarray(points, np.float32).astype(np.float64)
    Nn = np.asarray(normals, np.float32).astype(np.float64)
    n = len(P)
    g = _global(idx, offsets, n)
    T = idx.shape[1]
    qi = np.repeat(np.arange(n), T)
    cj = g.reshape(-1)
    t = np.tile(np.arange(T), n)
    v = (t < np.repeat(count, T)) & (cj != qi) & (np.repeat(count, T) > 1)
    qi, cj = qi[v], cj[v]
    f, tie = pair_features(P[qi], Nn[qi], P[cj], Nn[cj])
    b, edge = _bins(f)
    H = np.zeros((n, 33))
    for k in range(3):
        np.add.at(H, (qi, 11 * k + b[:, k]), 1)
    inc = np.where(count > 1, 100.0 / np.maximum(count - 1, 1), 0.0)
    flagged = np.bincount(qi, weights=((edge < edge_tol).any(1) | tie).astype(np.float64), minlength=n)
    return H * inc[:, None], flagged


def fpfh(points, normals, offsets, radius, max_nn=100, lists=None, edge_tol=1e-9):
    """-> FPFH [N,33] fp64 and a per-row bound of what bin-edge / tie pairs may move (0: the row has none)."""
    idx, d2, count = lists if lists is not None else radius_knn(points, offsets, radius, max_nn)
    n = len(points)
    S, flagged = spfh(points, normals, offsets, idx, count, edge_tol)
    g = _global(idx, offsets, n)
    inc = np.where(count > 1, 100.0 / np.maximum(count - 1, 1), 0.0)
    acc = np.zeros((n, 33))
    move = flagged * inc
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(idx.shape[1]):
            j = np.where(g[:, t] >= 0, g[:, t], 0)
            v = (t < count) & (j != np.arange(n)) & (d2[:, t] != 0)
            acc = acc + np.where(v[:, None], S[j] / np.where(v, d2[:, t], 1.0)[:, None], 0.0)
            move = move + np.where(v, flagged[j] * inc[j] / np.where(v, d2[:, t], 1.0), 0.0)
    out = np.zeros((n, 33))
    scale_max = np.zeros(n)
    for blk in range(3):
        s = acc[:, 11 * blk].copy()
        for u in range(1, 11):
            s = s + acc[:, 11 * blk + u]
        sc = np.where(s != 0, 100.0 / np.where(s != 0, s, 1.0), 0.0)
        out[:, 11 * blk:11 * blk + 11] = acc[:, 11 * blk:11 * blk + 11] * sc[:, None] + S[:, 11 * blk:11 * blk + 11]
        scale_max = np.maximum(scale_max, sc)
    out[count <= 1] = 0
    # a moved neighbour pair changes one block's pre-normalisation mass by `move`: at most 2 move scale per bin after it
    bound = np.where(flagged > 0, 2 * inc, 0.0) + 2 * (move - flagged * inc) * scale_max
    return out, bound


# ---------------------------------------------------------------------------------------------------------------------------
# voxel grids
# ---------------------------------------------------------------------------------------------------------------------------

def voxel_down_sample(points, offsets, voxel):
    """-> (means [M,3] float32 in first-occurrence order per cloud, offsets_down [B+1])."""
    P = np.asarray(points, np.float32)
    outs, off = [], [0]
    for lo, hi in _segments(offsets, len(P)):
        p64 = P[lo:hi].astype(np.float64)
        origin = P[lo:hi].min(0).astype(np.float64) - voxel * 0.5
        key = np.floor((p64 - origin) / voxel).astype(np.int64)
        _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
        rank = np.empty(len(first), np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(len(first))
        vid = rank[inv]
        s = np.zeros((len(first), 3))
        np.add.at(s, vid, p64)                 # sequential: ascending row order within each voxel
        outs.append((s / np.bincount(vid)[:, None]).astype(np.float32))
        off.append(off[-1] + len(first))
    return np.concatenate(outs), np.asarray(off)


def voxel_select(points, offsets, voxel):
    """-> (the smallest row within its cloud of each voxel floor(p / voxel), ascending per cloud; offsets_down)."""
    P = np.asarray(points, np.float32)
    outs, off = [], [0]
    for lo, hi in _segments(offsets, len(P)):
        key = np.floor(P[lo:hi].astype(np.float64) / voxel).astype(np.int64)
        _, first = np.unique(key, axis=0, return_index=True)
        outs.append(np.sort(first))
        off.append(off[-1] + len(first))
    return np.concatenate(outs), np.asarray(off)


def fpfh_descriptors(points, voxel, voxelize="mean", normals_fn=None):
    """The recipe: voxel grid -> normals (2v, 30) -> FPFH (5v, 100) -> nan_to_num -> f / (|f| + 1e-6), one cloud."""
    if voxelize == "mean":
        xyz, _ = voxel_down_sample(points, None, voxel)
    else:
        xyz = np.asarray(points, np.float32)[voxel_select(points, None, voxel)[0]]
    nrm = normals_fn(xyz) if normals_fn else estimate_normals(xyz, None, 2 * voxel, 30)[0].astype(np.float32)
    f, _ = fpfh(xyz, nrm, None, 5 * voxel, 100)
    f = np.nan_to_num(f)
    return xyz, f / (np.linalg.norm(f, axis=1, keepdims=True) + 1e-6)
