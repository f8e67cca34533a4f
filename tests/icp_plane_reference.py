"""Point-to-plane ICP restated in NumPy float64, operation for operation (gmf_amd.icp_point_to_plane_batched, DESIGN.md section
4e; open3d 0.9 TransformationEstimationPointToPlane inside registration_icp's loop), and the scene its tests run on.

One pair: source rows s_i, target rows q_j with normals n_j (used as given), init, tau.
  p_i = T s_i in float64, rounded once to fp32;  C = the rows whose exact nearest target has d^2 < tau^2 (cKDTree);
  fitness = |C| / Ns, inlier_rmse = sqrt(sum_C d^2 / |C|)  (Euclidean, whatever the estimator);
  evaluate at init, then up to max_iteration times T <- dT T, evaluate, stop when |d fitness| < rf and |d rmse| < rr.
dT, all in float64 from the fp32 p, q, n: over the rows of C with a finite normal r = (p - q) . n, J = [p x n ; n],
A = sum J J^T, b = sum J r;  A x = -b by LDL^T without pivoting (`ldlt_solve`: a pivot d_k is accepted when it is finite and
d_k > 2^-40 A_kk);  dT = [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)] (`vector6_to_matrix`).  A rejected pivot or an empty C: dT = I."""
import math

import numpy as np
from scipy.spatial import cKDTree

PIVOT_RATIO = 2.0 ** -40
TAU = 0.07
CASES = {"clean": (3000, 2000, 0.0), "noisy": (3000, 2000, 0.002), "small": (600, 257, 0.001)}     # Nt, Ns, noise


def transform_rows(T, S):
    """T s for fp32 rows S under the float64 [R | t] of T, innermost term first as the kernel's fma chain, rounded once to fp32."""
    S = np.asarray(S, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64)
    cols = [T[r, 0] * S[:, 0] + (T[r, 1] * S[:, 1] + (T[r, 2] * S[:, 2] + T[r, 3])) for r in range(3)]
    return np.stack(cols, 1).astype(np.float32)


def normal_equations(P, Q, N):
    """A [6,6] and b [6] over matched fp32 rows: p (transformed source), q (target), n (its normal); non-finite normals skipped."""
    P, Q, N = (np.asarray(x, np.float32).astype(np.float64) for x in (P, Q, N))
    keep = np.isfinite(N).all(1)
    P, Q, N = P[keep], Q[keep], N[keep]
    J = np.concatenate([np.cross(P, N), N], 1)
    r = ((P - Q) * N).sum(1)
    return J.T @ J, J.T @ r


def ldlt_solve(A, b):
    """x with A x = -b by LDL^T without pivoting in the contract's order, or None when a pivot is rejected."""
    A = np.asarray(A, np.float64)
    L, D = np.zeros((6, 6)), np.zeros(6)
    ok = True
    with np.errstate(all="ignore"):
        for c in range(6):
            d = A[c, c]
            for m in range(c):
                d = d - (L[c, m] * L[c, m]) * D[m]
            ok = ok and bool(np.isfinite(d)) and bool(d > PIVOT_RATIO * A[c, c])
            D[c] = d
            for i in range(c + 1, 6):
                v = A[i, c]
                for m in range(c):
                    v = v - (L[i, m] * L[c, m]) * D[m]
                L[i, c] = v / d
        if not ok:
            return None
        x = np.zeros(6)
        for i in range(6):
            y = -b[i]
            for m in range(i):
                y = y - L[i, m] * x[m]
            x[i] = y
        x = x / D
        for i in range(5, -1, -1):
            for m in range(i + 1, 6):
                x[i] = x[i] - L[m, i] * x[m]
    return x


def vector6_to_matrix(x):
    """open3d's TransformVector6dToMatrix4d: [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)]."""
    sx, cx, sy, cy, sz, cz = math.sin(x[0]), math.cos(x[0]), math.sin(x[1]), math.cos(x[1]), math.sin(x[2]), math.cos(x[2])
    T = np.eye(4)
    T[:3, :3] = [[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                 [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                 [-sy, cy * sx, cy * cx]]
    T[:3, 3] = x[3:]
    return T


def icp_plane_np(S, Q, N, T0, tau, max_iteration=30, rf=1e-6, rr=1e-6):
    """-> T [4,4] float64, fitness, inlier_rmse, passes, nn [Ns] (the matched target row, -1 outside C)."""
    S, Q, N = (np.asarray(x, np.float32) for x in (S, Q, N))
    tree = cKDTree(Q.astype(np.float64))

    def evaluate(T):
        P = transform_rows(T, S)
        d, j = tree.query(P.astype(np.float64))
        d2 = d * d
        c = d2 < tau * tau
        k = int(c.sum())
        return P, j, c, k / len(S), math.sqrt(d2[c].sum() / k) if k else 0.0

    T = np.asarray(T0, np.float64).copy()
    P, j, c, fit, rm = evaluate(T)
    it = 0
    for i in range(max_iteration):
        x = None
        if c.any():
            A, b = normal_equations(P[c], Q[j[c]], N[j[c]])
            x = ldlt_solve(A, b)
        if x is not None:
            T = vector6_to_matrix(x) @ T
        f0, r0 = fit, rm
        P, j, c, fit, rm = evaluate(T)
        it = i + 1
        if abs(fit - f0) < rf and abs(rm - r0) < rr:
            break
    return T, fit, rm, it, np.where(c, j, -1)


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def corner_surface(r, n):
    """n noiseless rows of the scene and their outward unit normals: a quarter on each of the planes x = 0, y = 0, z = 0
    (uniform in [0, 2]^2, normal = the axis), the rest on the octant facing the corner of the sphere of radius 0.6 about
    (1, 1, 1), with the radial normal."""
    X, Nn = np.zeros((n, 3)), np.zeros((n, 3))
    q = n // 4
    for a in range(3):
        rows = slice(a * q, (a + 1) * q)
        X[rows] = r.uniform(0, 2, (q, 3))
        X[rows, a] = 0.0
        Nn[rows, a] = 1.0
    v = -np.abs(r.normal(size=(n - 3 * q, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    X[3 * q:] = 1.0 + 0.6 * v
    Nn[3 * q:] = v
    return X, Nn


def corner(seed, Nt, Ns, noise):
    """-> source [Ns,3], target [Nt,3], target normals [Nt,3] (fp32) and the motion Tg [4,4] (float64) that ICP from the identity
    should find.  Target: `corner_surface` plus Gaussian noise of `noise` on the points only, every normal with a random sign.
    Source: a random subset of the noiseless surface moved by the inverse of Tg, a 3 degree / 0.04 m motion."""
    r = np.random.default_rng([seed, 0xc0a7e5])
    X, Nn = corner_surface(r, Nt)
    tgt = X + r.normal(0, noise, X.shape) if noise else X.copy()
    Nn = Nn * r.choice([-1.0, 1.0], (Nt, 1))
    Tg = np.eye(4)
    Tg[:3, :3] = rotation(r.normal(size=3), 3.0)
    v = r.normal(size=3)
    Tg[:3, 3] = 0.04 * v / np.linalg.norm(v)
    sub = X[r.permutation(Nt)[:Ns]]
    src = (sub - Tg[:3, 3]) @ Tg[:3, :3]                              # R^T (x - t)
    return src.astype(np.float32), tgt.astype(np.float32), Nn.astype(np.float32), Tg


def rotation_error_deg(T, Tg):
    cos = (np.trace(np.asarray(T, np.float64)[:3, :3].T @ Tg[:3, :3]) - 1) / 2
    return math.degrees(math.acos(min(1.0, max(-1.0, cos))))


def one_ulp(x, r):
    """Every fp32 entry moved one ulp up or down at random."""
    x = np.asarray(x, np.float32)
    return np.where(r.random(x.shape) < 0.5, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))).astype(np.float32)
