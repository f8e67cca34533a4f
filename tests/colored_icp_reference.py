"""Coloured ICP restated in NumPy float64 (gmf_amd.color_gradients_batched, gmf_amd.icp_colored_batched,
gmf_amd.voxel_down_sample_colored_batched; open3d 0.9 ColoredICP.cpp: InitializePointCloudForColoredICP and
TransformationEstimationForColoredICP inside registration_icp's loop), and the scenes its tests run on.

Intensity of a colour (r, g, b) in fp32: fp32(((r + g) + b) / 3) evaluated in float64.

Gradients of one cloud: rows v_i (fp32) with normals n_i (used as given) and intensities I_i, radius, max_nn.
  The list of row i: the rows with d^2 < radius^2, d^2 = (dx dx + dy dy) + dz dz in float64 from the fp32 coordinates, itself
  included, the max_nn smallest by the key (d^2, row), in that order.  Fewer than 4 entries: g = 0.  Otherwise the first entry
  is skipped and over the others, in list order: e = v_a - v, d = e - (e . n) n, A = sum d d^T + (count - 1)^2 n n^T,
  b = sum d (I_a - I); A g = b by 3 x 3 LDL^T without pivoting (`ldlt3_solve`: a pivot d_k is accepted when it is finite and
  d_k > 2^-40 A_kk).  A rejected pivot or a non-finite component: g = 0.

One pair: the loop, C, fitness and inlier_rmse of tests/icp_plane_reference.py.  dT, all in float64 from the fp32 p, q, n, g, I:
over the rows of C whose normal, gradient and two intensities are finite,
  r_G = (p - q) . n, J_G = [p x n ; n];  u = (p - q) - r_G n, r_I = I_s - (g . u + I_t), m = -(g - (g . n) n), J_I = [p x m ; m];
  A = sum lambda J_G J_G^T + (1 - lambda) J_I J_I^T, b = sum lambda J_G r_G + (1 - lambda) J_I r_I (each term scaled by the
  square root of its weight);  A x = -b by `ldlt_solve`;  dT = `vector6_to_matrix(x)`.  A rejected pivot or an empty C: dT = I."""
import math

import numpy as np
from scipy.spatial import cKDTree

from icp_plane_reference import PIVOT_RATIO, corner, corner_surface, ldlt_solve, rotation, transform_rows, vector6_to_matrix  # noqa: F401

TAU = 0.07
LAMBDA = 0.968
MAX_NN = 30
PLANE_CASES = {"clean": (3000, 1500, 0.0), "noisy": (3000, 1500, 0.001), "small": (800, 257, 0.0005)}     # Nt, Ns, noise
CORNER_CASE = (3000, 1500, 0.001)


# ---- colours ----------------------------------------------------------------------------------------------------------------------------

def field(X):
    """A smooth intensity in 0.15 .. 0.85 at the rows of X (float64)."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return 0.5 + 0.2 * np.sin(3 * x + 0.5) * np.cos(2 * y) + 0.15 * np.sin(2.5 * z + 1.7 * x - 1.1 * y)


def field_colors(X):
    """fp32 colours of three unequal channels whose mean is the field."""
    f = field(np.asarray(X, np.float64))
    return np.stack([f + 0.10, f - 0.04, f - 0.06], 1).astype(np.float32)


def intensity(colors):
    c = np.asarray(colors, np.float32).astype(np.float64)
    return (((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0).astype(np.float32)


# ---- gradients --------------------------------------------------------------------------------------------------------------------------

def neighbour_lists(P, radius, max_nn):
    """The lists of the radius search over one cloud of fp32 rows: for every row the rows with d^2 < radius^2, the max_nn
    smallest by (d^2, row)."""
    P = np.asarray(P, np.float32).astype(np.float64)
    tree = cKDTree(P)
    out = []
    for i, cand in enumerate(tree.query_ball_point(P, radius * (1 + 1e-9) + 1e-12)):
        cand = np.asarray(sorted(cand), np.int64)
        d = P[cand] - P[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = d2 < radius * radius
        cand, d2 = cand[keep], d2[keep]
        order = np.lexsort((cand, d2))[:max_nn]
        out.append(cand[order])
    return out


def ldlt3_solve(A, b):
    """g with A g = b by 3 x 3 LDL^T without pivoting in the contract's order, or None when a pivot is rejected or a component
    is not finite."""
    with np.errstate(all="ignore"):
        d0 = A[0, 0]
        ok = bool(np.isfinite(d0)) and bool(d0 > PIVOT_RATIO * A[0, 0])
        l10, l20 = A[1, 0] / d0, A[2, 0] / d0
        d1 = A[1, 1] - (l10 * l10) * d0
        ok = ok and bool(np.isfinite(d1)) and bool(d1 > PIVOT_RATIO * A[1, 1])
        l21 = (A[2, 1] - (l20 * l10) * d0) / d1
        d2 = (A[2, 2] - (l20 * l20) * d0) - (l21 * l21) * d1
        ok = ok and bool(np.isfinite(d2)) and bool(d2 > PIVOT_RATIO * A[2, 2])
        if not ok:
            return None
        y0 = b[0]
        y1 = b[1] - l10 * y0
        y2 = (b[2] - l20 * y0) - l21 * y1
        x2 = y2 / d2
        x1 = y1 / d1 - l21 * x2
        x0 = (y0 / d0 - l10 * x1) - l20 * x2
    g = np.array([x0, x1, x2])
    return g if np.isfinite(g).all() else None


def gradient_row(v, n, I, Va, Ia):
    """The gradient of one row from its list WITHOUT the skipped first entry: neighbours Va [k,3] with intensities Ia [k];
    count = k + 1.  None: rejected."""
    e = Va - v
    d = e - (e @ n)[:, None] * n
    A = d.T @ d + float(len(Va)) ** 2 * np.outer(n, n)
    b = d.T @ (Ia - I)
    return ldlt3_solve(A, b)


def color_gradients_np(P, N, I, radius, max_nn=MAX_NN):
    """-> g [n,3] float64 and zeroed [n] bool (fewer than 4 list entries, or rejected)."""
    P64, N64, I64 = (np.asarray(x, np.float32).astype(np.float64) for x in (P, N, I))
    g, zeroed = np.zeros((len(P64), 3)), np.ones(len(P64), bool)
    for i, row in enumerate(neighbour_lists(P, radius, max_nn)):
        if len(row) < 4:
            continue
        a = row[1:]
        x = gradient_row(P64[i], N64[i], I64[i], P64[a], I64[a])
        if x is not None:
            g[i], zeroed[i] = x, False
    return g, zeroed


# ---- the step and the loop --------------------------------------------------------------------------------------------------------------

def normal_equations(P, Q, N, G, Is, It, lam=LAMBDA):
    """A [6,6] and b [6] over matched fp32 rows; rows with a non-finite normal, gradient or intensity skipped."""
    P, Q, N, G, Is, It = (np.asarray(x, np.float32).astype(np.float64) for x in (P, Q, N, G, Is, It))
    keep = np.isfinite(N).all(1) & np.isfinite(G).all(1) & np.isfinite(Is) & np.isfinite(It)
    P, Q, N, G, Is, It = P[keep], Q[keep], N[keep], G[keep], Is[keep], It[keep]
    sg, si = math.sqrt(lam), math.sqrt(1.0 - lam)
    E = P - Q
    rG = (E * N).sum(1)
    JG = np.concatenate([np.cross(P, N), N], 1) * sg
    U = E - rG[:, None] * N
    rI = (Is - ((G * U).sum(1) + It)) * si
    M = (G * N).sum(1)[:, None] * N - G
    JI = np.concatenate([np.cross(P, M), M], 1) * si
    return JG.T @ JG + JI.T @ JI, JG.T @ (rG * sg) + JI.T @ rI


def icp_colored_np(S, Q, Is, It, N, G, T0, tau, lam=LAMBDA, max_iteration=30, rf=1e-6, rr=1e-6):
    """-> T [4,4] float64, fitness, inlier_rmse, passes, nn [Ns] (the matched target row, -1 outside C), rejected (passes whose
    pivots were rejected)."""
    S, Q, N, G, Is, It = (np.asarray(x, np.float32) for x in (S, Q, N, G, Is, It))
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
    it = rejected = 0
    for i in range(max_iteration):
        x = None
        if c.any():
            A, b = normal_equations(P[c], Q[j[c]], N[j[c]], G[j[c]], Is[c], It[j[c]], lam)
            x = ldlt_solve(A, b)
            rejected += x is None
        if x is not None:
            T = vector6_to_matrix(x) @ T
        f0, r0 = fit, rm
        P, j, c, fit, rm = evaluate(T)
        it = i + 1
        if abs(fit - f0) < rf and abs(rm - r0) < rr:
            break
    return T, fit, rm, it, np.where(c, j, -1), rejected


# ---- voxel grid -------------------------------------------------------------------------------------------------------------------------

def voxel_means_np(P, C, voxel):
    """open3d voxel_down_sample of one cloud with colours: origin min - voxel / 2, voxels in first-occurrence order, float64 means
    in ascending row order.  -> points [M,3], colours [M,3] (float64)."""
    P32 = np.asarray(P, np.float32)
    P64, C64 = P32.astype(np.float64), np.asarray(C, np.float32).astype(np.float64)
    origin = P32.min(0).astype(np.float64) - voxel * 0.5
    cell = np.floor((P64 - origin) / voxel).astype(np.int64)
    _, first, inv = np.unique(cell, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    vid = rank[inv.reshape(-1)]
    sp, sc, cnt = np.zeros((len(first), 3)), np.zeros((len(first), 3)), np.zeros(len(first))
    for i in range(len(P64)):                               # ascending rows
        sp[vid[i]] += P64[i]
        sc[vid[i]] += C64[i]
        cnt[vid[i]] += 1
    return sp / cnt[:, None], sc / cnt[:, None]


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------

def plane_motion():
    """2 degrees about z and 30 mm in the plane."""
    Tg = np.eye(4)
    Tg[:3, :3] = rotation([0, 0, 1], 2.0)
    Tg[:3, 3] = [0.03 * math.cos(0.7), 0.03 * math.sin(0.7), 0.0]
    return Tg


def textured_plane(seed, Nt, Ns, noise):
    """-> source [Ns,3], target [Nt,3], source colours [Ns,3], target colours [Nt,3], target normals [Nt,3] (fp32) and the
    motion Tg [4,4] (float64) that ICP from the identity should find.  Target: uniform on z = 0 over [0, 2]^2, Gaussian noise of
    `noise` on z only, every normal (0, 0, +-1) with a random sign.  Source: sampled on its own over [0.2, 1.8]^2 and moved by
    the inverse of Tg.  The colours are the field at the noiseless positions."""
    r = np.random.default_rng([seed, 0xc0104ed])
    X = np.zeros((Nt, 3))
    X[:, :2] = r.uniform(0, 2, (Nt, 2))
    tgt = X.copy()
    if noise:
        tgt[:, 2] += r.normal(0, noise, Nt)
    Nn = np.zeros((Nt, 3))
    Nn[:, 2] = r.choice([-1.0, 1.0], Nt)
    Y = np.zeros((Ns, 3))
    Y[:, :2] = r.uniform(0.2, 1.8, (Ns, 2))
    Tg = plane_motion()
    src = (Y - Tg[:3, 3]) @ Tg[:3, :3]                              # R^T (x - t)
    return (src.astype(np.float32), tgt.astype(np.float32), field_colors(Y), field_colors(X), Nn.astype(np.float32), Tg)


def colored_corner(seed, Nt, Ns, noise):
    """The corner scene of the plane tests with the field added: the colours of a target row are the field at its (noisy)
    position, those of a source row the field at its position under Tg."""
    src, tgt, nrm, Tg = corner(seed, Nt, Ns, noise)
    world = src.astype(np.float64) @ Tg[:3, :3].T + Tg[:3, 3]
    return src, tgt, field_colors(world), field_colors(tgt), nrm, Tg


def rotation_error_deg(T, Tg):
    cos = (np.trace(np.asarray(T, np.float64)[:3, :3].T @ Tg[:3, :3]) - 1) / 2
    return math.degrees(math.acos(min(1.0, max(-1.0, cos))))


def translation_error(T, Tg):
    return float(np.linalg.norm(np.asarray(T, np.float64)[:3, 3] - Tg[:3, 3]))
