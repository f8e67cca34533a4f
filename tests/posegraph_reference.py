"""Float64 NumPy restatement of multiway registration's two device pieces: the information matrix of an
edge and the pose-graph optimiser (Levenberg-Marquardt with a line process per uncertain edge, two passes with the pruning in
between).  It is the yardstick of tests/test_posegraph_host.py and tests/test_gpu_multiway.py; gmf_amd/csrc/posegraph_kernels.hip
follows it operation for operation where an order of operations can be followed (sums per node in edge order, the right-looking
LDL^T, the column-oriented substitutions, the 256-way strided sums with a halving tree), so what is left between the two is the
device's sin / cos / atan2 / sqrt and nothing else.

Decisions where the specification is silent (also listed in DESIGN.md 4m):
  * the inverse of a pose is the rigid one, [R^T | -R^T t];
  * vec(T) = (atan2(R21, R22), atan2(-R20, sqrt(R21^2 + R22^2)), atan2(R10, R00), t);
  * `r < min_residual` is tested at the top of every outer iteration, the first included;
  * an outer iteration counts once entered; a rejected step leaves the poses alone;
  * the reference node's pose is copied, not multiplied by mat(0), so it keeps its bits;
  * when an accepted step flags both min_relative_residual_increment and min_right_term, the reported code is min_right_term;
  * the solve uses L[i][k] = A[i][k] / d_k and A[i][j] -= L[i][k] * (d_k * L[j][k]);
  * the line process of an edge that is masked or pruned is reported as 0;
  * the trace holds (residual, lambda) at the start and after every outer iteration.
"""
import math
from fractions import Fraction

import numpy as np

STOP_MAX_ITERATION, STOP_RIGHT_TERM, STOP_INCREMENT, STOP_RESIDUAL_INCREMENT, STOP_RESIDUAL, STOP_LM_MAX, STOP_PIVOT = range(7)

CRITERIA = dict(max_iteration=100, max_iteration_lm=20, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                min_right_term=1e-6, min_residual=1e-6)


# ---- information matrix -------------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    """fma in fp64: the exact a b + c rounded once (Fraction -> float rounds correctly)."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def transform_rows_f32(T, src):
    """ICP's transformed rows: the fp64 [R | t] times the fp32 row by nested fmas, rounded once to fp32."""
    T = np.asarray(T, np.float64)
    a = np.asarray(src, np.float32).astype(np.float64)
    out = np.empty((len(a), 3), np.float32)
    for i in range(len(a)):
        for r in range(3):
            out[i, r] = np.float32(_fma(T[r, 0], a[i, 0], _fma(T[r, 1], a[i, 1], _fma(T[r, 2], a[i, 2], T[r, 3]))))
    return out


def nn_brute_f32(p, tgt, tau):
    """The exact nearest target row of every (already transformed, fp32) row under ICP's fp32 d^2, ties to the smaller row; -1
    when d^2 >= tau^2.  d^2 = fma(dx, dx, fma(dy, dy, dz dz)) is evaluated in fp64 and rounded per step: the fp64 product of two
    fp32 numbers is exact, so each rounding to fp32 is the fma's."""
    p = np.asarray(p, np.float32)
    q = np.asarray(tgt, np.float32)
    tau2 = np.float32(tau) * np.float32(tau)
    nn = np.full(len(p), -1, np.int64)
    for i in range(len(p)):
        d = (p[i][None, :] - q).astype(np.float32).astype(np.float64)                 # fp32 differences
        zz = (d[:, 2] * d[:, 2]).astype(np.float32).astype(np.float64)
        yz = (d[:, 1] * d[:, 1] + zz).astype(np.float32).astype(np.float64)          # exact product + fp32: one rounding
        d2 = (d[:, 0] * d[:, 0] + yz).astype(np.float32)
        j = int(np.argmin(d2)) if len(q) else -1
        if j >= 0 and d2[j] < tau2:
            nn[i] = j
    return nn


def info_terms(tgt, nn):
    """[K, 6, 6] fp64: G^T G of every matched target row (the device's terms: products and sums rounded one by one)."""
    q = np.asarray(tgt, np.float32)[nn[nn >= 0]].astype(np.float64)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    o, one = np.zeros_like(x), np.ones_like(x)
    rows = [[y * y + z * z, -(x * y), -(x * z), o, -z, y],
            [-(x * y), x * x + z * z, -(y * z), z, o, -x],
            [-(x * z), -(y * z), x * x + y * y, -y, x, o],
            [o, z, -y, one, o, o],
            [-z, o, x, o, one, o],
            [y, -x, o, o, o, one]]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def info_from_nn(tgt, nn):
    """(info [6, 6], bound [6, 6]): the fp64 sum of the terms and the bound K 2^-52 sum |terms| on any order of summation."""
    t = info_terms(tgt, nn)
    K = len(t)
    return t.sum(0), K * 2.0 ** -52 * np.abs(t).sum(0)


# ---- operators ----------------------------------------------------------------------------------------------------------------

def rigid_mul(A, B):
    C = np.zeros((4, 4))
    for i in range(3):
        for j in range(3):
            C[i, j] = A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j]
        C[i, 3] = A[i, 0] * B[0, 3] + A[i, 1] * B[1, 3] + A[i, 2] * B[2, 3] + A[i, 3]
    C[3, 3] = 1.0
    return C


def rigid_inv(A):
    C = np.zeros((4, 4))
    for i in range(3):
        for j in range(3):
            C[i, j] = A[j, i]
        C[i, 3] = -(A[0, i] * A[0, 3] + A[1, i] * A[1, 3] + A[2, i] * A[2, 3])
    C[3, 3] = 1.0
    return C


def lin(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


def mat(v):
    cx, sx, cy, sy, cz, sz = math.cos(v[0]), math.sin(v[0]), math.cos(v[1]), math.sin(v[1]), math.cos(v[2]), math.sin(v[2])
    M = np.eye(4)
    M[0, :3] = [cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx]
    M[1, :3] = [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx]
    M[2, :3] = [-sy, cy * sx, cy * cx]
    M[:3, 3] = v[3:6]
    return M


def vec(T):
    return np.array([math.atan2(T[2, 1], T[2, 2]), math.atan2(-T[2, 0], math.sqrt(T[2, 1] * T[2, 1] + T[2, 2] * T[2, 2])),
                     math.atan2(T[1, 0], T[0, 0]), T[0, 3], T[1, 3], T[2, 3]])


def wg_sum(values):
    """The device's workgroup sum: 256 strided partial sums in order, then a halving tree."""
    part = np.zeros(256)
    for c, v in enumerate(values):
        part[c % 256] += v
    s = 128
    while s > 0:
        part[:s] += part[s:2 * s]
        s //= 2
    return float(part[0])


def quad(Lm, z):
    q = 0.0
    for i in range(6):
        a = 0.0
        for j in range(6):
            a += Lm[i, j] * z[j]
        q += z[i] * a
    return q


def edge_A_zeta(X, Pt, Ps):
    A = rigid_mul(rigid_inv(X), rigid_inv(Pt))
    return A, lin(rigid_mul(A, Ps))


def edge_jacobian(A, Ps):
    """J_s [6, 6]: column i = lin(A G_i P_s)."""
    J = np.zeros((6, 6))
    for i in range(3):
        u, w = (i + 1) % 3, (i + 2) % 3
        GP = np.zeros((3, 4))
        GP[u] = -Ps[w]
        GP[w] = Ps[u]
        M = np.zeros((4, 4))
        for r in range(3):
            for c in range(4):
                M[r, c] = A[r, 0] * GP[0, c] + A[r, 1] * GP[1, c] + A[r, 2] * GP[2, c]
        J[:, i] = lin(M)
        J[3:, 3 + i] = A[:3, i]
    return J


def line_weight(q, p):
    w = p / (p + q)
    return w * w


def edge_share(l, q, uncertain, p):
    if not uncertain:
        return l * q
    d = math.sqrt(l) - 1.0
    return l * q + p * (d * d)


def ldl_solve(A, b):
    """Right-looking LDL^T without pivoting on the lower triangle and the column-oriented substitutions.  None: a pivot was not
    finite or not positive."""
    A = np.array(A, np.float64)
    N = len(A)
    for k in range(N):
        d = A[k, k]
        if not (d > 0.0) or not math.isfinite(d):
            return None
        if k + 1 < N:
            l = A[k + 1:, k] / d
            A[k + 1:, k] = l
            A[k + 1:, k + 1:] -= np.tril(l[:, None] * (d * l)[None, :])
    x = np.array(b, np.float64)
    for j in range(N):
        x[j + 1:] -= A[j + 1:, j] * x[j]
    x = x / np.diag(A)
    for j in range(N - 1, 0, -1):
        x[:j] -= A[j, :j] * x[j]
    return x


class _Graph:
    def __init__(self, src, tgt, X, Lam, unc, p, ref):
        self.src, self.tgt, self.X, self.Lam, self.unc, self.p, self.ref = src, tgt, X, Lam, unc, p, ref

    def linearise(self, P, alive):
        n = len(P)
        H, b = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
        l_all, shares = np.zeros(len(self.src)), []
        for k in alive:
            s, t = self.src[k], self.tgt[k]
            A, z = edge_A_zeta(self.X[k], P[t], P[s])
            q = quad(self.Lam[k], z)
            l = line_weight(q, self.p) if self.unc[k] else 1.0
            l_all[k] = l
            shares.append(edge_share(l, q, self.unc[k], self.p))
            J = edge_jacobian(A, P[s])
            Lm = self.Lam[k]
            LJ, Lz = np.zeros((6, 6)), np.zeros(6)
            for bb in range(6):                                       # sums over bb in increasing order, entry by entry
                LJ = LJ + Lm[:, bb, None] * J[bb, None, :]
                Lz = Lz + Lm[:, bb] * z[bb]
            M, g = np.zeros((6, 6)), np.zeros(6)
            for a in range(6):
                M = M + J[a, :, None] * LJ[a, None, :]
                g = g + J[a, :] * Lz[a]
            M, g = l * M, l * g
            ss, tt = slice(6 * s, 6 * s + 6), slice(6 * t, 6 * t + 6)
            H[ss, ss] += M
            H[tt, tt] += M
            H[ss, tt] -= M
            H[tt, ss] -= M
            b[ss] -= g
            b[tt] += g
        if self.ref >= 0:
            rr = slice(6 * self.ref, 6 * self.ref + 6)
            H[rr, :] = 0.0
            H[:, rr] = 0.0
            H[rr, rr] = np.eye(6)
            b[rr] = 0.0
        return wg_sum(shares), H, b, l_all

    def residual(self, P, alive, l_all):
        out = []
        for k in alive:
            _, z = edge_A_zeta(self.X[k], P[self.tgt[k]], P[self.src[k]])
            out.append(edge_share(l_all[k], quad(self.Lam[k], z), self.unc[k], self.p))
        return wg_sum(out)


def _one_pass(g, P, alive, crit, decisions):
    """-> poses, l, dict(iterations, rejected, stop, residual, trace, solves)."""
    n = len(P)
    P = [np.array(T, np.float64) for T in P]
    r, H, b, l_all = g.linearise(P, alive)
    lam, nu = 1e-5 * max([0.0] + [H[i, i] for i in range(6 * n)]), 2.0
    trace = [(r, lam)]
    iters = rejected = solves = 0
    stop = STOP_RIGHT_TERM if max([0.0] + [abs(v) for v in b]) < crit["min_right_term"] else -1
    eps = crit["min_relative_increment"]
    for _ in range(crit["max_iteration"]):
        if stop >= 0:
            break
        if r < crit["min_residual"]:
            stop = STOP_RESIDUAL
            break
        iters += 1
        lm = 0
        while True:
            delta = ldl_solve(H + lam * np.eye(6 * n), b)
            if delta is None:
                stop = STOP_PIVOT
                break
            solves += 1
            dn2 = wg_sum(delta * delta)
            xs = [vec(T) for T in P]
            xn2 = wg_sum([sum_seq(x * x) for x in xs])
            if math.sqrt(dn2) < eps * (math.sqrt(xn2) + eps):
                stop = STOP_INCREMENT
                break
            trial = [P[v].copy() if v == g.ref else rigid_mul(mat(delta[6 * v:6 * v + 6]), P[v]) for v in range(n)]
            r2 = g.residual(trial, alive, l_all)
            rho = (r - r2) / (wg_sum(delta * (lam * delta + b)) + 1e-3)
            if rho > 0.0:
                decisions.append(1)
                if r - r2 < crit["min_relative_residual_increment"] * r:
                    stop = STOP_RESIDUAL_INCREMENT
                c3 = 2.0 * rho - 1.0
                lam = lam * max(1.0 / 3.0, min(1.0 - c3 * c3 * c3, 2.0 / 3.0))
                nu = 2.0
                P = trial
                r, H, b, l_all = g.linearise(P, alive)
                if max([0.0] + [abs(v) for v in b]) < crit["min_right_term"]:
                    stop = STOP_RIGHT_TERM
                break
            decisions.append(0)
            lam, nu = lam * nu, 2.0 * nu
            rejected += 1
            lm += 1
            if lm >= crit["max_iteration_lm"]:
                stop = STOP_LM_MAX
                break
        trace.append((r, lam))
    if stop < 0:
        stop = STOP_RESIDUAL if r < crit["min_residual"] else STOP_MAX_ITERATION
    return P, l_all, dict(iterations=iters, rejected=rejected, stop=stop, residual=r, trace=trace, solves=solves, edges=len(alive))


def sum_seq(values):
    s = 0.0
    for v in values:
        s += v
    return s


def global_optimization(poses, edge_source, edge_target, edge_transformation, edge_information, edge_uncertain, edge_mask=None,
                        edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=-1, criteria=None):
    """One graph.  -> poses [n, 4, 4], line_process [m], kept [m] bool, stats (a list of the two passes' dicts; "decisions" holds
    the accept (1) / reject (0) sequence of both passes)."""
    crit = dict(CRITERIA, **(criteria or {}))
    m = len(edge_source)
    X = np.asarray(edge_transformation, np.float64).reshape(m, 4, 4)
    Lam = np.asarray(edge_information, np.float64).reshape(m, 6, 6)
    unc = [bool(u) for u in edge_uncertain]
    n = len(poses)
    ref = reference_node if 0 <= reference_node < n else -1
    g = _Graph([int(s) for s in edge_source], [int(t) for t in edge_target], X, Lam, unc, float(preference_loop_closure), ref)
    alive = [k for k in range(m) if edge_mask is None or bool(edge_mask[k])]
    decisions = []
    P, l1, st1 = _one_pass(g, poses, alive, crit, decisions)
    alive2 = [k for k in alive if not (unc[k] and l1[k] < edge_prune_threshold)]
    P, l2, st2 = _one_pass(g, P, alive2, crit, decisions)
    kept = np.zeros(m, bool)
    kept[alive2] = True
    st1["line_process"] = l1
    return np.stack(P), np.where(kept, l2, 0.0), kept, dict(passes=[st1, st2], decisions=decisions)


# ---- the rest of the layer ----------------------------------------------------------------------------------------------------

def odometry_poses(X):
    """pose_0 = I, pose_{i+1} = (X_i ... X_0)^-1 (test_multi_ate.py:129-130)."""
    acc, out = np.eye(4), [np.eye(4)]
    for Xi in np.asarray(X, np.float64):
        acc = Xi @ acc
        out.append(np.linalg.inv(acc))
    return np.stack(out)


def loop_closure_mask(info, n_source, n_target, T, min_overlap=0.30):
    info, T = np.asarray(info, np.float64), np.asarray(T, np.float64)
    small = info[:, 5, 5] / np.minimum(n_source, n_target) < min_overlap
    ident = np.trace(T, axis1=1, axis2=2) == 4.0
    return ~(small | ident)


def absolute_trajectory_error(gt, est):
    """RMSE in cm of the positions after the rigid alignment est -> gt (test_multi_ate.py align, 268-287)."""
    a = np.asarray(est, np.float64)[:, :3, 3]
    b = np.asarray(gt, np.float64)[:, :3, 3]
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ S @ U.T
    err = (R @ a.T).T + (cb - R @ ca) - b
    return float(np.sqrt((err ** 2).sum(1).mean()) * 100.0)


# ---- test graphs --------------------------------------------------------------------------------------------------------------

def random_pose(rng, rot, trans):
    v = np.concatenate([rng.uniform(-rot, rot, 3), rng.uniform(-trans, trans, 3)])
    return mat(v)


def random_information(rng, rows=300):
    q = rng.uniform(-1.5, 1.5, (rows, 3)).astype(np.float32)
    return info_terms(q, np.arange(rows)).sum(0)


def planted_graph(seed, n=12, n_true=10, n_false=4, noise=0.002, rot=0.5, trans=1.0):
    """An odometry chain with noise, `n_true` true and `n_false` false loop closures; the start is the odometry chain.
    -> dict(poses0, src, tgt, X, info, unc, planted [m] bool (the false closures), gt)."""
    rng = np.random.default_rng(seed)
    gt = [np.eye(4)]
    for _ in range(n - 1):
        gt.append(gt[-1] @ random_pose(rng, rot, trans))
    src, tgt, X, info, unc, planted = [], [], [], [], [], []

    def add(s, t, false):
        # an edge (s, t) measures P_t^-1 P_s
        Xk = random_pose(rng, 1.0, 2.0) if false else np.linalg.inv(gt[t]) @ gt[s] @ random_pose(rng, noise, noise)
        src.append(s); tgt.append(t); X.append(Xk); info.append(random_information(rng))
        unc.append(t != s + 1 if s < t else True); planted.append(false)

    for i in range(n - 1):
        add(i, i + 1, False)
    pairs = [(s, t) for s in range(n) for t in range(s + 2, n)]
    pick = rng.permutation(len(pairs))[:n_true + n_false]
    for c, idx in enumerate(pick):
        add(pairs[idx][0], pairs[idx][1], c >= n_true)
    poses0 = [np.eye(4)]
    for i in range(n - 1):
        # X_i = P_{i+1}^-1 P_i  ->  P_{i+1} = P_i X_i^-1
        poses0.append(poses0[-1] @ np.linalg.inv(X[i]))
    return dict(poses0=np.stack(poses0), src=np.array(src, np.int32), tgt=np.array(tgt, np.int32), X=np.stack(X), info=np.stack(info),
                unc=np.array(unc, bool), planted=np.array(planted, bool), gt=np.stack(gt))


def hard_graph(seed, n=8):
    """Large motions between neighbours, started from identity poses: Levenberg-Marquardt rejects steps here."""
    rng = np.random.default_rng(seed)
    gt = [np.eye(4)]
    for _ in range(n - 1):
        gt.append(gt[-1] @ random_pose(rng, 1.5, 2.0))
    src, tgt, X, info, unc = [], [], [], [], []
    for i in range(n - 1):
        src.append(i); tgt.append(i + 1); X.append(np.linalg.inv(gt[i + 1]) @ gt[i]); info.append(random_information(rng)); unc.append(False)
    for s, t in ((0, 3), (2, 6), (1, 7), (4, 7)):
        src.append(s); tgt.append(t); X.append(np.linalg.inv(gt[t]) @ gt[s] @ random_pose(rng, 0.01, 0.01))
        info.append(random_information(rng)); unc.append(True)
    return dict(poses0=np.stack([np.eye(4)] * n), src=np.array(src, np.int32), tgt=np.array(tgt, np.int32), X=np.stack(X),
                info=np.stack(info), unc=np.array(unc, bool), gt=np.stack(gt))


def run(graph, order=None, **kw):
    """global_optimization of a test graph with the edges in `order` (a permutation; None: as given); the per-edge outputs come
    back in the graph's own edge order."""
    m = len(graph["src"])
    o = np.arange(m) if order is None else np.asarray(order)
    mask = kw.pop("edge_mask", None)
    P, l, kept, st = global_optimization(graph["poses0"], graph["src"][o], graph["tgt"][o], graph["X"][o], graph["info"][o],
                                         graph["unc"][o], None if mask is None else np.asarray(mask)[o], **kw)
    inv = np.argsort(o)
    return P, l[inv], kept[inv], st


# ---- the graphs that the host and the device tests share --------------------------------------------------------------------------

REFERENCE_OPTIONS = dict(edge_prune_threshold=0.25, preference_loop_closure=20.0, reference_node=0)     # what the reference passes
PLANTED_SEEDS = ((0, 0.002), (1, 0.002), (2, 0.05))       # (seed, odometry noise) of the planted-closure graphs
HARD_SEED = 0                                               # the rejected-step case (seeds 0..11 tried: DESIGN.md 4m)


def two_node_graph():
    X = mat([0.1, -0.2, 0.3, 0.5, -0.4, 0.2])
    rng = np.random.default_rng(5)
    return dict(poses0=np.stack([np.eye(4), np.linalg.inv(X)]), src=np.array([0], np.int32), tgt=np.array([1], np.int32), X=X[None],
                info=random_information(rng)[None], unc=np.array([False]))


def sub_graph(graph, keep):
    """The graph with only the edges `keep` (a bool mask or an index list)."""
    out = dict(graph)
    for k in ("src", "tgt", "X", "info", "unc", "planted"):
        if k in graph:
            out[k] = graph[k][keep]
    return out


def chain_with_one_false_closure(seed=3, n=5):
    g = planted_graph(seed, n=n, n_true=0, n_false=1)
    assert g["planted"].sum() == 1
    return g


def test_graphs():
    """name -> (graph, options, mask or None): every graph the device tests run."""
    out = {}
    for seed, noise in PLANTED_SEEDS:
        out[f"planted{seed}"] = (planted_graph(seed, noise=noise), REFERENCE_OPTIONS, None)
    g0 = out["planted0"][0]
    out["ref5"] = (g0, dict(REFERENCE_OPTIONS, reference_node=5), None)
    out["free"] = (g0, dict(REFERENCE_OPTIONS, reference_node=-1), None)
    mask = np.ones(len(g0["src"]), bool)
    mask[[3, 13]] = False                                   # an odometry edge and a loop closure
    out["masked"] = (g0, REFERENCE_OPTIONS, mask)
    out["deleted"] = (sub_graph(g0, mask), REFERENCE_OPTIONS, None)
    out["two"] = (two_node_graph(), REFERENCE_OPTIONS, None)
    out["three"] = (planted_graph(4, n=3, n_true=1, n_false=0), REFERENCE_OPTIONS, None)
    out["only_closure_pruned"] = (chain_with_one_false_closure(), REFERENCE_OPTIONS, None)
    out["hard"] = (hard_graph(HARD_SEED), REFERENCE_OPTIONS, None)
    return out


def trace_array(stats, max_iteration=100):
    """[2, max_iteration + 1, 2] (residual, lambda), NaN padded: the device's trace of one graph."""
    t = np.full((2, max_iteration + 1, 2), np.nan)
    for p, st in enumerate(stats["passes"]):
        t[p, :len(st["trace"])] = st["trace"]
    return t


def order_floor():
    """The largest gap, per quantity, between the restatement with the edges as given and reversed, over every test graph: what
    the order of summation alone does.  -> dict(poses, line_process, residual); prints one line per graph."""
    floor = dict(poses=0.0, line_process=0.0, residual=0.0)
    for name, (g, opt, mask) in test_graphs().items():
        m = len(g["src"])
        a = run(g, edge_mask=mask, **opt)
        b = run(g, order=np.arange(m)[::-1], edge_mask=mask, **opt)
        same = a[3]["decisions"] == b[3]["decisions"] and np.array_equal(a[2], b[2])
        ta, tb = trace_array(a[3])[:, :, 0], trace_array(b[3])[:, :, 0]
        ok = np.isfinite(ta) & np.isfinite(tb)
        gaps = dict(poses=np.abs(a[0] - b[0]).max(), line_process=np.abs(a[1] - b[1]).max(),
                    residual=(np.abs(ta - tb)[ok] / np.maximum(1.0, np.abs(ta[ok]))).max())
        print(f"{name:22s} same decisions: {same}  " + "  ".join(f"{k} {v:.3e}" for k, v in gaps.items()))
        for k, v in gaps.items():
            floor[k] = max(floor[k], float(v))
    return floor


if __name__ == "__main__":
    f = order_floor()
    print("floor:", {k: f"{v:.3e}" for k, v in f.items()})
    print("tolerance (16 x floor):", {k: f"{16 * v:.3e}" for k, v in f.items()})
