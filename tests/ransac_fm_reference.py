"""A float64 numpy restatement of the feature-matching RANSAC of gmf_amd/solvers.py (`ransac_feature_matching_batched`; kernels
k_fm_* of csrc/solver_kernels.hip), one pair at a time: propose, select, evaluate, finish.  It shares the sampler and the Kabsch
restatements of tests/test_solvers_host.py, and it reports, beside each decision, how close that decision was, so that a test can
leave the borderline ones out instead of widening a bound.  tests/test_gpu_ransac_fm.py holds the device to it."""
import numpy as np
from scipy.spatial import cKDTree

from test_solvers_host import kabsch_np, ransac_draw

BORDER_CHECK = 1e-4          # a hypothesis is borderline when an fp64 checker margin is below this share of its threshold
BORDER_ROW = 1e-5            # a row is borderline when | d - tau | < this share of tau


def make_scene(seed, ns, nt, tau, inlier_share=0.6, noise=0.02, far=10.0, lo=-1.0, hi=1.0):
    """A pair made so that the checks are not borderline.  -> (src [ns,3] f32, tgt [nt,3] f32, nn [ns] int64, R, t, inl [ns] bool).
    The first k = min(inlier_share ns, nt - 8) source rows have their own target R s + t + noise tau U(-1, 1)^3 (far below tau);
    the other targets are clutter in the same box; the other source rows get a target at least `far` tau from their true place."""
    r = np.random.default_rng(seed)
    q, _ = np.linalg.qr(r.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    t = r.uniform(-0.3, 0.3, 3)
    src = r.uniform(lo, hi, (ns, 3)).astype(np.float32)
    k = int(min(inlier_share * ns, nt - 8))
    moved = src.astype(np.float64) @ q.T + t
    tgt = np.empty((nt, 3), np.float64)
    tgt[:k] = moved[:k] + noise * tau * r.uniform(-1, 1, (k, 3))
    tgt[k:] = r.uniform(lo, hi, (nt - k, 3)) @ q.T + t
    perm = r.permutation(nt)                                  # the matching targets are not in the sources' order
    inv = np.empty(nt, np.int64)
    inv[perm] = np.arange(nt)
    tgt = tgt[perm].astype(np.float32)
    nn = np.empty(ns, np.int64)
    nn[:k] = inv[:k]
    for i in range(k, ns):
        d = np.linalg.norm(tgt.astype(np.float64) - moved[i], axis=1)
        nn[i] = r.choice(np.flatnonzero(d > far * tau))
    order = r.permutation(ns)                                 # nor are the inliers the first source rows
    inl = np.zeros(ns, bool)
    inl[:k] = True
    return src[order], tgt, nn[order], q, t, inl[order]


def propose(src, tgt, nn, n, H, seed=0, pair=0, checker_distance=None, edge_length_threshold=None):
    """Step 1 for h = 0 .. H-1.  -> dict(smp [H,n], R [H,3,3], t [H,3], passed [H] bool, border [H] bool): border marks the
    hypotheses one of whose checker margins is below BORDER_CHECK of its threshold (in either direction)."""
    S, Q = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    nn = np.asarray(nn, np.int64)
    ns, nt = len(S), len(Q)
    if ns < n or nt == 0:
        z = np.zeros(H, bool)
        return dict(smp=np.zeros((H, n), np.int64), R=np.tile(np.eye(3), (H, 1, 1)), t=np.zeros((H, 3)), passed=z, border=z.copy())
    smp = ransac_draw(seed, pair, np.arange(H), ns, n)
    j = nn[smp]
    inside = ((j >= 0) & (j < nt)).all(1)
    A, Bq = S[smp], Q[np.clip(j, 0, nt - 1)]
    passed, border = inside.copy(), np.zeros(H, bool)
    if edge_length_threshold is not None:
        r2 = float(edge_length_threshold) ** 2
        iu, ju = np.triu_indices(n, 1)
        ds = ((A[:, iu] - A[:, ju]) ** 2).sum(-1)
        dt = ((Bq[:, iu] - Bq[:, ju]) ** 2).sum(-1)
        passed &= ((ds >= r2 * dt) & (dt >= r2 * ds)).all(1)
        scale = np.maximum(np.maximum(ds, dt), 1e-300)
        border |= (np.minimum(np.abs(ds - r2 * dt), np.abs(dt - r2 * ds)) / scale < 2 * BORDER_CHECK).any(1)
    with np.errstate(all="ignore"):
        R, t = kabsch_np(A, Bq)
    fin = np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1)
    passed &= fin
    if checker_distance is not None:
        cd = float(checker_distance)
        d = np.linalg.norm(np.einsum("hij,hkj->hki", R, A) + t[:, None, :] - Bq, axis=-1)
        passed &= (d <= cd).all(1)
        border |= (np.abs(d - cd) < BORDER_CHECK * cd).any(1)
    border &= inside & fin
    return dict(smp=smp, R=R, t=t, passed=passed, border=border)


def select(passed, V):
    """Step 2: the first V passing h in increasing order."""
    return np.flatnonzero(passed)[:V]


def evaluate(src, tgt, R, t, tau):
    """Step 3 for one pose.  -> dict(count, border (rows with |d - tau| < BORDER_ROW tau), sum_d2, j [ns] (nearest target), d [ns],
    gap [ns] (distance of the second nearest minus the nearest))."""
    P = np.asarray(src, np.float64) @ R.T + t
    k = min(2, len(tgt))
    d, j = cKDTree(np.asarray(tgt, np.float64)).query(P, k=k)
    if k == 2:
        gap, d, j = d[:, 1] - d[:, 0], d[:, 0], j[:, 0]
    else:
        gap = np.full(len(P), np.inf)
        d, j = d.reshape(-1), j.reshape(-1)
    c = d < tau
    return dict(count=int(c.sum()), border=int((np.abs(d - tau) < BORDER_ROW * tau).sum()), sum_d2=float((d[c] ** 2).sum()),
                j=np.where(c, j, -1), d=d, gap=gap)


def ransac_fm_np(src, tgt, nn, tau, n=4, H=1000, V=100, checker_distance=None, edge_length_threshold=None, seed=0, pair=0):
    """Steps 1 to 4 of one pair.  -> dict(prop (propose's), hyp [<= V], ev (one evaluate() per validated h), winner (position in
    hyp, -1: none), T [4,4], fitness, inlier_rmse, hypothesis, sample, nn_out)."""
    src, tgt = np.asarray(src), np.asarray(tgt)
    prop = propose(src, tgt, nn, n, H, seed, pair, checker_distance, edge_length_threshold)
    hyp = select(prop["passed"], V)
    ev = [evaluate(src, tgt, prop["R"][h], prop["t"][h], tau) for h in hyp]
    win = -1
    for v, e in enumerate(ev):                                # count larger, then sum smaller, then h smaller
        if e["count"] > 0 and (win < 0 or (e["count"], -e["sum_d2"]) > (ev[win]["count"], -ev[win]["sum_d2"])):
            win = v
    T = np.eye(4)
    out = dict(prop=prop, hyp=hyp, ev=ev, winner=win, T=T, fitness=0.0, inlier_rmse=0.0, hypothesis=-1,
               sample=np.full(n, -1, np.int64), nn_out=np.full(len(src), -1, np.int64))
    if win >= 0:
        h, e = hyp[win], ev[win]
        T[:3, :3], T[:3, 3] = prop["R"][h], prop["t"][h]
        out.update(fitness=e["count"] / len(src), inlier_rmse=float(np.sqrt(e["sum_d2"] / e["count"])), hypothesis=int(h),
                   sample=prop["smp"][h], nn_out=e["j"])
    return out


def self_test():
    """A clean scene recovers its pose; the first-V rule; the degenerate pairs; the scenes' own share of borderline decisions."""
    tau = 0.1
    src, tgt, nn, R, t, inl = make_scene(3, 300, 257, tau, noise=0.0)
    res = ransac_fm_np(src, tgt, nn, tau, H=2000, V=64, checker_distance=tau)
    assert res["winner"] >= 0 and np.abs(res["T"][:3, :3] - R).max() < 1e-5 and np.abs(res["T"][:3, 3] - t).max() < 1e-5
    assert res["fitness"] >= inl.mean() and res["ev"][res["winner"]]["d"][inl].max() < 1e-6       # (fp32 target coordinates)
    assert inl[res["sample"]].all()
    assert (res["nn_out"][inl] == nn[inl]).all()
    # the first-V rule: the list is increasing, V = 8 is a prefix of V = 64, and stopping at the 8th h validates exactly 8
    hyp = res["hyp"]
    assert len(hyp) == 64 and (np.diff(hyp) > 0).all() and res["prop"]["passed"][hyp].all()
    assert not res["prop"]["passed"][:hyp[0]].any()
    r8 = ransac_fm_np(src, tgt, nn, tau, H=2000, V=8, checker_distance=tau)
    assert (r8["hyp"] == hyp[:8]).all()
    assert len(ransac_fm_np(src, tgt, nn, tau, H=int(hyp[7]) + 1, V=64, checker_distance=tau)["hyp"]) == 8
    # without checkers everything validates; each checker alone only removes
    assert (ransac_fm_np(src, tgt, nn, tau, H=100, V=64)["hyp"] == np.arange(64)).all()
    for kw in (dict(checker_distance=tau), dict(edge_length_threshold=0.9)):
        assert propose(src, tgt, nn, 4, 2000, **kw)["passed"].sum() < 2000
    # degenerate pairs
    for s_, q_, n_ in ((src[:3], tgt, nn[:3]), (src, tgt[:0], nn)):
        d = ransac_fm_np(s_, q_, n_, tau, H=50, V=8)
        assert d["winner"] == -1 and d["hypothesis"] == -1 and (d["T"] == np.eye(4)).all() and (d["nn_out"] == -1).all()
    return True
