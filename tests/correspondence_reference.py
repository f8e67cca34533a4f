"""Float64 numpy restatement of what PointDSC's loaders do between descriptors and the network's input
(GMF_PointDSC/datasets/ThreeDMatch.py:163-210, KITTI.py:94-129), written from its meaning: nearest neighbours in descriptor
space both ways with first-index ties, the mutual filter, the gathers, the ground-truth labels, the centring, and the offsets of
a batch.  Also the recipe of the fixture the GPU tests share (make_fixture) and its two preconditions (check_fixture).

For unit descriptors sqrt(2 - 2 <s, t> + 1e-6) falls as <s, t> rises, so the nearest neighbour is the largest dot product."""
from __future__ import annotations

import numpy as np

LEN_BATCH = [(301, 700), (5, 3), (1, 40), (0, 20), (64, 64), (0, 0), (130, 33), (700, 301), (1500, 4200)]
INLIER_THRESHOLD = 0.1
WIDTHS = (5, 32, 33, 64, 128)
SEEDS = {5: 0, 32: 0, 33: 0, 64: 0, 128: 0}           # a seed per width at which check_fixture's preconditions hold


def dots(S, T, exact_ties=False):
    """<s_i, t_j> in float64.  exact_ties: every entry is summed on its own in one fixed order, so that bitwise-equal rows give
    bitwise-equal entries (a BLAS may sum the columns of a block differently)."""
    S, T = np.asarray(S, np.float64), np.asarray(T, np.float64)
    if exact_ties:
        return (S[:, None, :] * T[None, :, :]).sum(-1)
    return S @ T.T


def argmin_both(S, T, exact_ties=False):
    """(source_idx [Ns], target_idx [Nt]): every source row's nearest target row and every target row's nearest source row;
    among equal distances the first index (numpy's argmin)."""
    D = dots(S, T, exact_ties)
    return np.argmax(D, axis=1), np.argmax(D, axis=0)


def mutual_mask(source_idx, target_idx):
    """Row i is kept when the nearest source row of its own match is i."""
    return target_idx[source_idx] == np.arange(len(source_idx))


def build_pair(src_keypts, tgt_keypts, S, T, use_mutual=True, gt_trans=None, inlier_threshold=None, in_dim=6, exact_ties=False):
    """One pair -> dict: source_idx, mutual, corr [M, 2], src_keypts / tgt_keypts [M, 3] (gathers), corr_pos [M, in_dim] float64,
    gt_labels [M] (with gt_trans), label_dist [Ns] (every row's |R x + t - y| to its match, whether kept or not)."""
    Ns = len(S)
    src_keypts, tgt_keypts = np.asarray(src_keypts), np.asarray(tgt_keypts)
    if Ns == 0:
        source_idx, keep = np.zeros(0, np.int64), np.zeros(0, bool)
    else:
        source_idx, target_idx = argmin_both(S, T, exact_ties)
        keep = mutual_mask(source_idx, target_idx) if use_mutual else np.ones(Ns, bool)
    rows = np.nonzero(keep)[0]
    corr = np.stack([rows, source_idx[rows]], 1).astype(np.int64).reshape(-1, 2)
    a, b = src_keypts[corr[:, 0]].reshape(-1, 3), tgt_keypts[corr[:, 1]].reshape(-1, 3)
    out = {"source_idx": source_idx, "mutual": keep, "corr": corr, "src_keypts": a, "tgt_keypts": b}
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    if in_dim == 6:
        pos = np.concatenate([a64, b64], 1)
        out["corr_pos"] = pos - pos.mean(0) if len(pos) else pos
    elif in_dim == 3:
        out["corr_pos"] = a64 - b64
    else:
        raise ValueError(in_dim)
    if gt_trans is not None:
        G = np.asarray(gt_trans, np.float64)
        all_a = src_keypts.astype(np.float64).reshape(-1, 3)
        all_b = tgt_keypts.astype(np.float64).reshape(-1, 3)[source_idx].reshape(-1, 3)
        dist = np.sqrt((((all_a @ G[:3, :3].T + G[:3, 3]) - all_b) ** 2).sum(1))
        out["label_dist"] = dist
        out["gt_labels"] = (dist[rows] < inlier_threshold).astype(np.float32)
    return out


def build_batch(src_keypts, tgt_keypts, S, T, len_batch, use_mutual=True, gt_trans=None, inlier_threshold=None, in_dim=6):
    """The packed batch -> (list of build_pair dicts, offsets [B + 1])."""
    o0 = np.r_[0, np.cumsum([a for a, _ in len_batch])].astype(int)
    o1 = np.r_[0, np.cumsum([b for _, b in len_batch])].astype(int)
    pairs = [build_pair(src_keypts[o0[b]:o0[b + 1]], tgt_keypts[o1[b]:o1[b + 1]], S[o0[b]:o0[b + 1]], T[o1[b]:o1[b + 1]], use_mutual,
                        None if gt_trans is None else gt_trans[b], inlier_threshold, in_dim) for b in range(len(len_batch))]
    return pairs, np.r_[0, np.cumsum([len(p["corr"]) for p in pairs])].astype(np.int32)


# ---- the shared fixture ------------------------------------------------------------------------------------------------------------

def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _rigid(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = R, rng.uniform(-1, 1, 3)
    return G


def _top2_gaps(D, axis):
    """Per row (axis 1) or column (axis 0) of D: (gap between its two largest entries, index of the largest, of the second)."""
    if axis == 0:
        D = D.T
    two = np.argpartition(-D, 1, axis=1)[:, :2]
    v = np.take_along_axis(D, two, 1)
    swap = v[:, 1] > v[:, 0]
    first, second = np.where(swap, two[:, 1], two[:, 0]), np.where(swap, two[:, 0], two[:, 1])
    return np.abs(v[:, 0] - v[:, 1]), first, second


def _separate(rng, s, t, m, copied, min_gap):
    """Redraw random rows until every row's and every column's best and second-best dot product (float64, of the float32 rows)
    differ by more than min_gap.  Only rows that are random anyway are redrawn - source rows from m on, target rows no source row
    copies - so the recipe's distribution is kept but for this condition: it is a rejection step, still a function of the seed.
    With thousands of rows in a race for every maximum, plain seeds almost never meet the bound at d = 128 (about 2 in 10^4)."""
    d = s.shape[1]
    free_t = np.ones(len(t), bool)
    free_t[copied] = False
    for _ in range(200):
        s32, t32 = s.astype(np.float32), t.astype(np.float32)
        D = dots(s32, t32)
        redo_s, redo_t = set(), set()
        if len(t) >= 2:
            g, j1, j2 = _top2_gaps(D, 1)
            for i in np.nonzero(g <= min_gap)[0]:
                if free_t[j2[i]]: redo_t.add(int(j2[i]))
                elif free_t[j1[i]]: redo_t.add(int(j1[i]))
                elif i >= m: redo_s.add(int(i))
                else: raise RuntimeError("correspondence fixture: a race between copied rows; take another seed")
        if len(s) >= 2:
            g, i1, i2 = _top2_gaps(D, 0)
            for j in np.nonzero(g <= min_gap)[0]:
                if i2[j] >= m: redo_s.add(int(i2[j]))
                elif i1[j] >= m: redo_s.add(int(i1[j]))
                elif free_t[j]: redo_t.add(int(j))
                else: raise RuntimeError("correspondence fixture: a race between copied rows; take another seed")
        if not redo_s and not redo_t:
            return s, t
        for i in sorted(redo_s): s[i] = _unit(rng.standard_normal((1, d)))[0]
        for j in sorted(redo_t): t[j] = _unit(rng.standard_normal((1, d)))[0]
    raise RuntimeError("correspondence fixture: the rows did not separate; take another seed")


def make_fixture(d, seed, len_batch=LEN_BATCH):
    """Unit descriptors from a seeded generator; in each pair the first min(Ns, Nt) // 2 source rows are noisy copies (0.35 per
    component of the standard-normal row, before normalising) of distinct target rows, their keypoints the inverse-transformed target keypoints plus at most
    0.02 per axis; everything else random, keypoints in a box of side 4.  Random rows in too close a race are redrawn
    (_separate, to twice the bound check_fixture asserts).  All float32."""
    rng = np.random.default_rng(seed)
    S, T, P, Q, G = [], [], [], [], []
    for ns, nt in len_batch:
        g = _rigid(rng)
        raw = rng.standard_normal((nt, d))
        t = _unit(raw) if nt else np.zeros((0, d))
        s = _unit(rng.standard_normal((ns, d))) if ns else np.zeros((0, d))
        q = rng.uniform(0, 4, (nt, 3))
        p = rng.uniform(0, 4, (ns, 3))
        m = min(ns, nt) // 2
        sel = rng.permutation(nt)[:m] if m else np.zeros(0, int)
        if m:
            s[:m] = _unit(raw[sel] + 0.35 * rng.standard_normal((m, d)))
            p[:m] = (q[sel] - g[:3, 3]) @ g[:3, :3] + rng.uniform(-0.02, 0.02, (m, 3))      # R^T (y - t)
        if ns:
            s, t = _separate(rng, s, t, m, sel, 8 * d * 2.0 ** -24)
        S.append(s), T.append(t), P.append(p), Q.append(q), G.append(g)
    f32 = lambda xs: np.concatenate(xs).astype(np.float32)      # noqa: E731
    return {"src_desc": f32(S), "tgt_desc": f32(T), "src_keypts": f32(P), "tgt_keypts": f32(Q),
            "gt_trans": np.stack(G).astype(np.float32), "len_batch": list(len_batch), "d": d}


def check_fixture(fx, inlier_threshold=INLIER_THRESHOLD):
    """The two preconditions of the exact comparisons, in float64, no row left out -> (smallest gap between the best and the
    second-best dot product over all rows and all columns of all pairs, the bound 4 d 2^-24 it must exceed, the smallest distance of
    a label distance from the threshold)."""
    d = fx["d"]
    o0 = np.r_[0, np.cumsum([a for a, _ in fx["len_batch"]])].astype(int)
    o1 = np.r_[0, np.cumsum([b for _, b in fx["len_batch"]])].astype(int)
    gap, margin = np.inf, np.inf
    for b, (ns, nt) in enumerate(fx["len_batch"]):
        if ns == 0:
            continue
        S, T = fx["src_desc"][o0[b]:o0[b + 1]], fx["tgt_desc"][o1[b]:o1[b + 1]]
        D = dots(S, T)
        for axis, n in ((1, nt), (0, ns)):
            if n >= 2:
                top = np.sort(D, axis=axis)
                top = top[:, -2:] if axis == 1 else top[-2:, :].T
                gap = min(gap, float((top[:, 1] - top[:, 0]).min()))
        r = build_pair(fx["src_keypts"][o0[b]:o0[b + 1]], fx["tgt_keypts"][o1[b]:o1[b + 1]], S, T, True, fx["gt_trans"][b], inlier_threshold)
        margin = min(margin, float(np.abs(r["label_dist"] - inlier_threshold).min()))
    return gap, 4 * d * 2.0 ** -24, margin
