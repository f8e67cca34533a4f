"""GPU tests of the evaluation solvers (gmf_amd/solvers.py, csrc/solver_kernels.hip) against a numpy float64 restatement of their
contract: correspondence RANSAC (sampler, fit, scoring, winner) and point-to-point ICP (open3d's loop), ragged batching,
determinism and graph capture."""
import math

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import gmf_amd
from gmf_amd import synthetic
from test_solvers_host import kabsch_np, ransac_draw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatements
# ---------------------------------------------------------------------------------------------------------------------------

def ransac_np(src, tgt, mask, tau, n, H, seed, pair=0, chunk=500):
    """Every hypothesis of one pair: participating rows P, samples [H,n] (numbered in P), R [H,3,3], t [H,3], the inlier counts
    lo / mid / hi at tau^2 (1 - 1e-5) / tau^2 / tau^2 (1 + 1e-5), and the sum of the inliers' d^2 at tau^2."""
    src = np.asarray(src, np.float64)
    tgt = np.asarray(tgt, np.float64)
    P = np.arange(len(src)) if mask is None else np.flatnonzero(mask)
    S, Q = src[P], tgt[P]
    M = len(P)
    smp = ransac_draw(seed, pair, np.arange(H), M, n)
    R, t = kabsch_np(S[smp], Q[smp])
    t2 = tau * tau
    lo, mid, hi = (np.zeros(H, np.int64) for _ in range(3))
    sd = np.zeros(H)
    for h0 in range(0, H, chunk):
        d = np.einsum("hij,nj->hni", R[h0:h0 + chunk], S) + t[h0:h0 + chunk, None, :] - Q[None]
        d2 = (d * d).sum(-1)
        lo[h0:h0 + chunk] = (d2 < t2 * (1 - 1e-5)).sum(1)
        m = d2 < t2
        mid[h0:h0 + chunk] = m.sum(1)
        hi[h0:h0 + chunk] = (d2 < t2 * (1 + 1e-5)).sum(1)
        sd[h0:h0 + chunk] = np.where(m, d2, 0).sum(1)
    return dict(P=P, smp=smp, R=R, t=t, lo=lo, mid=mid, hi=hi, sd=sd, S=S, Q=Q)


def icp_np(S, Q, T0, tau, max_iteration=30, rf=1e-6, rr=1e-6):
    """open3d's registration_icp loop (point-to-point) in float64 with an exact nearest-neighbour search."""
    S = np.asarray(S, np.float64)
    Q = np.asarray(Q, np.float64)
    tree = cKDTree(Q)

    def evaluate(T):
        P = S @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(P)
        d2 = d * d
        c = d2 < tau * tau
        k = int(c.sum())
        return P, j, c, len(S) and k / len(S), math.sqrt(d2[c].sum() / k) if k else 0.0

    T = np.asarray(T0, np.float64).copy()
    P, j, c, fit, rm = evaluate(T)
    it = 0
    for i in range(max_iteration):
        dT = np.eye(4)
        if c.any():
            R, t = kabsch_np(P[c], Q[j[c]])
            dT[:3, :3], dT[:3, 3] = R, t
        T = dT @ T
        f0, r0 = fit, rm
        P, j, c, fit, rm = evaluate(T)
        it = i + 1
        if abs(fit - f0) < rf and abs(rm - r0) < rr:
            break
    return T, fit, rm, it, np.where(c, j, -1)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def _perturb(T, deg, dist, seed):
    r = np.random.default_rng(seed)
    D = np.eye(4)
    D[:3, :3] = _rot(r.normal(size=3), deg)
    v = r.normal(size=3)
    D[:3, 3] = dist * v / np.linalg.norm(v)
    return (D @ np.asarray(T, np.float64)).astype(np.float32)


def _g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. RANSAC against the restatement
# ---------------------------------------------------------------------------------------------------------------------------

def _pointdsc_case(seed, N, ratio, masked):
    p = synthetic.synthetic_pair(seed, N, inlier_ratio=ratio)
    mask = None
    if masked:                                   # pred_labels > 0: most inliers and some outliers
        r = np.random.default_rng([seed, 77])
        lab = p["gt_labels"] > 0
        mask = np.where(lab, r.random(N) < 0.9, r.random(N) < 0.3)
    return p["src_keypts"], p["tgt_keypts"], mask


RANSAC_CASES = [
    ("pointdsc-1000-25%", lambda: _pointdsc_case(11, 1000, 0.25, False), 0.10, 3, 5000),
    ("pointdsc-1000-25%-mask", lambda: _pointdsc_case(12, 1000, 0.25, True), 0.10, 3, 5000),
    ("pointdsc-5000-5%", lambda: _pointdsc_case(13, 5000, 0.05, False), 0.10, 3, 5000),
    ("pointdsc-5000-5%-mask", lambda: _pointdsc_case(14, 5000, 0.05, True), 0.10, 3, 5000),
    ("dgr-8000", lambda: tuple(x.numpy() if torch.is_tensor(x) else x for x in synthetic.dgr_scene(8000, 3)[:2]) + (None,),
     0.06, 4, 80000),
]


@pytest.mark.parametrize("name,make,tau,n,H", RANSAC_CASES, ids=[c[0] for c in RANSAC_CASES])
def test_ransac_matches_restatement(name, make, tau, n, H):
    src, tgt, mask = make()
    seed = 1234
    ref = ransac_np(src, tgt, mask, tau, n, H, seed)
    T, inl, fit, rmse, hyp, sample = gmf_amd.ransac_correspondence_batched(
        _g(src)[None], _g(tgt)[None], tau, mask=None if mask is None else _g(mask)[None], ransac_n=n, num_hypotheses=H, seed=seed)
    T, inl, fit, rmse = T[0].cpu().numpy(), inl[0].cpu().numpy(), float(fit[0]), float(rmse[0])
    w, sample = int(hyp[0]), sample[0].cpu().numpy()
    lo, hi, mid = ref["lo"], ref["hi"], ref["mid"]
    M = len(ref["P"])
    assert 0 <= w < H
    assert hi[w] >= lo.max(), (hi[w], lo.max())
    cnt = int(inl.sum())
    assert lo[w] <= cnt <= hi[w]
    assert np.array_equal(sample, ref["P"][ref["smp"][w]])
    assert np.abs(T[:3, :3] - ref["R"][w]).max() < 1e-5 and np.abs(T[:3, 3] - ref["t"][w]).max() < 1e-5
    assert np.array_equal(T[3], [0, 0, 0, 1])
    assert abs(fit - cnt / M) < 1e-6
    if mask is not None:
        assert not inl[~mask].any()
    # the scene has no ambiguous contender: every hypothesis that could reach the winner's count is counted exactly, and a tie in
    # count is broken by a sum of d^2 that differs clearly - then the winner and its inlier mask are exactly the restatement's
    best = np.lexsort((np.arange(H), ref["sd"], -mid))[0]
    contenders = np.flatnonzero(hi >= lo[best])
    assert (lo[contenders] == hi[contenders]).all(), name
    tied = contenders[(mid[contenders] == mid[best]) & (contenders != best)]
    assert (np.abs(ref["sd"][tied] - ref["sd"][best]) > 1e-5 * ref["sd"][best]).all(), name
    assert w == best, (w, best)
    d = ref["S"] @ ref["R"][w].T + ref["t"][w] - ref["Q"]
    d2 = (d * d).sum(1)
    want = np.zeros(len(src), bool)
    want[ref["P"]] = d2 < tau * tau
    assert np.array_equal(inl, want)
    assert abs(rmse - math.sqrt(ref["sd"][w] / mid[w])) <= 1e-4 * rmse


# ---------------------------------------------------------------------------------------------------------------------------
# 2. ICP against the restatement
# ---------------------------------------------------------------------------------------------------------------------------

def _keypoint_case(seed, N):
    p = synthetic.synthetic_pair(seed, N)
    return p["src_keypts"], p["tgt_keypts"], _perturb(p["gt_trans"], 5.0, 0.10, seed), 0.10, p["gt_trans"]


def _cloud_case(seed, Ns, Nt):
    r = np.random.default_rng([seed, 0xc10d])
    X = r.uniform(0, 3, (Nt, 3))
    R = synthetic.random_rotation(r)
    t = r.uniform(-0.5, 0.5, 3)
    tgt = (X @ R.T + t + r.normal(0, 0.005, X.shape)).astype(np.float32)
    src = X[r.permutation(Nt)[:Ns]].astype(np.float32)
    Tg = np.eye(4)
    Tg[:3, :3], Tg[:3, 3] = R, t
    return src, tgt, _perturb(Tg, 2.0, 0.03, seed), 0.05, Tg


ICP_CASES = [("keypoints-1000", lambda: _keypoint_case(21, 1000)), ("keypoints-5000", lambda: _keypoint_case(22, 5000)),
             ("cloud-8k-10k", lambda: _cloud_case(23, 8000, 10000))]


@pytest.mark.parametrize("name,make", ICP_CASES, ids=[c[0] for c in ICP_CASES])
def test_icp_matches_restatement(name, make):
    src, tgt, T0, tau, _ = make()
    Tr, fr, rr, itr, _ = icp_np(src, tgt, T0, tau)
    T, fit, rmse, it, nn = gmf_amd.icp_point_to_point_batched(_g(src)[None], _g(tgt)[None], _g(T0)[None], tau)
    T = T[0].cpu().numpy()
    assert np.abs(T - Tr).max() < 1e-4, np.abs(T - Tr).max()
    assert abs(float(fit[0]) - fr) <= 2.0 / len(src)
    assert abs(float(rmse[0]) - rr) <= 1e-4 * rr
    assert abs(int(it[0]) - itr) <= 2, (int(it[0]), itr)
    nn = nn[0].cpu().numpy()
    assert abs(int((nn >= 0).sum()) - round(fr * len(src))) <= 2


def test_icp_recovers_clean_scene():
    r = np.random.default_rng(31)
    src = r.uniform(0, 3, (1000, 3)).astype(np.float32)
    R = synthetic.random_rotation(r)
    t = r.uniform(-0.5, 0.5, 3)
    tgt = (src.astype(np.float64) @ R.T + t).astype(np.float32)
    Tg = np.eye(4)
    Tg[:3, :3], Tg[:3, 3] = R, t
    T0 = _perturb(Tg, 5.0, 0.10, 31)
    T, fit, _, _, _ = gmf_amd.icp_point_to_point_batched(_g(src)[None], _g(tgt)[None], _g(T0)[None], 0.10, max_iteration=100)
    T = T[0].cpu().numpy().astype(np.float64)
    cos = (np.trace(T[:3, :3].T @ R) - 1) / 2
    assert math.degrees(math.acos(min(1.0, max(-1.0, cos)))) < 0.1
    assert np.linalg.norm(T[:3, 3] - t) < 0.01
    assert float(fit[0]) > 0.99


# ---------------------------------------------------------------------------------------------------------------------------
# 3. ragged batches equal pair-by-pair calls bitwise
# ---------------------------------------------------------------------------------------------------------------------------

def _ragged_ransac_batch():
    sizes = [700, 1200, 40, 300, 2500, 5, 900, 1600]
    pairs, masks = [], []
    for b, N in enumerate(sizes):
        p = synthetic.synthetic_pair(100 + b, N)
        m = np.random.default_rng([b, 5]).random(N) < 0.8
        if b == 5:
            m[:] = False
            m[[1, 3]] = True                       # M_b = 2 < ransac_n: identity, no inliers
        pairs.append((p["src_keypts"], p["tgt_keypts"]))
        masks.append(m)
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    return pairs, masks, off


def _eq(a, b):
    return torch.equal(a.cpu(), b.cpu())


def test_ransac_ragged_batch_equals_pairs():
    pairs, masks, off = _ragged_ransac_batch()
    S = _g(np.concatenate([p[0] for p in pairs]))
    Q = _g(np.concatenate([p[1] for p in pairs]))
    Mk = _g(np.concatenate(masks))
    out = gmf_amd.ransac_correspondence_batched(S, Q, 0.1, offsets=off, mask=Mk, num_hypotheses=3000, seed=9)
    for b in range(len(pairs)):
        one = gmf_amd.ransac_correspondence_batched(_g(pairs[b][0])[None], _g(pairs[b][1])[None], 0.1, mask=_g(masks[b])[None],
                                                    num_hypotheses=3000, seed=9, first_pair=b)
        assert _eq(out[0][b], one[0][0]), b
        assert _eq(out[1][off[b]:off[b + 1]], one[1][0]), b
        for k in (2, 3, 4, 5):
            assert _eq(out[k][b], one[k][0]), (b, k)
    T, inl, fit, rmse, hyp, smp = (x.cpu() for x in out)
    assert int(hyp[5]) == -1 and torch.equal(T[5], torch.eye(4)) and float(fit[5]) == 0 and float(rmse[5]) == 0
    assert not inl[off[5]:off[6]].any() and (smp[5] == -1).all()
    # device offsets give the same bits
    dev_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    out2 = gmf_amd.ransac_correspondence_batched(S, Q, 0.1, offsets=dev_off, mask=Mk, num_hypotheses=3000, seed=9)
    for a, b in zip(out, out2):
        assert _eq(a, b)


def _ragged_icp_batch():
    cases = []
    for b, (Ns, Nt) in enumerate([(500, 700), (1000, 1000), (64, 300), (2000, 1500), (300, 300), (1200, 900), (50, 2000), (800, 800)]):
        r = np.random.default_rng([b, 0x1c9])
        X = r.uniform(0, 3, (max(Ns, Nt), 3))
        R = synthetic.random_rotation(r)
        t = r.uniform(-0.3, 0.3, 3)
        tgt = (X[:Nt] @ R.T + t + r.normal(0, 0.005, (Nt, 3))).astype(np.float32)
        src = X[:Ns].astype(np.float32)
        Tg = np.eye(4)
        Tg[:3, :3], Tg[:3, 3] = R, t
        T0 = _perturb(Tg, 3.0, 0.05, b)
        if b == 4:
            tgt = tgt + np.float32(100.0)          # no target within tau: C is empty
        cases.append((src, tgt, T0))
    return cases


def test_icp_ragged_batch_equals_pairs():
    cases = _ragged_icp_batch()
    soff = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]).tolist()
    S = _g(np.concatenate([c[0] for c in cases]))
    Q = _g(np.concatenate([c[1] for c in cases]))
    I = _g(np.stack([c[2] for c in cases]))
    out = gmf_amd.icp_point_to_point_batched(S, Q, I, 0.08, source_offsets=soff, target_offsets=toff)
    for b, (s, q, T0) in enumerate(cases):
        one = gmf_amd.icp_point_to_point_batched(_g(s)[None], _g(q)[None], _g(T0)[None], 0.08)
        for k in range(4):
            assert _eq(out[k][b], one[k][0]), (b, k)
        assert _eq(out[4][soff[b]:soff[b + 1]], one[4][0]), b
    T, fit, rmse, it, nn = (x.cpu() for x in out)
    assert float(fit[4]) == 0 and float(rmse[4]) == 0 and int(it[4]) == 1
    assert torch.equal(T[4], torch.as_tensor(cases[4][2])) and (nn[soff[4]:soff[5]] == -1).all()


def test_icp_refine_equals_registration_icp():
    B, N = 3, 1500
    pairs = [synthetic.synthetic_pair(200 + b, N) for b in range(B)]
    src = _g(np.stack([p["src_keypts"] for p in pairs]))
    tgt = _g(np.stack([p["tgt_keypts"] for p in pairs]))
    T0 = _g(np.stack([_perturb(p["gt_trans"], 4.0, 0.05, b) for b, p in enumerate(pairs)]))
    Tb = gmf_amd.icp_refine(src, tgt, T0)
    assert Tb.shape == (B, 4, 4) and Tb.dtype == torch.float32
    for b in range(B):
        r = gmf_amd.registration_icp(src[b], tgt[b], 0.10, init=T0[b])
        assert _eq(Tb[b], r.transformation), b
        k = r.correspondence_set
        assert k.shape[1] == 2 and abs(r.fitness - k.shape[0] / N) < 1e-6
        if k.shape[0]:
            d = (src[b][k[:, 0]] @ r.transformation[:3, :3].T + r.transformation[:3, 3] - tgt[b][k[:, 1]]).norm(dim=1)
            assert float(d.max()) < 0.10 + 1e-4


def test_open3d_ransac_wrapper():
    p = synthetic.synthetic_pair(300, 2000)
    src, tgt = _g(p["src_keypts"]), _g(p["tgt_keypts"])
    keep = np.flatnonzero(np.random.default_rng(4).random(2000) < 0.6)
    corres = torch.as_tensor(np.stack([keep, keep], 1)).to(DEV)
    res = gmf_amd.registration_ransac_based_on_correspondence(src, tgt, corres, 0.10, ransac_n=3, max_iteration=5000,
                                                              max_validation=4000, seed=2)
    mask = torch.zeros(2000, dtype=torch.bool, device=DEV)
    mask[corres[:, 0]] = True
    T, inl, fit, rmse, _, _ = gmf_amd.ransac_correspondence_batched(src[corres[:, 0]][None], tgt[corres[:, 1]][None], 0.10,
                                                                    num_hypotheses=4000, seed=2)
    assert _eq(res.transformation, T[0])
    assert _eq(res.correspondence_set, corres[inl[0]])
    assert res.fitness == float(fit[0]) and res.inlier_rmse == float(rmse[0])
    Tg = p["gt_trans"]
    assert np.abs(res.transformation.cpu().numpy() - Tg).max() < 0.05


# ---------------------------------------------------------------------------------------------------------------------------
# 4. determinism and graph capture
# ---------------------------------------------------------------------------------------------------------------------------

def test_determinism_and_seed():
    src, tgt, mask = _pointdsc_case(41, 3000, 0.1, True)
    args = (_g(src)[None], _g(tgt)[None], 0.1)
    a = gmf_amd.ransac_correspondence_batched(*args, mask=_g(mask)[None], num_hypotheses=5000, seed=5)
    b = gmf_amd.ransac_correspondence_batched(*args, mask=_g(mask)[None], num_hypotheses=5000, seed=5)
    for x, y in zip(a, b):
        assert _eq(x, y)
    c = gmf_amd.ransac_correspondence_batched(*args, mask=_g(mask)[None], num_hypotheses=5000, seed=6)
    assert int(c[4][0]) != int(a[4][0])
    s, q, T0, tau, _ = _keypoint_case(42, 3000)
    i1 = gmf_amd.icp_point_to_point_batched(_g(s)[None], _g(q)[None], _g(T0)[None], tau)
    i2 = gmf_amd.icp_point_to_point_batched(_g(s)[None], _g(q)[None], _g(T0)[None], tau)
    for x, y in zip(i1, i2):
        assert _eq(x, y)


def test_graph_capture_equals_eager():
    pairs, masks, off = _ragged_ransac_batch()
    S = _g(np.concatenate([p[0] for p in pairs]))
    Q = _g(np.concatenate([p[1] for p in pairs]))
    Mk = _g(np.concatenate(masks))
    cases = _ragged_icp_batch()
    soff = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]).tolist()
    IS = _g(np.concatenate([c[0] for c in cases]))
    IQ = _g(np.concatenate([c[1] for c in cases]))
    II = _g(np.stack([c[2] for c in cases]))

    def run():
        r = gmf_amd.ransac_correspondence_batched(S, Q, 0.1, offsets=off, mask=Mk, num_hypotheses=3000, seed=9)
        i = gmf_amd.icp_point_to_point_batched(IS, IQ, II, 0.08, source_offsets=soff, target_offsets=toff)
        return r + i

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                           # (also sizes the workspace and uploads the offsets before the capture)
            eager = [x.clone() for x in run()]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = run()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, captured):
        assert _eq(x, y)
