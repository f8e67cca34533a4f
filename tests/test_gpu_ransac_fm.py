"""GPU tests of the feature-matching RANSAC (gmf_amd/solvers.py: ransac_feature_matching_batched and its open3d-shaped wrapper;
kernels k_fm_* of csrc/solver_kernels.hip; DeepGlobalRegistration.safeguard_method) against the float64 restatement of
tests/ransac_fm_reference.py: the two searches bit for bit, the validated list, counts, winner, the first-V rule, the checkers,
ragged batching, determinism, graph capture, the C entry and DGR's safeguard branch."""
import os
import types

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import dgr, fcgf

import fcgf_reference as FR
import ransac_fm_reference as FM
from test_solvers_host import ransac_draw

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0.1
H_CELL = TAU * (1.0 + 1.0 / 1024)            # the grid's cell edge
NAMES = ("T", "fitness", "inlier_rmse", "hypothesis", "sample", "nn_out", "validated", "hyp", "count", "sum")


def _g(x):
    return torch.as_tensor(x).to(DEV)


@pytest.fixture(autouse=True)
def _clean_status():
    yield
    gmf_amd.check_status()


_SCENES = {}


def _scene(name):
    """(src, tgt, nn) numpy arrays.  'small' 300 / 257 and 'mid' 1000 / 777: tests/ransac_fm_reference.make_scene (the sizes differ
    and are no multiples of 64 or 256; coordinates on both sides of zero).  'crowded': 'small' plus 40 targets inside one cell and
    source rows that land there.  'faces': 'small' with half of the targets' coordinates moved to within 1e-6 tau of a cell face."""
    if name not in _SCENES:
        if name in ("small", "mid"):
            seed, ns, nt = {"small": (11, 300, 257), "mid": (12, 1000, 777)}[name]
            _SCENES[name] = FM.make_scene(seed, ns, nt, TAU)
        elif name == "crowded":
            src, tgt, nn, R, t, inl = _scene("small")
            r = np.random.default_rng(21)
            corner = np.array([2, -3, 1]) * H_CELL
            extra = (corner + H_CELL * r.uniform(0.2, 0.8, (40, 3))).astype(np.float32)
            back = ((corner + H_CELL * r.uniform(0.2, 0.8, (7, 3)) - t) @ R).astype(np.float32)      # R^T (c - t)
            _SCENES[name] = (np.concatenate([src, back]), np.concatenate([tgt, extra]),
                             np.concatenate([nn, len(tgt) + np.arange(7)]), R, t, np.concatenate([inl, np.ones(7, bool)]))
        elif name == "faces":
            src, tgt, nn, R, t, inl = _scene("small")
            r = np.random.default_rng(22)
            face = np.round(tgt.astype(np.float64) / H_CELL) * H_CELL + 1e-6 * TAU * r.choice([-1.0, 1.0], tgt.shape)
            move = r.random(tgt.shape) < 0.5
            _SCENES[name] = (src, np.where(move, face, tgt).astype(np.float32), nn, R, t, inl)
    return _SCENES[name]


def _run(name, **kw):
    src, tgt, nn = _scene(name)[:3]
    kw.setdefault("return_hypotheses", True)
    return gmf_amd.ransac_feature_matching_batched(_g(src)[None], _g(tgt)[None], _g(nn)[None], TAU, **kw)


def _assert_equal(a, b, what=""):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and torch.equal(x, y), (what, NAMES[k])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the two searches give the same bits
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kw", [
    ("small", dict(checker_distance=TAU)), ("mid", dict(checker_distance=TAU, edge_length_threshold=0.9)),
    ("crowded", dict(checker_distance=TAU)), ("faces", dict()), ("mid", dict(ransac_n=3))])
def test_brute_equals_grid(name, kw):
    kw = dict(kw, max_iteration=3000, max_validation=32, seed=5)
    brute = _run(name, search="brute", **kw)
    grid = _run(name, search="grid", **kw)
    _assert_equal(brute, grid, name)
    assert int(brute[6][0]) == 32 and int(brute[3][0]) >= 0 and (brute[8][0] > 0).all()
    if name == "crowded":                                    # the crowded cell is reached: its rows are somebody's neighbours
        assert (brute[5][0] >= 257).sum() >= 7


# ---------------------------------------------------------------------------------------------------------------------------
# 2. against the restatement
# ---------------------------------------------------------------------------------------------------------------------------

_REF = {}


def _ref(name, H, V, seed, **kw):
    key = (name, H, V, seed, tuple(sorted(kw.items())))
    if key not in _REF:
        src, tgt, nn = _scene(name)[:3]
        _REF[key] = FM.ransac_fm_np(src, tgt, nn, TAU, H=H, V=V, seed=seed, **kw)
    return _REF[key]


def _compare_lists(got_hyp, ref, what):
    """The validated list against the restatement's, borderline hypotheses aside; -> the h both validated.  Asserts the cap of
    1 % borderline hypotheses over the range the lists cover."""
    got = [int(h) for h in got_hyp if h >= 0]
    want = [int(h) for h in ref["hyp"]]
    assert got and want, what
    upto = min(got[-1], want[-1])                             # a borderline difference shifts the lists' ends
    border = ref["prop"]["border"]
    diff = {h for h in set(got) ^ set(want) if h <= upto}
    assert all(border[h] for h in diff), (what, sorted(diff))
    assert border[:upto + 1].mean() <= 0.01, what
    return [h for h in got if h in set(want)]


@pytest.mark.parametrize("name", ["small", "mid"])
def test_against_restatement(name):
    src, tgt, nn = _scene(name)[:3]
    ns = len(src)
    H, V, seed = 3000, 32, 5
    ref = _ref(name, H, V, seed, checker_distance=TAU)
    T, fit, rmse, hyp_w, sample, nn_out, validated, hyp, count, total = [x[0].cpu().numpy() for x in
                                                                        _run(name, max_iteration=H, max_validation=V, seed=seed,
                                                                             checker_distance=TAU)]
    assert validated == V
    both = _compare_lists(hyp, ref, name)
    assert len(both) >= V - 1
    # counts: the kd-tree's on the fp64-transformed points, up to the rows within 1e-5 tau of tau; at most 0.5 % such rows
    pos_ref = {int(h): v for v, h in enumerate(ref["hyp"])}
    pos_got = {int(h): v for v, h in enumerate(hyp)}
    n_border = 0
    for h in both:
        e = ref["ev"][pos_ref[h]]
        n_border += e["border"]
        assert abs(int(count[pos_got[h]]) - e["count"]) <= e["border"], (name, h)
    assert n_border <= 0.005 * ns * len(both)
    # the winner is the argmax of the device's own scores in the total order (count larger, sum smaller, h smaller)
    order = sorted(range(V), key=lambda v: (-int(count[v]), int(total[v]), int(hyp[v])))
    h_w = int(hyp[order[0]])
    assert int(hyp_w) == h_w and count[order[0]] > 0
    assert (sample == ransac_draw(seed, 0, [h_w], ns, 4)[0]).all()
    R, t = ref["prop"]["R"][h_w], ref["prop"]["t"][h_w]
    assert np.abs(T[:3, :3] - R).max() < 1e-6 and np.abs(T[:3, 3] - t).max() < 1e-6 and (T[3] == [0, 0, 0, 1]).all()
    e = FM.evaluate(src, tgt, R, t, TAU)
    assert e["count"] == max(x["count"] for x in ref["ev"]) or e["border"] > 0
    # nn_out: the kd-tree's index, except where the two nearest tie within fp32 or the row is borderline
    sure = (e["gap"] > 1e-6) & (np.abs(e["d"] - TAU) >= FM.BORDER_ROW * TAU)
    assert sure.mean() > 0.99
    assert (nn_out[sure] == e["j"][sure]).all()
    # fitness is |C| / Ns exactly
    c = int((nn_out >= 0).sum())
    assert c == int(count[order[0]]) and fit == np.float32(c / ns)
    # inlier_rmse.  The device takes d^2 in fp32 from the fp32 pose.  Per coordinate of p = T s: the 4 pose entries are rounded
    # (each <= 2^-24 relative, times an operand of magnitude <= M) and 3 fmas round (<= 2^-24 M each), M = 3 max|s| + max|t| + ...
    # <= 3.5 bounding every partial sum here (|s_c| <= 1, |t_c| <= 0.3 + rounding): e_c <= 7 x 2^-24 x 3.5.  So d moves by at
    # most sqrt(3) e_c, plus the relative roundings of the subtraction and of the three-term d^2 (<= 4 x 2^-24 d, d < tau), and an
    # rms of distances moves by no more than the largest move.  The fp64 sum and sqrt and the final fp32 rounding (2^-24 rmse)
    # are below that.  C itself is the same set when no row is borderline, which the scene is built for.
    if e["border"] == 0:
        tol = np.sqrt(3) * 7 * 2.0 ** -24 * 3.5 + 4 * 2.0 ** -24 * TAU + 2.0 ** -23 * TAU
        want = np.sqrt(e["sum_d2"] / e["count"])
        print(f"{name}: inlier_rmse {rmse:.9g}, restatement {want:.9g}, tolerance {tol:.3g}")
        assert abs(float(rmse) - want) <= tol
        # the fixed-point sum: each row is cut to a multiple of tau^2 / 2^24, and d^2 moves by at most 2 tau x the move of d
        q = TAU * TAU / 2 ** 24
        assert abs(int(total[order[0]]) * q - e["sum_d2"]) <= e["count"] * (q + 2 * TAU * tol)
        # the same bound ties every validated hypothesis's sum to the restatement's, so the tie-break by the sum is the
        # restatement's wherever its own sums differ by more than the two bounds: the winner is the restatement's winner then
        clean = [h for h in both if ref["ev"][pos_ref[h]]["border"] == 0]
        for h in clean:
            x = ref["ev"][pos_ref[h]]
            assert abs(int(total[pos_got[h]]) * q - x["sum_d2"]) <= x["count"] * (q + 2 * TAU * tol), (name, h)
        if len(clean) == V:
            w = ref["ev"][ref["winner"]]
            rivals = [x for v, x in enumerate(ref["ev"]) if v != ref["winner"] and x["count"] == w["count"]]
            if all(x["sum_d2"] - w["sum_d2"] > 2 * w["count"] * (q + 2 * TAU * tol) for x in rivals):
                assert h_w == int(ref["hyp"][ref["winner"]]) == ref["hypothesis"]


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the first-V rule, the checkers
# ---------------------------------------------------------------------------------------------------------------------------

def test_first_v_rule():
    kw = dict(max_iteration=3000, seed=7, checker_distance=TAU)
    r64 = _run("small", max_validation=64, **kw)
    r8 = _run("small", max_validation=8, **kw)
    h64, h8 = r64[7][0], r8[7][0]
    assert int(r64[6][0]) == 64 and int(r8[6][0]) == 8
    assert (h64[1:] > h64[:-1]).all() and h64[0] >= 0
    assert torch.equal(h8, h64[:8])
    assert torch.equal(r8[8][0], r64[8][0][:8]) and torch.equal(r8[9][0], r64[9][0][:8])      # and the same scores
    stop = _run("small", max_validation=64, **dict(kw, max_iteration=int(h8[7]) + 1))
    assert int(stop[6][0]) == 8
    assert torch.equal(stop[7][0][:8], h8) and (stop[7][0][8:] == -1).all()
    assert (stop[8][0][8:] == 0).all() and (stop[9][0][8:] == 0).all()


def test_no_checker_validates_everything():
    out = _run("small", max_iteration=500, max_validation=64, seed=3)
    assert int(out[6][0]) == 64
    assert torch.equal(out[7][0].cpu(), torch.arange(64, dtype=torch.int32))
    few = _run("small", max_iteration=40, max_validation=64, seed=3)
    assert int(few[6][0]) == 40 and torch.equal(few[7][0][:40].cpu(), torch.arange(40, dtype=torch.int32))


@pytest.mark.parametrize("kw", [dict(checker_distance=TAU), dict(edge_length_threshold=0.9),
                                dict(checker_distance=0.5 * TAU, edge_length_threshold=0.95)])
def test_each_checker_removes_what_the_restatement_removes(kw):
    H = 2000                                                  # max_validation = max_iteration: the list is every passing h
    src, tgt, nn = _scene("small")[:3]
    prop = FM.propose(src, tgt, nn, 4, H, seed=9, **kw)
    out = _run("small", max_iteration=H, max_validation=H, seed=9, **kw)
    got = np.zeros(H, bool)
    hyp = out[7][0].cpu().numpy()
    got[hyp[hyp >= 0]] = True
    assert int(out[6][0]) == got.sum() and 0 < got.sum() < H
    diff = got != prop["passed"]
    assert not (diff & ~prop["border"]).any(), np.flatnonzero(diff & ~prop["border"])
    assert prop["border"].mean() <= 0.01


# ---------------------------------------------------------------------------------------------------------------------------
# 4. ragged batches, degenerate pairs
# ---------------------------------------------------------------------------------------------------------------------------

def _ragged_pairs():
    """A normal pair, one with Ns < ransac_n, one with random nn (and a tight checker: nothing passes), one of another size."""
    r = np.random.default_rng(31)
    a = _scene("small")[:3]
    few = (a[0][:3], a[1][:50], np.array([0, 1, 2]))
    rnd = (r.uniform(-1, 1, (200, 3)).astype(np.float32), r.uniform(-1, 1, (150, 3)).astype(np.float32), r.integers(0, 150, 200))
    return [a, few, rnd, _scene("mid")[:3]]


@pytest.mark.parametrize("search", ["grid", "brute"])
def test_ragged_batch_equals_single_calls(search):
    pairs = _ragged_pairs()
    soff = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])]).tolist()
    kw = dict(max_iteration=2000, max_validation=16, seed=13, checker_distance=0.02 * TAU * 4, search=search,
              return_hypotheses=True)
    S, Q, J = (_g(np.concatenate([p[k] for p in pairs])) for k in range(3))
    out = gmf_amd.ransac_feature_matching_batched(S, Q, J, TAU, source_offsets=soff, target_offsets=toff, **kw)
    for b, (s, q, j) in enumerate(pairs):
        one = gmf_amd.ransac_feature_matching_batched(_g(s)[None], _g(q)[None], _g(j)[None], TAU, first_pair=b, **kw)
        got = [out[k][b:b + 1] for k in range(5)] + [out[5][soff[b]:soff[b + 1]][None], out[6][b:b + 1]] + \
              [out[k][b:b + 1] for k in (7, 8, 9)]
        _assert_equal(got, one, f"pair {b}")
    ident = torch.eye(4, device=DEV)
    for b in (1, 2):                                         # the degenerate pairs report identity
        assert torch.equal(out[0][b], ident) and out[1][b] == 0 and out[2][b] == 0 and out[3][b] == -1
        assert (out[4][b] == -1).all() and (out[5][soff[b]:soff[b + 1]] == -1).all() and out[6][b] == 0
        assert (out[7][b] == -1).all() and (out[8][b] == 0).all()
    assert out[3][0] >= 0 and out[3][3] >= 0 and out[6][0] == 16 and out[6][3] == 16
    # first_pair is the sampler's pair index: pair 0 alone under first_pair = 3 draws other rows
    other = gmf_amd.ransac_feature_matching_batched(_g(pairs[0][0])[None], _g(pairs[0][1])[None], _g(pairs[0][2])[None], TAU,
                                                    first_pair=3, **kw)
    assert not torch.equal(other[7][0], out[7][0])


def test_pair_without_targets_and_bad_nn():
    s, q, j = _scene("small")[:3]
    S, J = _g(np.concatenate([s, s])), _g(np.concatenate([j, j]))
    out = gmf_amd.ransac_feature_matching_batched(S, _g(q), J, TAU, source_offsets=[0, 300, 600], target_offsets=[0, 257, 257],
                                                  max_iteration=500, max_validation=8, checker_distance=TAU)
    assert out[3][0] >= 0 and out[6][0] == 8
    assert torch.equal(out[0][1], torch.eye(4, device=DEV)) and out[1][1] == 0 and out[3][1] == -1 and out[6][1] == 0
    assert (out[5][300:] == -1).all()
    # an nn outside the pair's targets fails its hypotheses instead of being read
    bad = j.copy()
    bad[::2] = 257
    bad[1::4] = -1
    out = gmf_amd.ransac_feature_matching_batched(_g(s)[None], _g(q)[None], _g(bad)[None], TAU, max_iteration=2000,
                                                  max_validation=2000, return_hypotheses=True)
    ok = ((bad >= 0) & (bad < 257))[ransac_draw(0, 0, np.arange(2000), 300, 4)].all(1)
    hyp = out[7][0].cpu().numpy()
    assert (hyp[hyp >= 0] == np.flatnonzero(ok)).all() and int(out[6][0]) == ok.sum() > 0


def test_host_target_offsets_with_an_empty_pair_in_the_middle():
    """A host list of target offsets with an empty pair is uploaded like every other table (pinned, cached): the pair without
    targets reports no winner, its neighbours return what they return alone, and the second call, which finds the list in the
    cache, returns the same bits."""
    r = np.random.default_rng(41)
    tgt = r.uniform(-1, 1, (32, 3)).astype(np.float32)
    nn = np.tile(np.arange(24) % 16, 3)
    src = np.concatenate([tgt[:16][nn[:24]], tgt[:16][nn[:24]], tgt[16:][nn[:24]]]) + r.normal(0, 1e-3, (72, 3)).astype(np.float32)
    S, Q, J = _g(src.astype(np.float32)), _g(tgt), _g(nn)
    soff, toff = [0, 24, 48, 72], [0, 16, 16, 32]
    kw = dict(max_iteration=64, max_validation=8, ransac_n=3, seed=3)
    out = gmf_amd.ransac_feature_matching_batched(S, Q, J, TAU, source_offsets=soff, target_offsets=toff, **kw)
    assert torch.equal(out[0][1], torch.eye(4, device=DEV)) and out[3][1] == -1 and out[1][1] == 0 and out[2][1] == 0
    for b in (0, 2):
        one = gmf_amd.ransac_feature_matching_batched(S[soff[b]:soff[b + 1]][None], Q[toff[b]:toff[b + 1]][None],
                                                      J[soff[b]:soff[b + 1]][None], TAU, first_pair=b, **kw)
        got = [out[k][b:b + 1] for k in range(5)] + [out[5][soff[b]:soff[b + 1]][None], out[6][b:b + 1]]
        _assert_equal(got, one, f"pair {b}")
        assert out[3][b] >= 0                                # (exact correspondences up to 1e-3: a triple fits and has inliers)
    again = gmf_amd.ransac_feature_matching_batched(S, Q, J, TAU, source_offsets=soff, target_offsets=toff, **kw)
    _assert_equal(out, again, "second call")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. determinism, the seed, graph capture, a clean scene
# ---------------------------------------------------------------------------------------------------------------------------

def test_determinism_and_seed():
    kw = dict(max_iteration=3000, max_validation=32, checker_distance=TAU)
    a, b = _run("mid", seed=5, **kw), _run("mid", seed=5, **kw)
    _assert_equal(a, b)
    c = _run("mid", seed=6, **kw)
    assert not torch.equal(a[7], c[7])


def test_graph_capture_equals_eager():
    pairs = _ragged_pairs()
    soff = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])]).tolist()
    S, Q, J = (_g(np.concatenate([p[k] for p in pairs])) for k in range(3))

    def run():
        out = ()
        for search in ("grid", "brute"):
            out += gmf_amd.ransac_feature_matching_batched(S, Q, J, TAU, source_offsets=soff, target_offsets=toff,
                                                           max_iteration=2000, max_validation=16, seed=13,
                                                           checker_distance=TAU, search=search, return_hypotheses=True)
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                   # (also sizes the workspace and uploads the offsets before the capture)
            eager = [x.clone() for x in run()]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = run()
    g.replay()
    torch.cuda.synchronize()
    _assert_equal(eager, captured)


def test_clean_scene_recovers_its_pose():
    src, tgt, nn, R, t, inl = FM.make_scene(3, 1000, 777, TAU, noise=0.0)
    out = gmf_amd.ransac_feature_matching_batched(_g(src)[None], _g(tgt)[None], _g(nn)[None], TAU, checker_distance=TAU,
                                                  max_iteration=4000, max_validation=64)
    T = out[0][0].double().cpu().numpy()
    assert np.abs(T[:3, :3] - R).max() < 1e-4 and np.abs(T[:3, 3] - t).max() < 1e-4
    assert float(out[1][0]) >= inl.mean() and inl[out[4][0].cpu().numpy()].all()
    got = out[5][0].cpu().numpy()
    assert (got[inl] == nn[inl]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the open3d-shaped wrapper and the C entry
# ---------------------------------------------------------------------------------------------------------------------------

def _features(src, tgt, nn):
    """Descriptors whose nearest neighbour in feature space is `nn`: a target's descriptor is a random vector, a source row's is
    its target's plus a little noise."""
    r = np.random.default_rng(41)
    ft = r.normal(size=(len(tgt), 16)).astype(np.float32)
    fs = (ft[nn] + 0.01 * r.normal(size=(len(src), 16))).astype(np.float32)
    return fs, ft


@pytest.mark.parametrize("as_numpy", [False, True])
def test_open3d_shaped_wrapper(as_numpy):
    src, tgt, nn = _scene("small")[:3]
    fs, ft = _features(src, tgt, nn)
    assert (gmf_amd.find_knn_gpu(_g(fs), _g(ft)).cpu().numpy() == nn).all()
    conv = (lambda x: x) if as_numpy else _g
    args = (conv(src), conv(tgt), _g(fs), conv(ft), TAU)      # (one tensor names the device)
    kw = dict(checker_distance=TAU, max_iteration=3000, max_validation=32, seed=5)
    res = gmf_amd.registration_ransac_based_on_feature_matching(*args, **kw)
    core = _run("small", return_hypotheses=False, **kw)
    assert isinstance(res, gmf_amd.RegistrationResult)
    assert torch.equal(res.transformation, core[0][0])
    assert res.fitness == float(core[1][0]) and res.inlier_rmse == float(core[2][0])
    rows = torch.nonzero(core[5][0] >= 0).view(-1)
    assert res.correspondence_set.dtype == torch.int64
    assert torch.equal(res.correspondence_set, torch.stack([rows, core[5][0][rows]], 1))
    assert len(rows) == round(res.fitness * len(src))
    brute = gmf_amd.registration_ransac_based_on_feature_matching(*args, search="brute", **kw)
    assert torch.equal(brute.transformation, res.transformation) and torch.equal(brute.correspondence_set, res.correspondence_set)


def _c_args(s, q, j, V=8):
    from gmf_amd._util import handle_and_stream
    ns, nt = s.shape[0], q.shape[0]
    so = torch.tensor([0, ns], dtype=torch.int32, device=DEV)
    to = torch.tensor([0, nt], dtype=torch.int32, device=DEV)
    out = dict(T=torch.zeros((1, 4, 4), device=DEV), fit=torch.zeros(1, device=DEV), rmse=torch.zeros(1, device=DEV),
               hyp=torch.zeros(1, dtype=torch.int64, device=DEV), sample=torch.zeros((1, 4), dtype=torch.int64, device=DEV),
               nn=torch.zeros(ns, dtype=torch.int64, device=DEV), val=torch.zeros(1, dtype=torch.int32, device=DEV))
    keep = (s, q, j, so, to)
    #       0..4: src soff tgt toff nn | 5 B 6 total_src 7 total_tgt 8 max_src 9 ransac_n 10 max_iteration 11 max_validation 12 tau
    #       13 checker 14 edge 15 seed 16 first_pair 17 search | 18..24 outputs | 25..27 hyp count sum
    args = [s.data_ptr(), so.data_ptr(), q.data_ptr(), to.data_ptr(), j.data_ptr(), 1, ns, nt, ns, 4, 500, V, TAU, TAU, 0.0, 5, 0, 1,
            out["T"].data_ptr(), out["fit"].data_ptr(), out["rmse"].data_ptr(), out["hyp"].data_ptr(), out["sample"].data_ptr(),
            out["nn"].data_ptr(), out["val"].data_ptr(), None, None, None]
    h, st = handle_and_stream(s)
    return h, st, args, out, keep


def test_c_abi_entry():
    src, tgt, nn = _scene("small")[:3]
    s, q, j = _g(src), _g(tgt), _g(nn)
    want = _run("small", max_iteration=500, max_validation=8, seed=5, checker_distance=TAU, return_hypotheses=False)
    for search in (0, 1):
        h, st, args, out, keep = _c_args(s, q, j)
        args[17] = search
        h.call("gmf_ransac_feature_matching", *args, st)      # hyp / count / sum are optional
        got = (out["T"], out["fit"], out["rmse"], out["hyp"], out["sample"], out["nn"][None], out["val"])
        _assert_equal(got, want, f"search={search}")
    # max_src only sizes the launch: a value below the pair's rows (or 0, unknown) gives the same bits
    for max_src in (1, 0, 256):
        h, st, args, out, keep = _c_args(s, q, j)
        args[8] = max_src
        h.call("gmf_ransac_feature_matching", *args, st)
        got = (out["T"], out["fit"], out["rmse"], out["hyp"], out["sample"], out["nn"][None], out["val"])
        _assert_equal(got, want, f"max_src={max_src}")
    h, st, args, out, keep = _c_args(s, q, j)

    def put(k, v):
        return args[:k] + [v] + args[k + 1:]

    bad = [
        (put(0, None), -1, "null pointer"), (put(4, None), -1, "null pointer"), (put(24, None), -1, "null pointer"),
        (put(5, 0), -2, "empty batch"), (put(6, 1 << 31), -2, "empty batch"),
        (put(7, 0), -2, "total_tgt"), (put(7, 1 << 31), -2, "total_tgt"), (put(7, 1 << 29), -2, "fewer than 2\\^29"),
        (put(9, 2), -1, "ransac_n"), (put(9, 9), -1, "ransac_n"),
        (put(10, 0), -1, "max_iteration"), (put(10, (1 << 24) + 1), -1, "max_iteration"),
        (put(11, 0), -1, "max_validation"), (put(11, 65537), -1, "max_validation"),
        (put(12, 0.0), -1, "max_correspondence_distance"), (put(13, float("nan")), -1, "checker_distance"),
        (put(14, 1.5), -1, "edge_length_threshold"), (put(16, -1), -1, "first_pair"),
        (put(17, 2), -1, "search must be"),
    ]
    for a, code, msg in bad:
        with pytest.raises(RuntimeError, match=rf"status {code}\b.*ransac_feature_matching.*" + msg):
            h.call("gmf_ransac_feature_matching", *a, st)
    gmf_amd.check_status()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. DGR's safeguard branch (the synthetic checkpoint of tests/test_gpu_fcgf.py)
# ---------------------------------------------------------------------------------------------------------------------------

_NC = {"feat_model": "ResUNetBN2C", "feat_model_n_out": 32, "bn_momentum": 0.05, "feat_conv1_kernel_size": 7,
       "normalize_feature": True, "inlier_model": "ResUNetBN2C", "inlier_conv1_kernel_size": 3, "inlier_feature_type": "ones",
       "voxel_size": 0.0625, "nn_max_n": 500}
_STATE = {}


def _quantized_cloud():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
    return (np.round(z["cloud0"].astype(np.float64) * 1024) / 1024).astype(np.float32)


def _voxel_coords(xyz, v, batch):
    x = _g(xyz)
    c = torch.floor(x[gmf_amd.voxel_select(x, v)].double() / v).int()
    return torch.cat([torch.full((len(c), 1), batch, dtype=torch.int32, device=DEV), c], 1)


def _dgr(clip):
    """The synthetic checkpoint of tests/test_gpu_fcgf.py: a conditioned FCGF and an inlier network whose every logit is 4."""
    v = _NC["voxel_size"]
    if "fcgf" not in _STATE:
        xyz = _quantized_cloud()
        coords = torch.cat([_voxel_coords(xyz, v, 0), _voxel_coords(xyz + 0.5, v, 1)]).cpu().numpy()
        torch.manual_seed(5)
        m = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=7, normalize_feature=True, D=3)
        _STATE["fcgf"] = FR.conditioned_state_dict(m, coords, torch.ones(len(coords), 1))
        torch.manual_seed(6)
        sd = gmf_amd.ResUNetBN2C(1, 1, D=6, pe=True).state_dict()
        sd["final.kernel"] = torch.zeros_like(sd["final.kernel"])
        sd["final.bias"] = torch.full_like(sd["final.bias"], 4.0)
        _STATE["inlier"] = sd
        g = torch.Generator().manual_seed(9)
        _STATE["tokens"] = (_g(torch.randn(1, 80, 128, generator=g)), _g(torch.randn(1, 80, 128, generator=g)))
    state = {"config": types.SimpleNamespace(**_NC), "state_dict": _STATE["fcgf"], "state_dict_inlier": _STATE["inlier"]}
    return dgr.DeepGlobalRegistration({"clip_weight_thresh": clip}, device=DEV, state=state)


def _dgr_clouds():
    xyz0 = _quantized_cloud()
    t_true = np.array([8, 16, -8], np.float64) * _NC["voxel_size"]
    return xyz0, xyz0 + t_true.astype(np.float32), t_true


@pytest.mark.parametrize("clip", [0.05, 1.0])
def test_dgr_default_is_the_correspondence_safeguard(clip):
    xyz0, xyz1, _ = _dgr_clouds()
    d = _dgr(clip)
    assert d.safeguard_method == "correspondence"
    pt, qt = _STATE["tokens"]
    T0 = d.register(xyz0, xyz1, p_tokens=pt, q_tokens=qt)    # the attribute not touched
    stats0 = dict(d.last_stats)
    d.safeguard_method = "correspondence"
    T1 = d.register(xyz0, xyz1, p_tokens=pt, q_tokens=qt)
    assert np.array_equal(T0, T1) and d.last_stats == stats0
    assert stats0["branch"] == ("safeguard" if clip == 1.0 else "global_registration")
    assert set(stats0) == {"wsum", "wsum_threshold", "global_registration", "num_correspondences", "branch"}
    if clip == 1.0:                                          # and the branch is the parent's call, argument for argument
        p0, p1 = d.preprocess(xyz0)[0], d.preprocess(xyz1)[0]
        i0, i1 = d.correspondences(*d.features(d.preprocess(xyz0)[1], d.preprocess(xyz1)[1]))
        want = gmf_amd.registration_ransac_based_on_correspondence(p0, p1, torch.stack([i0, i1], 1), 2 * _NC["voxel_size"],
                                                                   ransac_n=4, max_iteration=4000000, max_validation=80000)
        assert np.array_equal(d.safeguard_registration(p0, p1, i0, i1), want.transformation.double().cpu().numpy())


def test_dgr_feature_matching_safeguard():
    xyz0, xyz1, t_true = _dgr_clouds()
    d = _dgr(1.0)                                            # the clip zeroes every weight: wsum = 0 < its threshold
    d.safeguard_method = "fcgf_feature_matching"
    d.use_icp = False
    pt, qt = _STATE["tokens"]
    T = d.register(xyz0, xyz1, p_tokens=pt, q_tokens=qt)
    assert d.last_stats["branch"] == "safeguard" and d.last_stats["wsum"] == 0.0
    assert d.last_stats["wsum"] < d.last_stats["wsum_threshold"]
    # a direct call of the batched core on the same inputs
    p0, c0 = d.preprocess(xyz0)
    p1, c1 = d.preprocess(xyz1)
    F0, F1 = d.features(c0, c1)
    _, idx1 = d.correspondences(F0, F1)
    tau = 2 * _NC["voxel_size"]
    want = gmf_amd.ransac_feature_matching_batched(p0[None], p1[None], idx1[None], tau, ransac_n=4, checker_distance=tau,
                                                   max_iteration=80000, max_validation=1000)
    assert np.array_equal(T, want[0][0].double().cpu().numpy())
    assert int(want[6][0]) == 1000 and float(want[1][0]) > 0.9
    assert np.abs(T[:3, :3] - np.eye(3)).max() < 1e-4 and np.abs(T[:3, 3] - t_true).max() < 1e-3
    d.use_icp = True                                         # and ICP follows it as it follows the other safeguard
    T2 = d.register(xyz0, xyz1, p_tokens=pt, q_tokens=qt)
    assert np.abs(T2[:3, 3] - t_true).max() < 1e-3


def test_dgr_unknown_safeguard_method_raises():
    xyz0, xyz1, _ = _dgr_clouds()
    d = _dgr(1.0)
    d.safeguard_method = "fpfh_feature_matching"
    pt, qt = _STATE["tokens"]
    with pytest.raises(ValueError, match="safeguard_method"):
        d.register(xyz0, xyz1, p_tokens=pt, q_tokens=qt)
    with pytest.raises(ValueError, match="safeguard_method"):
        d.safeguard_registration(None, None, None, None)
