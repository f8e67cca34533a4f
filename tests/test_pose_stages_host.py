"""The conditions under which tests/test_gpu_pose_stages.py means something, checked from the reference alone (CPU, float32 and
float64 evaluations of tests/pose_stage_reference.py on the reference's own exact kNN).  If a scene misses a condition, its seed
or noise level changes - not the condition.

  1. stop index      float32 and float64 traces stop at the same index, and up to it |gap64| >= 4 max|v32 - v64|: the exit is
                     not near its threshold, a device that stops elsewhere is wrong
  2. conditioning    at most 5 % of a case's seeds (none in a clean scene) have a float32 reference further than 1e-4 gmax from
                     the float64 one; those are excluded from the `seed_trans` comparison
  3. band            at most 10 % of a case's hypotheses have a float64 residual within `band` of the threshold
  4. plateau         >= 8 seeds share the maximal float64 inlier count without a band point, and their transforms differ
  5. refinement      every step of every refinement scene keeps 4 bands from the threshold (so every count, and with it the
                     exit decision, is the same in fp32), and the float32 count sequence is the float64 one

and what the scenes have to tell apart: a solve from the iterate before the last one (noisy scenes), a refinement that stops at
a count that did not grow (shrinking scene), the arithmetic the planted threshold cases rely on.

k = 2 is the one case conditions 1 and 2 cannot hold for: M is [[0, m], [m, 0]], H has rank <= 1, and the rotation about the
axis through the two neighbours is free - common.py's SVD returns some rotation, and so does the device.  There the tests ask
for what IS defined (see test_k2_is_rank_one)."""
import numpy as np
import pytest
import torch

import pose_stage_reference as P
from test_train_gradients import ABS_G, FLOOR_MULT, REL

F64, F32 = P.F64, P.F32
CASES = P.trans_cases()


@pytest.fixture(scope="module")
def evaluated():
    """name -> (T32, T64, stops32, stops64, gaps64, traces32, traces64) on the reference's own neighbours, computed once."""
    out = {}
    for name, case in CASES.items():
        knn = P.reference_knn(case)
        T64, st64, g64, tr64 = P.reference_transforms(case, knn, F64)
        T32, st32, _, tr32 = P.reference_transforms(case, knn, F32)
        out[name] = (T32, T64, st32, st64, g64, tr32, tr64)
    return out


def test_case_shapes():
    """The shapes the GPU tests rely on: 63 flags in B.2 and 189 in its tail variant (neither a multiple of 16), ragged seed
    counts that differ, k + 1 = N in the `all` cases, 1 <= S."""
    for k in (40, 41):
        assert CASES[f"B2-k{k}"]["seeds"].numel() * CASES[f"B2-k{k}"]["iters"] == 63
        assert CASES[f"B2-tail-k{k}"]["seeds"].numel() * CASES[f"B2-tail-k{k}"]["iters"] == 189
        assert CASES[f"B-copies-k{k}"]["seeds"].numel() * CASES[f"B-copies-k{k}"]["iters"] == 210
        assert [len(s) for s in CASES[f"B3-k{k}"]["seeds"]] == [13, 17, 25]
    for k in (40, 64):
        assert CASES[f"A-k{k}-all"]["scenes"][0]["src"].shape[0] == k + 1
    for S, N in ((13, 130), (7, 130), (13, 41), (13, 65), (1050, 2100), (30, 300), (65, 300), (1, 300)):
        assert int(N * P.ratio_for(S, N)) == S


@pytest.mark.parametrize("name", [n for n in CASES if n != "A-k2"])
def test_condition_1_stop_index(evaluated, name):
    T32, T64, st32, st64, g64, tr32, tr64 = evaluated[name]
    assert st32 == st64, f"{name}: float32 stops at {st32}, float64 at {st64}"
    for b in range(len(T64)):
        dv = (tr32[b].to(F64) - tr64[b]).abs().flatten(1).max(dim=1)[0]
        assert bool((g64[b].abs() >= 4 * dv).all()), f"{name}: pair {b}: |gap64| {g64[b].tolist()} against max|v32 - v64| {dv.tolist()}"
        assert bool((g64[b][:-1] > 0).all())                                    # not taken before the stop ...
        if st64[b] < CASES[name]["iters"] - 1:
            assert float(g64[b][-1]) <= 0                                       # ... and taken at it


def test_stop_indices_cover_every_resolution():
    """What the cases are for: clean pairs take the exit early, noisy ones never; B.2 spans the batch, B.3 does not."""
    ev = {n: P.reference_transforms(c, P.reference_knn(c), F64)[1] for n, c in CASES.items() if n.startswith(("B1", "B2", "B3", "B-it64", "B-copies"))}
    for k in (40, 41):
        assert ev[f"B1-clean-k{k}"][0] < 9 and ev[f"B1-noisy-k{k}"] == [9]
        assert ev[f"B2-k{k}"] == [2, 2, 2] and ev[f"B2-tail-k{k}"] == [8, 8, 8]
        st = ev[f"B3-k{k}"]
        assert st[0] < 9 and st[1] == 9 and st[2] < 9
        assert ev[f"B-it64-k{k}"][0] < 63 and ev[f"B-it64-k{k}-B2"][0] < 63
        assert 2 <= ev[f"B-copies-k{k}"][0] < 9


@pytest.mark.parametrize("name", [n for n in CASES if n != "A-k2"])
def test_condition_2_conditioning(evaluated, name):
    T32, T64 = evaluated[name][:2]
    ill, floors, gmax = P.ill_conditioned(T32, T64)
    n_ill, n = sum(int(m.sum()) for m in ill), sum(m.numel() for m in ill)
    assert n_ill <= P.ILL_CAP * n, f"{name}: {n_ill} of {n} seeds are ill-conditioned"
    for kind, m in zip(CASES[name]["kinds"], ill):
        if kind == "clean":
            assert not bool(m.any()), name


def test_k2_is_rank_one(evaluated):
    """k = 2: every seed whose float32 reference misses the float64 one has an H of rank one up to the 1e-6 in the centroids'
    denominators (second singular value below 1e-9 of the first) - its rotation is not unique, the miss is not noise - and every other seed has zero weights (M = 0:
    both references give the identity).  The GPU test asks such seeds for what is defined: a rotation matrix that takes the
    weighted source centroid to the target centroid and the source direction to the target direction."""
    case = CASES["A-k2"]
    T32, T64 = evaluated["A-k2"][:2]
    ill = P.ill_conditioned(T32, T64)[0][0]
    f, s, t = (P.stack(case["scenes"], key).to(F64) for key in ("feat_n", "src", "tgt"))
    H, w = P.kabsch_moments(f, s, t, P.reference_knn(case), case["iters"], "pair")[2:]
    sv = torch.linalg.svdvals(H[0])
    assert bool((sv[:, 1] <= 1e-9 * sv[:, 0]).all())
    assert bool(ill.any())
    for i in range(len(ill)):
        if not bool(ill[i]):
            assert float(w[0, i].abs().max()) == 0 and torch.equal(T64[0][i], torch.eye(4, dtype=F64))


def _bound(floor, gmax):
    return torch.clamp(FLOOR_MULT * floor, min=REL * gmax) + ABS_G * gmax


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if "noisy" in c["kinds"] and c["k"] > 2 and c["iters"] == 3])
def test_noisy_scenes_tell_the_iterates_apart(name):
    """A device that solves from the iterate BEFORE the one the reference stops at must miss bound A: in every noisy pair
    whose exit is never taken, at least half of the seeds move by more than 4 x the bound between those two iterates."""
    case = CASES[name]
    knn = P.reference_knn(case)
    T64 = P.reference_transforms(case, knn, F64)[0]
    T32 = P.reference_transforms(case, knn, F32)[0]
    early = dict(case, iters=case["iters"] - 1)
    Te = P.reference_transforms(early, knn, F64)[0]
    _, floors, gmax = P.ill_conditioned(T32, T64)
    for b, kind in enumerate(case["kinds"]):
        if kind == "noisy":
            moved = P.seed_floor(Te[b], T64[b]) > 4 * _bound(floors[b], gmax)
            assert int(moved.sum()) * 2 >= moved.numel(), f"{name}: pair {b}: {int(moved.sum())} of {moved.numel()} seeds"


@pytest.mark.parametrize("k", [40, 41])
def test_tail_seed_holds_the_exit(k):
    """B2-tail: every seed but the last one of the last pair passes the exit test at some iterate before the last, the last
    one never does (the batch's stop is the last iterate because of flags behind the last whole 16-byte piece alone: bytes
    176 .. 188 of 189 belong to the last two seeds), and its transform at the iterate the others pass at is far from the
    reference: a stop taken without those flags misses bound A."""
    case = CASES[f"B2-tail-k{k}"]
    knn = P.reference_knn(case)
    T64, stops, _, traces = P.reference_transforms(case, knn, F64)
    V = torch.cat(traces, dim=1)                                                   # [iters, B S, k]
    prev = torch.cat([torch.ones_like(V[:1]), V[:-1]])
    ok = ((V - prev).abs() <= 1e-8 + 1e-5 * prev.abs()).all(-1)                    # [iters, B S]
    first = [int(ok[:, i].nonzero()[0]) if bool(ok[:, i].any()) else -1 for i in range(ok.shape[1])]
    assert first[-1] == -1 and all(0 <= f < case["iters"] - 1 for f in first[:-1]) and stops == [8, 8, 8]
    all_but_last = max(first[:-1])
    assert bool(ok[all_but_last:, :-1].all())
    T32 = P.reference_transforms(case, knn, F32)[0]
    _, floors, gmax = P.ill_conditioned(T32, T64)
    for it in range(all_but_last, case["iters"] - 1):                              # whichever earlier iterate it would take
        Te = P.reference_transforms(dict(case, iters=it + 1), knn, F64)[0]
        assert float(P.seed_floor(Te[2][-1], T64[2][-1])) > 4 * float(_bound(floors[2][-1], gmax)), it


# ---- scoring, argmax ------------------------------------------------------------------------------------------------------------
def _score_reference(sc, seeds, k=40, iters=10):
    f, s, t = sc["feat_n"][None], sc["src"][None], sc["tgt"][None]
    knn = P.exact_knn(f, seeds, k)
    T64 = P.seed_transforms(f.to(F64), s.to(F64), t.to(F64), knn, P.SIGMA, P.SIGMA_D, iters, "pair")[0]
    r = P.residuals(T64, s, t)[0]
    return T64[0], r, P.band(s, t, T64)


def _score_cases():
    cases = [(f"S{S}", P.plateau(300, 0), S) for S in P.SCORE_S] + [(f"N{N}", P.plateau(N, 0), 30) for N in P.SCORE_N]
    cases += [(f"argmax{N}", P.plateau(N, 0), S) for N, S in P.ARGMAX_CASES]
    return [(name, sc, P.plateau_seeds(sc, S, 0)[None]) for name, sc, S in cases] + \
           [("scatter",) + P.scatter()]


@pytest.mark.parametrize("name,sc,seeds", _score_cases(), ids=[c[0] for c in _score_cases()])
def test_condition_3_and_4_band_and_plateau(name, sc, seeds):
    T64, r, bd = _score_reference(sc, seeds)
    in_band = ((r - P.TAU).abs() <= bd).any(-1)
    assert int(in_band.sum()) <= 0.10 * len(in_band), f"{name}: {int(in_band.sum())} of {len(in_band)} hypotheses have a band point"
    if name.startswith("argmax"):
        cnt = (r < P.TAU).sum(-1)
        top = ((cnt == cnt.max()) & ~in_band).nonzero()[:, 0]
        assert len(top) >= 8 and int(top[0]) == 1, f"{name}: {len(top)} seeds share the maximum, the first one at {int(top[0])}"
        assert len(cnt) <= 1025 or 1025 in top.tolist()          # (the second seed of the thread that holds the first maximum)
        assert len({T64[i].numpy().tobytes() for i in top.tolist()}) > 1
        assert not bool(in_band[cnt == cnt.max()].any())


def test_condition_3_ragged_plateau():
    for b, (n, seeds) in enumerate(zip(P.RAGGED_SIZES, P.top_seeds(P.ragged_logits(P.RAGGED_SIZES, 3), P.RAGGED_SIZES, P.RAGGED_RATIO))):
        _, r, bd = _score_reference(P.plateau(n, 10 + b), seeds[None])
        in_band = ((r - P.TAU).abs() <= bd).any(-1)
        assert int(in_band.sum()) <= 0.10 * len(in_band), b


def test_scatter_scene_spreads_the_counts():
    """The plateau counts are all-or-nothing; `scatter` (a third of the targets displaced by about the threshold) is the scene
    whose hypotheses take several different counts, none of them trivial, some with a band point.  Its best hypothesis leads
    by two inliers, and the refinement from it (here: from the float32 reference's) takes at least three steps, each of them
    4 bands from the threshold."""
    sc, seeds = P.scatter()
    f, s, t = sc["feat_n"][None], sc["src"][None], sc["tgt"][None]
    T32 = P.seed_transforms(f, s, t, P.exact_knn(f, seeds, 40), P.SIGMA, P.SIGMA_D, 10, "pair")[0]
    r, bd = P.residuals(T32, s, t)[0], P.band(s, t, T32)
    cnt = (r < P.TAU).sum(-1)
    assert len(set(cnt.tolist())) >= 5 and 0 < int(cnt.min()) and int(cnt.max()) < 300
    assert bool(((r - P.TAU).abs() <= bd).any())
    top = cnt.sort(descending=True)[0]
    assert int(top[0] - top[1]) >= 2
    T0 = T32[0, int(cnt.argmax())][None]
    _, cs, ms = P.refine(T0.to(F64), s.to(F64), t.to(F64), P.TAU)
    assert len(cs[0]) >= 3 and min(ms[0]) > 4 * bd and not bool(((r[int(cnt.argmax())] - P.TAU).abs() <= bd).any())


# ---- refinement -----------------------------------------------------------------------------------------------------------------
def _refine_scenes():
    return [(f"N{N}", P.refine_scene(N, seed)) for N, seed in P.REFINE_SEEDS.items()] + \
           [(f"batch{seed}", P.refine_scene(257, seed)) for seed in P.REFINE_BATCH] + [("shrinking", P.shrinking_scene(P.SHRINKING_SEED))]


@pytest.mark.parametrize("name,sc", _refine_scenes(), ids=[c[0] for c in _refine_scenes()])
def test_condition_5_refinement_counts(name, sc):
    T0, s, t = sc["T0"][None], sc["src"][None], sc["tgt"][None]
    _, cs64, ms = P.refine(T0.to(F64), s.to(F64), t.to(F64), P.TAU)
    _, cs32, _ = P.refine(T0, s, t, P.TAU)
    assert cs32 == cs64 and len(cs64[0]) >= 3, (cs32, cs64)
    assert min(ms[0]) > 4 * P.band(s, t, T0), f"{name}: a residual {min(ms[0]):.3e} from the threshold, band {P.band(s, t, T0):.3e}"
    assert cs64[0][-1] == cs64[0][-2] and len(cs64[0]) < 20                 # the exit is taken, on an unchanged count


def test_shrinking_seed_is_the_first_and_tells_the_exits_apart():
    """The committed seed is what the search over 0 .. 999 finds, its float64 count sequence goes down at a step the loop
    continues behind (so does REFINE_BATCH's third scene), and a loop that stops at a count that did not grow returns a
    transform more than 4 x bound A's tolerance away."""
    assert P.find_shrinking_seed() == P.SHRINKING_SEED
    for sc in (P.shrinking_scene(P.SHRINKING_SEED), P.refine_scene(257, P.REFINE_BATCH[2])):
        T0, s, t = sc["T0"][None], sc["src"][None], sc["tgt"][None]
        T64, cs, _ = P.refine(T0.to(F64), s.to(F64), t.to(F64), P.TAU)
        assert P.counts_shrink(cs[0]), cs
        T32 = P.refine(T0, s, t, P.TAU)[0]
        Tw = P.refine(T0.to(F64), s.to(F64), t.to(F64), P.TAU, exit_when_not_growing=True)[0]
        gmax = float(T64.abs().max())
        assert float(P.seed_floor(Tw, T64)) > 4 * float(_bound(P.seed_floor(T32, T64), gmax))


def test_planted_threshold_arithmetic():
    """What the planted cases rely on, in IEEE float32: sqrt(fl(d d)) == d for d = float32(0.1) and its predecessor, so a point
    at distance d from a source at the origin under the identity has the fp32 residual d exactly: not below the threshold at
    d = float32(0.1), below it one ulp lower.  And for the scoring (which compares squared distances with the smallest float
    whose root reaches tau): at tau = 0.25 that float is 0.0625 = fl(0.25^2) itself."""
    thr = np.float32(0.1)
    below = np.nextafter(thr, np.float32(0))
    for d in (thr, below):
        assert np.sqrt(np.float32(d * d), dtype=np.float32) == d
    assert not thr < thr and below < thr and float(below) < 0.1 <= float(thr)
    q = np.float32(0.0625)
    assert np.float32(0.25) * np.float32(0.25) == q and np.sqrt(q) == np.float32(0.25)
    assert np.sqrt(np.nextafter(q, np.float32(0))) < np.float32(0.25)
    b = np.nextafter(np.float32(0.25), np.float32(0))
    assert np.float32(b * b) < q


def test_zero_inlier_start():
    sc = P.refine_scene(257, 0)
    T0 = sc["T0"].clone()
    T0[:3, 3] += 10.0
    _, cs, ms = P.refine(T0[None].to(F64), sc["src"][None].to(F64), sc["tgt"][None].to(F64), P.TAU)
    assert cs == [[0]] and ms[0][0] > 1.0
