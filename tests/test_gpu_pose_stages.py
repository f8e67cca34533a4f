"""The forward pose head, stage by stage, against the float64 evaluation of the oracle's own functions.

k_seed_power / k_stop_iteration / k_seed_kabsch (`seed_trans`), k_score_hyp (`fitness`), k_finalize_pose (argmax, labels,
refinement) and k_post_refine are each fed the DEVICE's output of the stage before (its kNN, its transforms, its fitness), so a
discrete choice of one stage cannot excuse an error of the next.  The inputs are the scenes of tests/pose_stage_reference.py;
tests/test_pose_stages_host.py shows from the reference alone that on them every discrete decision (stop index, inlier counts,
the refinement's exit) is far from its threshold.

  A  seed_trans at every k that takes another branch of the Gram tiles / the row length of the power iteration
  B  the stop iteration resolved by k_seed_kabsch (one pair), by k_stop_iteration (uniform batch; 63 and 189 flags: the scalar
     tail) and per pair (ragged batch), and num_iterations 1, 2, 64
  C  fitness * N == the float64 inlier count of the device's own transforms, at every S around the 8-hypothesis groups
  D  first index of the maximum, labels, train-mode output
  E  refinement (stand-alone and inside k_finalize_pose), with planted points exactly at the threshold
  F  repeatability

Bound A, the project's existing one (tests/test_train_gradients.py): per seed max|hip - T64| <= max(4 floor_s, 2e-5 gmax) +
3e-6 gmax with floor_s = max|T32 - T64| of the reference's own float32 evaluation.  `pytest -s` prints the worst err / tol of
every case.  k = 2 is the one case whose rotation is not defined (two neighbours: H has rank one, see the host tests); there
the seeds with non-zero weights are asked for what is defined."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import _lib

import pose_stage_reference as P
from test_train_gradients import ABS_G, FLOOR_MULT, REL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = P.F64, P.F32
CASES = P.trans_cases()


@functools.lru_cache(maxsize=None)
def _model(k, iters, ratio, tau=P.TAU):
    """(the weights are irrelevant: pose_head gets the sigmas, the features and the seeds)"""
    return gmf_amd.PointDSC(in_dim=6, num_layers=1, num_channels=128, num_iterations=iters, ratio=ratio, inlier_threshold=tau,
                            sigma_d=P.SIGMA_D, k=k, nms_radius=0.10)


def _dev(x):
    return x.to(DEV).contiguous()


def _head(scenes, seeds, k, iters, testing=False, tau=P.TAU, logits=None, ratio=None):
    """One gmf_pose_head call on stacked scenes: seeds [B,S] given, or taken from `logits` (top-S, no NMS: testing=False)."""
    f, s, t = (_dev(P.stack(scenes, key)) for key in ("feat_n", "src", "tgt"))
    B, N, _ = f.shape
    if seeds is not None:
        ratio = P.ratio_for(seeds.shape[1], N)
    lg = torch.zeros(B, N, device=DEV) if logits is None else _dev(logits)
    final, labels, aux = _model(k, iters, ratio, tau).pose_head(f, s, t, lg, testing=testing, seeds=None if seeds is None else _dev(seeds),
                                                                return_aux=True, sigmas=(P.SIGMA, P.SIGMA_D))
    torch.cuda.synchronize()
    gmf_amd.check_status()
    return {"final": final.cpu(), "labels": labels.cpu(), "knn": aux["knn_idx"].cpu(), "T": aux["seed_trans"].cpu(),
            "fit": aux["fitness"].cpu(), "seeds": aux["seeds"].cpu()}


def _head_ragged(scenes, logits, k, iters, ratio, tau=P.TAU, refine_iters=0):
    """gmf_pose_head_ragged with all four optional outputs; seeds = the top int(n ratio) logits of each pair (no NMS)."""
    sizes = [sc["src"].shape[0] for sc in scenes]
    total, B, S_max = sum(sizes), len(sizes), int(max(sizes) * ratio)
    cat = lambda key: _dev(torch.cat([sc[key] for sc in scenes]))
    f, s, t, lg = cat("feat_n"), cat("src"), cat("tgt"), _dev(logits)
    pp = _lib.PoseParams()
    pp.num_seeds, pp.k, pp.num_iterations, pp.use_nms, pp.refine_iters = S_max, k, iters, 0, refine_iters
    pp.sigma, pp.sigma_d, pp.inlier_threshold, pp.nms_radius, pp.refine_threshold = P.SIGMA, P.SIGMA_D, tau, 0.10, 0.10
    final, labels = torch.full((B, 16), -7.0, device=DEV), torch.full((total,), -7.0, device=DEV)
    seeds = torch.full((B, S_max), -1, dtype=torch.int32, device=DEV)
    knn = torch.full((B, S_max, k), -1, dtype=torch.int32, device=DEV)
    sT, fit = torch.full((B, S_max, 16), -7.0, device=DEV), torch.full((B, S_max), -7.0, device=DEV)
    h, st = _lib.handle_for(0), torch.cuda.current_stream().cuda_stream
    h.call("gmf_pose_head_ragged", pp, ratio, f.data_ptr(), s.data_ptr(), t.data_ptr(), lg.data_ptr(), (ctypes.c_int * B)(*sizes), B,
           final.data_ptr(), labels.data_ptr(), seeds.data_ptr(), knn.data_ptr(), sT.data_ptr(), fit.data_ptr(), st)
    torch.cuda.synchronize()
    gmf_amd.check_status()
    return {"final": final.cpu().reshape(B, 4, 4), "labels": labels.cpu(), "knn": knn.cpu(), "T": sT.cpu().reshape(B, S_max, 4, 4),
            "fit": fit.cpu(), "seeds": seeds.cpu(), "sizes": sizes}


def _bound(floor, gmax):
    return torch.clamp(FLOOR_MULT * floor, min=REL * gmax) + ABS_G * gmax


def _check_bound_a(name, case, got_T, got_knn):
    """got_T / got_knn: per pair [S_b,4,4] float32 / [S_b,k] of the device.  The reference runs on the device's neighbours with
    the case's span; condition 2 is re-evaluated on them (same cap).  Prints and returns the worst err / tol."""
    knn = [nb.long() for nb in got_knn] if case["form"] == "ragged" else torch.stack(list(got_knn)).long()
    T64 = P.reference_transforms(case, knn, F64)[0]
    T32 = P.reference_transforms(case, knn, F32)[0]
    ill, floors, gmax = P.ill_conditioned(T32, T64)
    n_ill, n = sum(int(m.sum()) for m in ill), sum(m.numel() for m in ill)
    assert n_ill <= P.ILL_CAP * n, f"{name}: {n_ill} of {n} seeds are ill-conditioned on the device's neighbours"
    worst = 0.0
    for b, (g, r, fl, m) in enumerate(zip(got_T, T64, floors, ill)):
        assert bool(torch.isfinite(g).all()), f"{name}: pair {b}: non-finite seed_trans"
        assert torch.equal(g[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(len(g), 4)), f"{name}: pair {b}: last row"
        ratio = (P.seed_floor(g, r) / _bound(fl, gmax))[~m]
        if ratio.numel():
            worst = max(worst, float(ratio.max()))
            assert float(ratio.max()) <= 1.0, (f"{name}: pair {b}: seed {int(ratio.argmax())} (of the well-conditioned ones) misses bound A: "
                                               f"err / tol = {float(ratio.max()):.3g}; all: {[round(float(x), 3) for x in ratio]}")
    print(f"[pose stages] {name}: worst err / tol = {worst:.3f} ({n_ill} of {n} seeds excluded)")
    return worst


def _run_case(name):
    case = CASES[name]
    if case["form"] == "ragged":
        out = _head_ragged(case["scenes"], P.ragged_logits(P.RAGGED_SIZES, case["k"]), case["k"], case["iters"], P.RAGGED_RATIO)
        for b, sd in enumerate(case["seeds"]):
            assert torch.equal(out["seeds"][b, :len(sd)], sd), f"{name}: pair {b}: the seeds are not the top logits"
        return out, [out["T"][b, :len(sd)] for b, sd in enumerate(case["seeds"])], [out["knn"][b, :len(sd)] for b, sd in enumerate(case["seeds"])]
    out = _head(case["scenes"], case["seeds"], case["k"], case["iters"])
    assert torch.equal(out["seeds"], case["seeds"])
    return out, list(out["T"]), list(out["knn"])


# ---- A. compatibility matrix, power iteration, weights, Kabsch ---------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("A-") and n not in ("A-k1", "A-k2")])
def test_a_seed_trans(name):
    """k = 31 / 32 / 33: one Gram tile or three, one row of the second fragment; 40 / 41: the row length of the power iteration;
    48, 63, 64: one and two register groups of the lower tiles, every lane a neighbour; `all`: N = k + 1."""
    _, T, knn = _run_case(name)
    case = CASES[name]
    N = case["scenes"][0]["src"].shape[0]
    assert knn[0].shape == (13, min(case["k"], N - 1)) and int(knn[0].min()) >= 0 and int(knn[0].max()) < N
    _check_bound_a(name, case, T, knn)


def test_a_k1_identity():
    """k = 1: M is the 1 x 1 zero matrix, every weight is zero and every transform is the identity, as the float64 reference
    gives it (H = 0); every entry is finite."""
    case = CASES["A-k1"]
    _, T, knn = _run_case("A-k1")
    T64 = P.reference_transforms(case, torch.stack(knn).long(), F64)[0][0]
    assert torch.equal(T64, torch.eye(4, dtype=F64).expand(13, 4, 4))
    assert bool(torch.isfinite(T[0]).all())
    assert torch.equal(T[0], torch.eye(4).expand(13, 4, 4)), T[0]


def test_a_k2_defined_part():
    """k = 2: H has rank one and the rotation about the axis through the two neighbours is free (the float32 and float64
    references disagree on it: host test test_k2_is_rank_one).  Defined, and asked here within bound A's tolerance without a
    floor: seeds with zero weights give the identity; the others a proper rotation that takes the weighted source centroid to
    the target centroid and the direction between the source neighbours to the one between the target neighbours."""
    case = CASES["A-k2"]
    _, T, knn = _run_case("A-k2")
    f, s, t = (P.stack(case["scenes"], key).to(F64) for key in ("feat_n", "src", "tgt"))
    nb = torch.stack(knn).long()
    ca, cb, H, w = (x[0] for x in P.kabsch_moments(f, s, t, nb, case["iters"], "pair"))
    g = T[0].to(F64)
    assert bool(torch.isfinite(g).all())
    gmax = max(1.0, float(cb.abs().max()))
    tol = (REL + ABS_G) * gmax
    worst, live = 0.0, 0
    for i in range(len(g)):
        R, tt = g[i, :3, :3], g[i, :3, 3]
        if float(w[i].abs().max()) == 0:
            assert torch.equal(T[0][i], torch.eye(4)), i
            continue
        live += 1
        a, b = s[0, nb[0, i]], t[0, nb[0, i]]
        da, db = (a[0] - a[1]) / (a[0] - a[1]).norm(), (b[0] - b[1]) / (b[0] - b[1]).norm()
        errs = [float((R @ R.t() - torch.eye(3, dtype=F64)).abs().max()), abs(float(torch.det(R)) - 1.0),
                float((R @ ca[i] + tt - cb[i]).abs().max()), float((R @ da - db).abs().max())]
        worst = max(worst, max(errs) / tol)
        assert max(errs) <= tol, (i, errs, tol)
    assert live >= 3
    print(f"[pose stages] A-k2: worst err / tol of the defined part = {worst:.3f} ({live} seeds with weights)")


# ---- B. the stop iteration in each of its three resolutions ---------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith(("B1-", "B2-", "B-it"))])
def test_b_stop_iteration(name):
    """B1: k_seed_kabsch finds the stop of its pair (clean: an early exit, the sums redone from that iterate; noisy: never).
    B2: k_stop_iteration over 63 flags (48 in 16-byte pieces, 15 in the scalar tail), the exit spanning the batch; B2-tail: 189
    flags, of which only the last seed's - all of them in the scalar tail - hold the batch's exit back.  B-it: num_iterations
    1, 2 and 64 (bit 63 of the mask), one pair and a uniform batch of two."""
    _, T, knn = _run_case(name)
    _check_bound_a(name, CASES[name], T, knn)


@pytest.mark.parametrize("k", [40, 41])
def test_b_batch_of_copies_stops_where_the_pair_stops(k):
    """The exit test over B copies of one pair passes exactly where it passes for the pair, so a uniform batch of three copies
    of a clean pair (k_stop_iteration: 3 x 7 x 10 = 210 flags, pieces that start at every phase of the iteration count, a
    tail of two) gives bitwise the seed_trans of the pair's own call (k_seed_kabsch's own search).  Where the exit IS taken,
    neighbouring iterates differ by less than bound A can see (the exit's own criterion); the bits still tell them apart."""
    name = f"B-copies-k{k}"
    case = CASES[name]
    three, T, knn = _run_case(name)
    _check_bound_a(name, case, T, knn)
    one = _head(case["scenes"][:1], case["seeds"][:1], k, case["iters"])
    stop = P.reference_transforms(dict(case, scenes=case["scenes"][:1], seeds=case["seeds"][:1]), one["knn"].long(), F64)[1][0]
    assert 2 <= stop < case["iters"] - 1
    for b in range(3):
        for key in ("knn", "T", "fit"):
            assert torch.equal(three[key][b], one[key][0]), f"pair {b}: `{key}` differs from the single pair's"


@pytest.mark.parametrize("k", [40, 41])
def test_b3_ragged_stop_per_pair(k):
    """The three kinds as one ragged batch (130, 171, 257 rows; 13, 17, 25 seeds): the exit is per pair - bound A against the
    reference run pair by pair -, every per-seed output of a pair is bitwise that of its own B = 1 call, and the slots behind
    a pair's seeds are zero."""
    name = f"B3-k{k}"
    case = CASES[name]
    out, T, knn = _run_case(name)
    _check_bound_a(name, case, T, knn)
    logits, r0 = P.ragged_logits(P.RAGGED_SIZES, k), 0
    for b, (sc, sd) in enumerate(zip(case["scenes"], case["seeds"])):
        n, S = P.RAGGED_SIZES[b], len(sd)
        one = _head([sc], None, k, case["iters"], logits=logits[None, r0:r0 + n], ratio=P.RAGGED_RATIO)
        assert one["seeds"].shape == (1, S)
        for key in ("seeds", "knn", "T", "fit"):
            assert torch.equal(out[key][b, :S], one[key][0]), f"{name}: pair {b}: `{key}` differs from the pair's own call"
            assert not bool(out[key][b, S:].any()), f"{name}: pair {b}: `{key}` behind the pair's seeds is not zero"
        assert torch.equal(out["final"][b], one["final"][0]) and torch.equal(out["labels"][r0:r0 + n], one["labels"][0])
        r0 += n


# ---- C. hypothesis scoring ------------------------------------------------------------------------------------------------------
def _check_scores(what, T, fit, src, tgt, tau=P.TAU):
    """T [S,4,4], fit [S] of the device, src / tgt [N,3]: fitness * N is the float64 inlier count of the device's own transform
    for every hypothesis without a band point, and between the counts at tau -+ band for the others (at most 10 %)."""
    N = src.shape[0]
    assert bool(torch.isfinite(T).all())
    r = P.residuals(T[None], src[None], tgt[None])[0]
    bd = P.band(src, tgt, T)
    in_band = ((r - tau).abs() <= bd).any(-1)
    assert int(in_band.sum()) <= 0.10 * len(in_band), f"{what}: {int(in_band.sum())} of {len(in_band)} hypotheses have a band point"
    got = torch.round(fit.to(F64) * N).long()
    assert torch.equal((got.to(F32) / N), fit), f"{what}: fitness is not count / N"
    cnt, lo, hi = (r < tau).sum(-1), (r < tau - bd).sum(-1), (r <= tau + bd).sum(-1)
    exact = ~in_band
    assert torch.equal(got[exact], cnt[exact]), f"{what}: counts {got[exact].tolist()} against {cnt[exact].tolist()}"
    assert bool(((got >= lo) & (got <= hi))[in_band].all()), what
    return r, bd, in_band


@pytest.mark.parametrize("S", P.SCORE_S)
def test_c_fitness_seed_counts(S):
    """S = 1, 7, 8, 9, 63, 64, 65 at N = 300: whole and partial groups of 8 hypotheses, odd S (the clamped last lane of a packed
    pair), more than one workgroup."""
    sc = P.plateau(300, 0)
    out = _head([sc], P.plateau_seeds(sc, S, 0)[None], 40, 10)
    assert out["fit"].shape == (1, S)
    _check_scores(f"S = {S}", out["T"][0], out["fit"][0], sc["src"], sc["tgt"])


@pytest.mark.parametrize("N", P.SCORE_N)
def test_c_fitness_point_counts(N):
    """N = 255, 256, 257: the 256-wide stride over the points."""
    sc = P.plateau(N, 0)
    out = _head([sc], P.plateau_seeds(sc, 30, 0)[None], 40, 10)
    _check_scores(f"N = {N}", out["T"][0], out["fit"][0], sc["src"], sc["tgt"])


def test_c_fitness_scattered_counts():
    """A third of the targets displaced by about the threshold: hypotheses with many different, non-trivial counts."""
    sc, seeds = P.scatter()
    out = _head([sc], seeds, 40, 10)
    r, _, in_band = _check_scores("scatter", out["T"][0], out["fit"][0], sc["src"], sc["tgt"])
    assert len(set((r < P.TAU).sum(-1)[~in_band].tolist())) >= 5


def test_c_fitness_ragged():
    """Plateau pairs of 130, 171, 257 rows with 13, 17, 25 seeds: odd per-pair seed counts below the stride S_max = 25 - the
    last packed pair of a pair's hypotheses is clamped to ITS S_p - 1, and each pair's points end at its own n."""
    scenes = [P.plateau(n, 10 + b) for b, n in enumerate(P.RAGGED_SIZES)]
    logits = P.ragged_logits(P.RAGGED_SIZES, 3)
    out = _head_ragged(scenes, logits, 40, 10, P.RAGGED_RATIO)
    for b, (sc, sd) in enumerate(zip(scenes, P.top_seeds(logits, P.RAGGED_SIZES, P.RAGGED_RATIO))):
        S = len(sd)
        assert torch.equal(out["seeds"][b, :S], sd)
        _check_scores(f"ragged pair {b}", out["T"][b, :S], out["fit"][b, :S], sc["src"], sc["tgt"])
        assert not bool(out["fit"][b, S:].any())


def test_c_threshold_is_strict():
    """Planted: k = 1 (every hypothesis is the identity), every source at the origin, tau = 0.25, targets on the axes at
    distance exactly 0.25 (squared distance 0.0625 = the smallest float whose root reaches tau: NOT below it) and one ulp
    less (below it).  Every operation of the fp32 residual is exact here, so the count is exact: the second half of the points."""
    N, S = 96, 9
    sc = P.clean(N, 0)
    d = torch.tensor([0.25] * (N // 2) + [float(np.nextafter(np.float32(0.25), np.float32(0)))] * (N // 2), dtype=F32)
    axis = torch.eye(3)[torch.arange(N) % 3] * torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)[:, None]
    sc = dict(sc, src=torch.zeros(N, 3), tgt=axis * d[:, None])
    out = _head([sc], P.seed_rows(N, S, 0), 1, 3, tau=0.25)
    assert torch.equal(out["T"][0], torch.eye(4).expand(S, 4, 4))
    assert torch.equal(out["fit"][0], torch.full((S,), (N // 2) / N)), out["fit"]
    assert torch.equal(out["labels"][0], (torch.arange(N) >= N // 2).float())
    assert torch.equal(out["final"][0], torch.eye(4))


# ---- D. argmax, labels, train-mode output ------------------------------------------------------------------------------------------
def _first_max(fit):
    return int((fit == fit.max()).nonzero()[0])


def _check_tie(what, T, fit, r, bd):
    """Condition 4 on the device's fitness: >= 8 seeds share the maximum, none of them has a band point, their transforms are
    not all the same bits, the first of them is not seed 0, and with more than 1024 seeds the thread that holds the first of
    them holds a second one (its stride loop must keep the first)."""
    top = (fit == fit.max()).nonzero()[:, 0]
    assert len(top) >= 8 and int(top[0]) > 0, f"{what}: {len(top)} seeds share the maximum, the first one at {int(top[0])}"
    assert len(fit) <= 1024 or int(top[0]) + 1024 in top.tolist(), f"{what}: the thread of the first maximum holds no second one"
    assert not bool(((r[top] - P.TAU).abs() <= bd).any())
    assert len({T[i].numpy().tobytes() for i in top.tolist()}) > 1


@pytest.mark.parametrize("N,S", P.ARGMAX_CASES)
def test_d_argmax_and_labels(N, S):
    """testing=False (no refinement): final_trans is bitwise seed_trans[s*], s* the FIRST index of the maximum of the device's
    fitness, among many tied seeds - 30 seeds in one wave; 70 across two waves of the 256-thread form; 1050 in the 1024-thread
    form, whose threads 0 .. 25 hold two seeds each -, and the labels are residual64 < tau outside the band."""
    sc = P.plateau(N, 0)
    out = _head([sc], P.plateau_seeds(sc, S, 0)[None], 40, 10, testing=False)
    T, fit = out["T"][0], out["fit"][0]
    r, bd, _ = _check_scores(f"argmax N = {N}", T, fit, sc["src"], sc["tgt"])
    _check_tie(f"argmax N = {N}", T, fit, r, bd)
    best = _first_max(fit)
    assert torch.equal(out["final"][0], T[best]), f"final_trans is not seed_trans[{best}]"
    clear = (r[best] - P.TAU).abs() > bd
    assert int(clear.sum()) >= 0.9 * N
    assert torch.equal(out["labels"][0][clear], (r[best] < P.TAU).float()[clear])
    assert bool(((out["labels"][0] == 0) | (out["labels"][0] == 1)).all())


# ---- E. refinement -----------------------------------------------------------------------------------------------------------------
def _post_refine(T0, src, tgt):
    out = _model(40, 10, 0.1).post_refinement(_dev(T0), _dev(src), _dev(tgt))
    torch.cuda.synchronize()
    gmf_amd.check_status()
    return out.cpu()


def _check_refined(what, got, T0, src, tgt):
    """got [B,4,4] of the device against `refine` in float64 from the float32 start T0, bound A's form with the floor of the
    float32 `refine`; every step of the float64 run keeps a band from the threshold (condition 5, here from the device's start)."""
    T64, cs, ms = P.refine(T0.to(F64), src.to(F64), tgt.to(F64), P.TAU)
    T32, cs32, _ = P.refine(T0, src, tgt, P.TAU)
    assert cs32 == cs, (cs32, cs)
    bd = P.band(src, tgt, T0)
    assert min(min(m) for m in ms) > bd, f"{what}: a residual within the band of the threshold: the counts are not defined in fp32"
    gmax = float(T64.abs().max())
    ratio = P.seed_floor(got, T64) / _bound(P.seed_floor(T32, T64), gmax)
    print(f"[pose stages] {what}: counts {cs}, worst err / tol = {float(ratio.max()):.3f}")
    assert bool(torch.isfinite(got).all()) and float(ratio.max()) <= 1.0, f"{what}: err / tol = {ratio.tolist()}, counts {cs}"
    return cs


@pytest.mark.parametrize("N", sorted(P.REFINE_SEEDS))
def test_e_post_refinement(N):
    """k_post_refine with 256 threads (N = 257) and 1024 (N = 2049)."""
    sc = P.refine_scene(N, P.REFINE_SEEDS[N])
    T0, s, t = sc["T0"][None], sc["src"][None], sc["tgt"][None]
    _check_refined(f"E refine N = {N}", _post_refine(T0, s, t), T0, s, t)


def test_e_post_refinement_batch():
    """B = 3, a different scene and a different number of steps per pair (the third one's count goes down once)."""
    scenes = [P.refine_scene(257, seed) for seed in P.REFINE_BATCH]
    T0, s, t = P.stack(scenes, "T0"), P.stack(scenes, "src"), P.stack(scenes, "tgt")
    cs = _check_refined("E refine B = 3", _post_refine(T0, s, t), T0, s, t)
    assert len({len(c) for c in cs}) > 1 and P.counts_shrink(cs[2])


def test_e_post_refinement_shrinking_count():
    """The inlier count goes DOWN at a step and the loop goes on: the exit is on an unchanged count."""
    sc = P.shrinking_scene(P.SHRINKING_SEED)
    T0, s, t = sc["T0"][None], sc["src"][None], sc["tgt"][None]
    cs = _check_refined("E refine shrinking", _post_refine(T0, s, t), T0, s, t)
    assert P.counts_shrink(cs[0])


def test_e_post_refinement_no_inlier():
    """A start without a single inlier: the first count equals the initial 0, the output is bitwise the input."""
    sc = P.refine_scene(257, 0)
    T0 = sc["T0"].clone()
    T0[:3, 3] += 10.0
    assert torch.equal(_post_refine(T0[None], sc["src"][None], sc["tgt"][None]), T0[None])


def test_e_post_refinement_planted_threshold():
    """All sources at the origin, the identity as input, targets on the positive axes.  At distance exactly float32(0.1) no point
    is an inlier (sqrt(fl(d d)) == d in IEEE fp32: the residual is d, not below the threshold) and the output is bitwise the
    input; one ulp closer every point is one: the rotation stays the identity (H = 0) and the translation is the weighted
    target mean (all weights equal, the denominator's 1e-6 included) to 1e-6."""
    N = 300
    axis = torch.eye(3)[torch.arange(N) % 3]
    eye = torch.eye(4)[None]
    at = torch.tensor(np.float32(0.1)) * axis
    assert torch.equal(_post_refine(eye, torch.zeros(1, N, 3), at[None]), eye)
    below = torch.tensor(np.nextafter(np.float32(0.1), np.float32(0))) * axis
    got = _post_refine(eye, torch.zeros(1, N, 3), below[None])[0]
    assert torch.equal(got[:3, :3], torch.eye(3)) and torch.equal(got[3], torch.tensor([0.0, 0.0, 0.0, 1.0]))
    w = 1.0 / (1.0 + (float(below.max()) / float(np.float32(0.1))) ** 2)
    want = below.to(F64).sum(0) * w / (N * w + 1e-6)
    assert float((got[:3, 3].to(F64) - want).abs().max()) <= 1e-6, (got[:3, 3], want)


def test_e_finalize_refines_the_best_seed():
    """testing=True (k_finalize_pose): on a plateau scene final_trans is bitwise post_refinement(seed_trans[s*]); on the
    scattered scene - where the refinement takes several steps - it meets the bound against `refine` in float64 from the
    device's seed_trans[s*].  The labels are those of the UN-refined hypothesis."""
    sc = P.plateau(700, 0)
    out = _head([sc], P.plateau_seeds(sc, 70, 0)[None], 40, 10, testing=True)
    r, bd, _ = _check_scores("finalize plateau", out["T"][0], out["fit"][0], sc["src"], sc["tgt"])
    _check_tie("finalize plateau", out["T"][0], out["fit"][0], r, bd)
    best = _first_max(out["fit"][0])
    start = out["T"][0][best][None]
    assert torch.equal(out["final"], _post_refine(start, sc["src"][None], sc["tgt"][None]))
    _check_refined("E finalize plateau", out["final"], start, sc["src"][None], sc["tgt"][None])
    sc, seeds = P.scatter()
    out = _head([sc], seeds, 40, 10, testing=True)
    r, bd, _ = _check_scores("finalize scatter", out["T"][0], out["fit"][0], sc["src"], sc["tgt"])
    best = _first_max(out["fit"][0])
    start = out["T"][0][best][None]
    cs = _check_refined("E finalize scatter", out["final"], start, sc["src"][None], sc["tgt"][None])
    assert len(cs[0]) >= 3
    clear = (r[best] - P.TAU).abs() > bd
    assert torch.equal(out["labels"][0][clear], (r[best] < P.TAU).float()[clear])


# ---- F. repeatability ------------------------------------------------------------------------------------------------------------------
def test_f_two_runs_same_bits():
    for name in ("A-k41", "B2-k40"):
        a, b = _run_case(name)[0], _run_case(name)[0]
        for key in ("final", "labels", "knn", "T", "fit", "seeds"):
            assert torch.equal(a[key], b[key]), (name, key)
    sc = P.plateau(700, 0)
    seeds = P.plateau_seeds(sc, 70, 0)[None]
    a, b = _head([sc], seeds, 40, 10), _head([sc], seeds, 40, 10)
    for key in ("final", "labels", "knn", "T", "fit", "seeds"):
        assert torch.equal(a[key], b[key]), ("argmax", key)
