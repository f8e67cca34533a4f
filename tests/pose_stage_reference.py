"""Stage-by-stage restatement of the forward pose head, and the scenes its tests run on.  TEST INFRASTRUCTURE ONLY.

Everything here evaluates the oracle's own functions (oracle/gmf_oracle.py: the seed_weights arithmetic, power_iteration's exit,
rigid_transform_3d, the residual of score_hypotheses, post_refinement) in the dtype of its inputs, so that a float64 call is
the reference of a stage and a float32 call measures that stage's noise floor.  Nothing derives from the code under test.

  compat_matrices         M of seed_weights (PointDSC.py:335-361), [B, S, k, k]
  power_iteration_trace   every iterate and the index the reference's exit stops at (PointDSC.py:437-448)
  seed_transforms         M -> trace -> w = v / (sum v + 1e-6) -> rigid_transform_3d, the exit spanning the batch or one pair
  residuals               |R p + t - q| in float64, [B, S, N]
  refine                  post_refinement for any B and any threshold, with the inlier-count sequence of every pair
  band                    bound on the fp32 evaluation error of a residual
  scenes                  clean / noisy / plateau / refine_scene / shrinking_scene / slow_tail_batch, all from seeded generators
"""
import torch
import torch.nn.functional as F

from oracle import gmf_oracle as O

C = 128                     # channels of the unit features (the seed kernels gather 128-wide rows)
SIGMA, SIGMA_D = 1.0, 0.10  # what every pose-stage test passes as `sigmas`
TAU = 0.10                  # inlier threshold of the scoring and of the refinement
F64, F32 = torch.float64, torch.float32


# ---- restatement helpers -------------------------------------------------------------------------------------------------------
def compat_matrices(feat_n, src, tgt, knn_idx, sigma, sigma_d):
    """The arithmetic of O.seed_weights up to M: feat_n [B,N,C], src, tgt [B,N,3], knn_idx [B,S,k] -> M [B,S,k,k] (zero diagonal),
    src_knn, tgt_knn [B,S,k,3]."""
    B, S, k = knn_idx.shape
    knn_idx = knn_idx.long()
    bi = torch.arange(B)[:, None, None]
    f = feat_n[bi, knn_idx]
    Mf = torch.clamp(1 - (1 - f @ f.transpose(2, 3)) / sigma ** 2, min=0)
    sk, tk = src[bi, knn_idx], tgt[bi, knn_idx]
    d = torch.cdist(sk, sk, compute_mode="donot_use_mm_for_euclid_dist") - \
        torch.cdist(tk, tk, compute_mode="donot_use_mm_for_euclid_dist")
    Ms = torch.clamp(1 - d * d / sigma_d ** 2, min=0)
    M = (Mf * Ms).clone()
    idx = torch.arange(k)
    M[:, :, idx, idx] = 0
    return M, sk, tk


def power_iteration_trace(M, iters):
    """O.power_iteration with every iterate kept: M [n,k,k] -> (V [stop + 1, n, k], stop).  The exit is the reference's
    (torch.allclose, rtol 1e-5, atol 1e-8, over ALL n rows given); stop = iters - 1 if it is never taken."""
    v = torch.ones_like(M[:, :, :1])
    last, trace, stop = v, [], iters - 1
    for it in range(iters):
        v = torch.bmm(M, v)
        v = v / (torch.norm(v, dim=1, keepdim=True) + 1e-6)
        trace.append(v[..., 0])
        if torch.allclose(v, last):
            stop = it
            break
        last = v
    return torch.stack(trace), stop


def trace_gaps(V):
    """gap_it = max(|v_it - v_(it-1)| - (1e-8 + 1e-5 |v_(it-1)|)) over everything in V [T,n,k] (v_(-1) = 1): positive while the
    exit is not taken, non-positive at the iterate it is taken at."""
    prev = torch.cat([torch.ones_like(V[:1]), V[:-1]])
    return ((V - prev).abs() - (1e-8 + 1e-5 * prev.abs())).flatten(1).max(dim=1)[0]


def seed_transforms(feat_n, src, tgt, knn_idx, sigma, sigma_d, iters, span, return_trace=False):
    """-> T [B,S,4,4], stop (list of B ints), gap (list of B tensors [stop_b + 1]).  span = "batch": one exit over all B S
    matrices (a uniform batch); "pair": every pair on its own (one pair, and each pair of a ragged batch).
    With return_trace also the list of the B traces [stop_b + 1, S, k]."""
    assert span in ("batch", "pair")
    B, S, k = knn_idx.shape
    M, sk, tk = compat_matrices(feat_n, src, tgt, knn_idx, sigma, sigma_d)
    if span == "batch":
        V, stop = power_iteration_trace(M.reshape(B * S, k, k), iters)
        g = trace_gaps(V)
        traces, stops, gaps = [V[:, b * S:(b + 1) * S] for b in range(B)], [stop] * B, [g] * B
    else:
        traces, stops, gaps = [], [], []
        for b in range(B):
            V, stop = power_iteration_trace(M[b], iters)
            traces.append(V), stops.append(stop), gaps.append(trace_gaps(V))
    v = torch.stack([t[-1] for t in traces])                              # [B,S,k]
    w = v / (v.sum(-1, keepdim=True) + 1e-6)
    T = O.rigid_transform_3d(sk.reshape(B * S, k, 3), tk.reshape(B * S, k, 3), w.reshape(B * S, k)).reshape(B, S, 4, 4)
    if return_trace:
        return T, stops, gaps, traces
    return T, stops, gaps


def kabsch_moments(feat_n, src, tgt, knn_idx, iters, span, sigma=SIGMA, sigma_d=SIGMA_D):
    """What rigid_transform_3d solves from (common.py:25-37), for the cases whose rotation is not unique: the weighted
    centroids ca, cb [B,S,3], H = sum w (a - ca)(b - cb)^T [B,S,3,3] and the weights w [B,S,k] of the iterate the trace stops at."""
    _, _, _, traces = seed_transforms(feat_n, src, tgt, knn_idx, sigma, sigma_d, iters, span, True)
    _, sk, tk = compat_matrices(feat_n, src, tgt, knn_idx, sigma, sigma_d)
    v = torch.stack([t[-1] for t in traces])
    w = v / (v.sum(-1, keepdim=True) + 1e-6)
    sw = w.sum(-1, keepdim=True)[..., None] + 1e-6
    ca = (sk * w[..., None]).sum(2, keepdim=True) / sw
    cb = (tk * w[..., None]).sum(2, keepdim=True) / sw
    H = (sk - ca).transpose(2, 3) @ (w[..., None] * (tk - cb))
    return ca[:, :, 0], cb[:, :, 0], H, w


def residuals(T, src, tgt):
    """float64 |R p + t - q|: T [B,S,4,4], src, tgt [B,N,3] -> [B,S,N]."""
    T, src, tgt = T.to(F64), src.to(F64), tgt.to(F64)
    pred = torch.einsum("bsnm,bkm->bskn", T[:, :, :3, :3], src) + T[:, :, None, :3, 3]
    return torch.norm(pred - tgt[:, None], dim=-1)


def refine(T, src, tgt, thr, iters=20, exit_when_not_growing=False):
    """O.post_refinement with the threshold given, pair by pair, in the dtype of the inputs: T [B,4,4] -> (T_out [B,4,4],
    counts, margins): per pair the inlier count of every step evaluated (the last one is the step that took the exit, unless
    `iters` ran out) and the distance min | |r| - thr | of that step's residuals from the threshold.
    exit_when_not_growing: NOT the reference - the loop that also stops at a smaller count; the host tests use it to show that a
    scene tells the two exits apart."""
    out, counts, margins = [], [], []
    for b in range(T.shape[0]):
        Tb, s, t = T[b:b + 1], src[b:b + 1], tgt[b:b + 1]
        prev, cs, ms = 0, [], []
        for _ in range(iters):
            warped = s @ Tb[:, :3, :3].transpose(1, 2) + Tb[:, None, :3, 3]
            d = torch.norm(warped - t, dim=-1)
            inl = (d < thr)[0]
            n = int(inl.sum())
            cs.append(n), ms.append(float((d - thr).abs().min()))
            if abs(n - prev) < 1 or (exit_when_not_growing and n <= prev):
                break
            prev = n
            Tb = O.rigid_transform_3d(s[:, inl], t[:, inl], (1 / (1 + (d / thr) ** 2))[:, inl])
        out.append(Tb[0]), counts.append(cs), margins.append(ms)
    return torch.stack(out), counts, margins


def band(src, tgt, T):
    """16 * 2^-24 * (3 max|src| + max|tgt| + max|t|): the fp32 evaluation of one residual component takes at most 7 roundings
    at magnitudes no larger than that sum; a residual closer than this to a threshold may fall on either side in fp32."""
    return 16 * 2.0 ** -24 * (3 * float(src.abs().max()) + float(tgt.abs().max()) + float(T[..., :3, 3].abs().max()))


def seed_floor(T32, T64):
    """Per-seed noise floor max|T32 - T64| over rows 0-2: [..., 4, 4] -> [...]."""
    return (T32.to(F64) - T64)[..., :3, :].abs().flatten(-2).max(dim=-1)[0]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(int(sum(int(v) * 1000003 ** i for i, v in enumerate(key)) % (2 ** 62)))
    return g


def _motion(g):
    Q, Rr = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))
    Q = Q * torch.sign(torch.diagonal(Rr))
    if torch.det(Q) < 0:
        Q[:, 2] = -Q[:, 2]
    return Q, torch.randn(3, generator=g, dtype=F64)


def _pose(R, t):
    T = torch.eye(4, dtype=F64)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _scene(feat, src, tgt, T):
    """float32 tensors (what the device gets; the float64 reference reads the same values, upcast)."""
    return {"feat_n": F.normalize(feat, dim=-1).to(F32), "src": src.to(F32), "tgt": tgt.to(F32), "gt": T}


def clean(N, seed, jitter=0.0):
    """A rigid motion of N points with unit features normalize(u + 0.02 noise) around one direction u: M is dense and the
    power iteration takes its exit after a few iterates.  jitter = 0: exact motion (every weighting gives the same transform);
    jitter > 0 displaces every target by jitter * sigma_d * noise, so that the weights matter and the exit stays early."""
    g = _gen(1, N, seed)
    R, t = _motion(g)
    src = torch.randn(N, 3, generator=g, dtype=F64)
    tgt = src @ R.t() + t + jitter * SIGMA_D * torch.randn(N, 3, generator=g, dtype=F64)
    u = F.normalize(torch.randn(C, generator=g, dtype=F64), dim=0)
    return _scene(u + 0.02 * torch.randn(N, C, generator=g, dtype=F64), src, tgt, _pose(R, t))


def noisy(N, seed, disp=4.0, feat_noise=0.6):
    """A third of the targets displaced by disp * sigma_d * noise, features u + feat_noise * noise (almost unrelated rows):
    M is sparse and uneven, the iterates move for many steps - with few iterations allowed the exit is never taken and the
    transform depends on the iterate it is solved from.  disp = 4 (0.4 units) is the level at which a solve from the iterate
    before the right one moves most seeds by more than 4 x the comparison's bound (at 0.5 it moves them by 3 x at the most:
    tests/test_pose_stages_host.py::test_noisy_scenes_tell_the_iterates_apart); disp = 1 puts the displaced third near the
    inlier threshold (`scatter`)."""
    g = _gen(2, N, seed)
    R, t = _motion(g)
    src = torch.randn(N, 3, generator=g, dtype=F64)
    tgt = src @ R.t() + t
    moved = torch.randperm(N, generator=g)[:N // 3]
    tgt[moved] += disp * SIGMA_D * torch.randn(len(moved), 3, generator=g, dtype=F64)
    u = F.normalize(torch.randn(C, generator=g, dtype=F64), dim=0)
    return _scene(u + feat_noise * torch.randn(N, C, generator=g, dtype=F64), src, tgt, _pose(R, t))


def plateau(N, seed):
    """60 % exact inliers with tightly clustered features, 40 % outliers displaced by 2-3 units with unrelated features.  Every
    inlier seed's neighbours are inliers, so its hypothesis is the motion up to rounding: many seeds reach the same maximal
    inlier count with different transform bits.  `inlier` [N] marks the inliers."""
    g = _gen(3, N, seed)
    R, t = _motion(g)
    src = torch.randn(N, 3, generator=g, dtype=F64)
    tgt = src @ R.t() + t
    out = torch.randperm(N, generator=g)[:N - (6 * N) // 10]
    step = F.normalize(torch.randn(len(out), 3, generator=g, dtype=F64), dim=-1)
    tgt[out] += step * (2 + torch.rand(len(out), 1, generator=g, dtype=F64))
    u = F.normalize(torch.randn(C, generator=g, dtype=F64), dim=0)
    feat = u + 0.02 * torch.randn(N, C, generator=g, dtype=F64)
    feat[out] = torch.randn(len(out), C, generator=g, dtype=F64)
    sc = _scene(feat, src, tgt, _pose(R, t))
    sc["inlier"] = torch.ones(N, dtype=torch.bool)
    sc["inlier"][out] = False
    return sc


def plateau_seeds(sc, S, seed):
    """S seed rows of a plateau scene, inliers and outliers mixed at random, with seed 0 an outlier and seed 1 an inlier (the
    first maximum of the fitness is at index 1) and, for S > 1025, seed 1025 an inlier too: the 1024-thread argmax holds
    seeds 1 and 1025 in one thread, and both reach the maximum."""
    g = _gen(4, S, seed)
    N = sc["inlier"].numel()
    order = torch.randperm(N, generator=g)[:S]
    fixed = [(0, False), (1, True), (1025, True)]

    def put(pos, inlier):
        if pos < S and bool(sc["inlier"][order[pos]]) != inlier:
            free = [j for j in range(S) if j not in (0, 1, 1025) and bool(sc["inlier"][order[j]]) == inlier]
            if free:
                j, here = free[0], int(order[pos])
                order[pos], order[j] = int(order[j]), here

    for pos, inlier in fixed:
        put(pos, inlier)
    return order.to(torch.int32)


def refine_scene(N, seed, inlier_noise=0.03, outliers=0.3, rot=0.04, shift=0.04):
    """A scene and an initial transform for post_refinement: inliers with inlier_noise of target noise, a fraction of outliers
    displaced by up to one unit, the ground-truth pose perturbed by `rot` radians and `shift` units: the inlier count changes
    over several steps before it repeats.  -> scene with "T0" [4,4] float32."""
    g = _gen(5, N, seed)
    R, t = _motion(g)
    src = torch.randn(N, 3, generator=g, dtype=F64)
    tgt = src @ R.t() + t + inlier_noise * torch.randn(N, 3, generator=g, dtype=F64)
    out = torch.randperm(N, generator=g)[:int(N * outliers)]
    tgt[out] += F.normalize(torch.randn(len(out), 3, generator=g, dtype=F64), dim=-1) * torch.rand(len(out), 1, generator=g, dtype=F64)
    ax = F.normalize(torch.randn(3, generator=g, dtype=F64), dim=0) * rot
    K = torch.tensor([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], dtype=F64)
    T0 = _pose(torch.linalg.matrix_exp(K) @ R, t + shift * F.normalize(torch.randn(3, generator=g, dtype=F64), dim=0))
    sc = _scene(torch.randn(N, C, generator=g, dtype=F64), src, tgt, _pose(R, t))
    sc["T0"] = T0.to(F32)
    return sc


def counts_shrink(cs):
    """The inlier-count sequence decreases at some step and the loop continues behind it."""
    return any(cs[i] < cs[i - 1] for i in range(1, len(cs) - 1))


SHRINKING_N = 300


def shrinking_scene(seed):
    """refine_scene at N = 300 with heavy inlier noise and a large perturbation: for some seeds the float64 inlier count goes
    DOWN at a step and the loop goes on (the exit is on an unchanged count, not on a count that stopped growing)."""
    return refine_scene(SHRINKING_N, seed, inlier_noise=0.05, outliers=0.4, rot=0.10, shift=0.08)


def find_shrinking_seed(limit=1000):
    """The deterministic search the committed SHRINKING_SEED comes from: the first seed in 0 .. limit - 1 whose float64 count
    sequence shrinks somewhere, whose steps all keep 4 bands of distance from the threshold and whose float32 sequence is the
    same.  None if there is none."""
    for seed in range(limit):
        sc = shrinking_scene(seed)
        T0, s, t = sc["T0"][None], sc["src"][None], sc["tgt"][None]
        _, cs, ms = refine(T0.to(F64), s.to(F64), t.to(F64), TAU)
        if counts_shrink(cs[0]) and min(ms[0]) > 4 * band(s, t, T0) and refine(T0, s, t, TAU)[1] == cs:
            return seed
    return None


def slow_tail_batch(N, S, seed):
    """Three clean (jittered) pairs and S seed rows each, for the flags k_stop_iteration reads behind its last whole 16-byte
    piece: the LAST seed of the LAST pair - and no other - sits in a group of 2 x 24 points that follow two different motions
    and share one feature cluster of their own.  Its M has two blocks of nearly equal weight: its iterates keep moving (and
    its transform with them) long after every other seed passed the exit test, so the batch's exit is never taken.
    -> (list of 3 scenes, seeds [3, S] int32)."""
    g = _gen(6, N, seed)
    scenes = [clean(N, 100 * seed + b, jitter=0.2) for b in range(3)]
    sc = scenes[2]
    grp = torch.randperm(N, generator=g)[:48]
    R2, t2 = _motion(g)
    src, tgt = sc["src"].to(F64), sc["tgt"].to(F64)
    tgt[grp[24:]] = src[grp[24:]] @ R2.t() + t2
    v = F.normalize(torch.randn(C, generator=g, dtype=F64), dim=0)
    feat = sc["feat_n"].to(F64)
    feat[grp] = v + 0.02 * torch.randn(48, C, generator=g, dtype=F64)
    scenes[2] = dict(_scene(feat, src, tgt, sc["gt"]))
    seeds = torch.empty(3, S, dtype=torch.int32)
    for b in range(3):
        free = torch.ones(N, dtype=torch.bool)
        if b == 2:
            free[grp] = False
        rows = free.nonzero()[:, 0]
        seeds[b] = rows[torch.randperm(len(rows), generator=g)[:S]].to(torch.int32)
    seeds[2, S - 1] = int(grp[0])
    return scenes, seeds


def stack(scenes, key):
    return torch.stack([sc[key] for sc in scenes])


def exact_knn(feat_n, seeds, k):
    """The reference's own neighbours of the seed rows (O.knn_indices in float64): feat_n [B,N,C], seeds [B,S] -> [B,S,k]."""
    knn = O.knn_indices(feat_n.to(F64), k)
    return torch.gather(knn, 1, seeds.long()[:, :, None].expand(-1, -1, k))


# ---- the cases, shared by the host conditions and the GPU comparisons ------------------------------------------------------------
def seed_rows(N, S, seed):
    """S distinct rows of a pair, [1, S] int32."""
    return torch.randperm(N, generator=_gen(7, N, seed))[:S][None].to(torch.int32)


def ratio_for(S, N):
    """A ratio with int(N * ratio) == S, away from the rounding of the product."""
    return (S + 0.5) / N


K_LIST = (1, 2, 31, 32, 33, 40, 41, 48, 63, 64)
RAGGED_SIZES, RAGGED_RATIO = (130, 171, 257), 0.1


def ragged_logits(sizes, seed):
    """Distinct scores for the packed rows of a ragged batch: the seeds of pair b are the top int(n_b * ratio) of its slice."""
    total = sum(sizes)
    return torch.randperm(total, generator=_gen(8, total, seed)).to(F32) / total


def top_seeds(logits, sizes, ratio):
    """The rows the top-S selection returns for distinct scores (exact on the host), one [S_b] int32 tensor per pair."""
    out, r0 = [], 0
    for n in sizes:
        out.append(torch.argsort(logits[r0:r0 + n], descending=True)[:int(n * ratio)].to(torch.int32))
        r0 += n
    return out


def trans_cases():
    """{name: dict} of every `seed_trans` comparison: scenes (one per pair), seeds ([B,S] int32; ragged: a list of [S_b]),
    k (as requested; the model caps it at N - 1), iters, span, form ("single" / "uniform" / "ragged"), kind per pair."""
    cases = {}

    def add(name, scenes, seeds, k, iters, span, form, kinds):
        cases[name] = {"scenes": scenes, "seeds": seeds, "k": k, "iters": iters, "span": span, "form": form, "kinds": kinds}

    for k in K_LIST:                                                       # A: every branch of the tiles and of the row length
        N = max(k + 1, 130)
        add(f"A-k{k}", [noisy(N, k)], seed_rows(N, 13, k), k, 3, "pair", "single", ["noisy"])
    for k in (40, 64):                                                     # ... and N = k + 1: every point is a neighbour
        add(f"A-k{k}-all", [noisy(k + 1, 100 + k)], seed_rows(k + 1, 13, k), k, 3, "pair", "single", ["noisy"])
    for k in (40, 41):
        # B.1: one pair resolves the stop itself; clean takes the exit early (the sums are redone from an earlier iterate)
        add(f"B1-clean-k{k}", [clean(130, 7, jitter=0.2)], seed_rows(130, 13, k), k, 10, "pair", "single", ["clean"])
        add(f"B1-noisy-k{k}", [noisy(130, k)], seed_rows(130, 13, k), k, 10, "pair", "single", ["noisy"])
        # B.2: B S iters = 63 flags, the exit spans the batch
        scenes = [clean(130, 10 + k, jitter=0.2), noisy(130, 20 + k), clean(130, 30 + k, jitter=0.2)]
        add(f"B2-k{k}", scenes, torch.cat([seed_rows(130, 7, 40 + b) for b in range(3)]), k, 3, "batch", "uniform",
            ["clean", "noisy", "clean"])
        # ... and 189 flags of which only the last seed's (behind the last whole 16-byte piece) keep the batch from its exit
        scenes, seeds = slow_tail_batch(130, 7, k)
        add(f"B2-tail-k{k}", scenes, seeds, k, 9, "batch", "uniform", ["clean", "clean", "clean+slow"])
        # B.3: the three kinds as a ragged batch, the exit per pair
        scenes = [clean(RAGGED_SIZES[0], 19, jitter=0.2), noisy(RAGGED_SIZES[1], 60 + k), clean(RAGGED_SIZES[2], 10, jitter=0.2)]
        add(f"B3-k{k}", scenes, top_seeds(ragged_logits(RAGGED_SIZES, k), RAGGED_SIZES, RAGGED_RATIO), k, 10, "pair", "ragged",
            ["clean", "noisy", "clean"])
        # three copies of one clean pair: 210 flags; the batch's exit is the pair's own
        add(f"B-copies-k{k}", [clean(130, 7, jitter=0.2)] * 3, seed_rows(130, 7, k).expand(3, 7).contiguous(), k, 10, "batch", "uniform",
            ["clean"] * 3)
        for iters in (1, 2, 64):
            add(f"B-it{iters}-k{k}", [clean(130, 8, jitter=0.2)], seed_rows(130, 13, k), k, iters, "pair", "single", ["clean"])
            add(f"B-it{iters}-k{k}-B2", [clean(130, 8, jitter=0.2), clean(130, 10, jitter=0.2)],
                torch.cat([seed_rows(130, 13, k), seed_rows(130, 13, k + 1)]), k, iters, "batch", "uniform", ["clean", "clean"])
    return cases


def case_pairs(case):
    """The pairs of a case as B = 1 problems: [(feat_n, src, tgt [1,N,*], seeds [1,S])]."""
    return [(sc["feat_n"][None], sc["src"][None], sc["tgt"][None], case["seeds"][b][None])
            for b, sc in enumerate(case["scenes"])]


def reference_transforms(case, knn, dtype):
    """seed_transforms of a case on given neighbours (knn: [B,S,k], or a list of [S_b,k] for a ragged case) in `dtype`:
    -> per pair a list of T [S_b,4,4], stops, gaps, traces."""
    if case["form"] == "ragged":
        out = [], [], [], []
        for (f, s, t, _), nb in zip(case_pairs(case), knn):
            r = seed_transforms(f.to(dtype), s.to(dtype), t.to(dtype), nb[None], SIGMA, SIGMA_D, case["iters"], "pair", True)
            out[0].append(r[0][0]), out[1].append(r[1][0]), out[2].append(r[2][0]), out[3].append(r[3][0])
        return out
    f, s, t = (stack(case["scenes"], key).to(dtype) for key in ("feat_n", "src", "tgt"))
    T, stops, gaps, traces = seed_transforms(f, s, t, knn, SIGMA, SIGMA_D, case["iters"], case["span"], True)
    return list(T), stops, gaps, traces


def reference_knn(case):
    """The reference's own exact neighbours of a case's seeds (list per pair for a ragged case)."""
    if case["form"] == "ragged":
        return [exact_knn(f, sd, min(case["k"], f.shape[1] - 1))[0] for f, _, _, sd in case_pairs(case)]
    f = stack(case["scenes"], "feat_n")
    return exact_knn(f, case["seeds"], min(case["k"], f.shape[1] - 1))


ILL_REL, ILL_CAP = 1e-4, 0.05


def ill_conditioned(T32, T64):
    """Condition 2: per pair lists of T [S,4,4] -> (list of bool [S] masks of the seeds whose float32 reference misses the
    float64 one by more than 1e-4 gmax, the floors, gmax of the case)."""
    gmax = max(float(T.abs().max()) for T in T64)
    floors = [seed_floor(a, b) for a, b in zip(T32, T64)]
    return [fl > ILL_REL * gmax for fl in floors], floors, gmax


# scoring / argmax / refinement scenes
SCORE_S = (1, 7, 8, 9, 63, 64, 65)
SCORE_N = (255, 256, 257)
ARGMAX_CASES = ((300, 30), (700, 70), (2100, 1050))
REFINE_SEEDS = {257: 3, 2049: 2}                 # refine_scene seeds whose every step keeps >= 4 bands from the threshold
REFINE_BATCH = (0, 1, 2)                         # B = 3 at N = 257: three different scenes (seed 2's count shrinks once)
SHRINKING_SEED = 7                               # find_shrinking_seed()
SCATTER_SEED = 20


def scatter():
    """The scene whose hypotheses take several non-trivial inlier counts: noisy with a third of the targets displaced by about
    the threshold, 65 seeds.  Its best hypothesis leads by two inliers and the refinement from it takes four steps.
    -> (scene, seeds [1, 65])"""
    return noisy(300, SCATTER_SEED, disp=1.0), seed_rows(300, 65, SCATTER_SEED)
