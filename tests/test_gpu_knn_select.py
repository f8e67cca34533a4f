"""The kNN row selection, held to its exact order in every kernel form.

The result is fully defined: the k + 1 smallest entries of a distance row under (distance ascending, index ascending), rank 0
dropped, k indices written - a stable argsort of the row.  Every comparison here is exact equality against numpy on the host;
the only exceptions are rows with fewer than k + 1 finite entries, for which the kernels promise the exact prefix over the finite
entries and an in-range index in every other slot (pose_kernels.hip, the comment at the head of k_knn_select_fast).

  1. gmf_knn_from_distances on rows built from small integers and dyadic fractions - ties at every rank, the kCandMax = 1024
     boundary from both sides, winners owned by one thread / one group of four, signed zeros, subnormals, +inf and NaN tails -
     at every N on both sides of each instantiation's limit (k_knn_select_fast<8 / 20 / 32 / 64>, k_knn_select_stream).  The
     row padding (columns N .. ld - 1) holds -3e38: a read of it would win the selection.
  2. The feature-fed forms (gmf_knn_rows through k_seed_dist + selection, and through the in-LDS k_knn_seeds for k > 63; the pose
     head at k = 64 - the only entry that reaches the 256-minima threshold branch; the ragged pose head) on unit rows whose dot
     products are exact in every arithmetic the library uses, with heavy ties and bitwise duplicate rows.
  3. The public gmf_amd.knn on rows with bitwise duplicates, both `ignore_self` values, both distance paths."""
import ctypes

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import _lib, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_CAND_MAX = 1024           # kCandMax of pose_kernels.hip
PAD = -3e38                 # what the row padding holds: below every test value, so a read of it shows up as a neighbour
INF, NAN = float("inf"), float("nan")


def _h():
    return _lib.handle_for(0), torch.cuda.current_stream().cuda_stream


def _ld(N):
    return 32 * ((N + 31) // 32)


def _stable_knn(rows, k):
    """rows [R, N] (any float type) -> [R, k]: ranks 1 .. k of every row under (value, index); NaN last."""
    return np.stack([np.argsort(r, kind="stable")[1:k + 1] for r in rows])


# ---- 1. gmf_knn_from_distances against a stable argsort ----------------------------------------------------------------------
def _candidates(row, k):
    """The threshold step of k_knn_select_fast / k_knn_select_stream for k + 1 <= 64, restated: thread t owns the indices
    j = t (mod 256), a group is four neighbouring threads, T is the (k + 1)-th smallest of the 64 group minima (NaN is below no
    minimum; a group without an entry has +inf), and the candidates are the entries <= T.  Returns their number c: c <= kCandMax
    takes the candidate-ranking path, c > kCandMax the round-based fallback."""
    N = row.shape[0]
    full = np.full(256 * ((N + 255) // 256), NAN, np.float32)
    full[:N] = row
    by_group = np.where(np.isnan(full), INF, full).reshape(-1, 64, 4)          # [m, group, thread in group]
    T = np.sort(by_group.min(axis=(0, 2)), kind="stable")[k]
    with np.errstate(invalid="ignore"):
        return int((row <= T).sum())


def _spread(n, N, taken=()):
    """n distinct indices spread evenly over [0, N), none of them in `taken`."""
    free = np.setdiff1d(np.arange(N), np.asarray(taken, np.int64))
    return free[(np.arange(n) * len(free)) // n]


def _owner_slots(N, residues):
    """All indices j < N with j mod 256 in `residues`, ascending."""
    j = np.arange(N)
    return j[np.isin(j % 256, residues)]


def _row_kinds(N, k, rng):
    """[(name, row float32 [N], finite)]: `finite` None = the whole result is exact; a number f < k + 1 = only f entries are
    finite, the prefix over them is exact and every other slot only has to be in range."""
    f32 = np.float32
    kinds = []

    def add(name, row, finite=None):
        row = np.asarray(row, f32)
        assert row.shape == (N,)
        kinds.append((name, row, finite))

    # 1. distinct values; 2. all equal (above N = 1024 every element is a candidate: the fallback; expected 1 .. k);
    # 3. ties at every rank; 4. ramps - the descending one has its winners at the highest indices, in the last, partly filled slot
    add("distinct", rng.permutation(N))
    add("equal", np.full(N, 3.0))
    add("mod7", np.arange(N) % 7)
    add("ramp_up", np.arange(N))
    add("ramp_down", N - 1 - np.arange(N))
    # 5. the kCandMax boundary: exactly 1024 / 1025 zeros at random places (they reach every group), the rest ones -> T = 0 and
    # the candidates are the zeros: c = 1024 is the last count the ranking path takes, c = 1025 the first one of the fallback
    if N >= 2049:
        for z in (K_CAND_MAX, K_CAND_MAX + 1):
            row = np.ones(N, f32)
            row[rng.permutation(N)[:z]] = 0.0
            assert _candidates(row, k) == z
            add(f"zeros{z}", row)
        # c = 1025 again, with winners where a kernel that ranked 1025 candidates in its 1024 LDS slots would lose one: the register
        # kernel places a wave's candidates by (lane, slot m), so the one beyond the array is the last slot of lane 63 of the wave
        # that arrives last; the stream kernel places them as its loop reaches them, the last slots last.  Four zeros sit exactly
        # there (thread 64 w + 63, its last slot), 1021 halves lie at random places among the rest: for k >= 4, T = 0.5 and c = 1025
        last = np.array([t + 256 * ((N - 1 - t) // 256) for t in (63, 127, 191, 255)])
        row = np.ones(N, f32)
        row[rng.permutation(np.setdiff1d(np.arange(N), last))[:K_CAND_MAX - 3]] = 0.5
        row[last] = 0.0
        if k >= 4:
            assert _candidates(row, k) == K_CAND_MAX + 1
        add("zeros_placed_last", row)
    # 6. ties below the fallback: a few smaller values, then a run of up to 500 equal values that contains rank k, then distinct
    # larger ones -> the candidate-ranking path, decided by the index
    n_small = k // 2
    n_tie = min(500, N - n_small)
    pos = rng.permutation(N)
    row = 1.0 + rng.permutation(N).astype(f32)
    row[pos[:n_small]] = -1.0 - np.arange(n_small)
    row[pos[n_small:n_small + n_tie]] = 0.0
    add("tie_run", row)
    # 7. every winner in one owner.  Thread 5 owns the indices = 5 (mod 256); the group of threads 4 .. 7 the indices = 4 .. 7.
    # Only one of the 64 group minima is small then, so T is the k-th smallest of the OTHER groups' minima - loose:
    #   rest constant: T = that constant and every element is a candidate - c = N: the ranking path up to N = 1024 (here only the
    #     group rows of N = 255 .. 257 at k = 1: no smaller size holds k + 1 such slots), the fallback above - every size from
    #     2048 on -, whose every round is won by the same owner, which rescans its registers k + 1 times;
    #   rest distinct: T = about the k-th smallest of the rest, c = a few k: the ranking path at every size.
    for name, residues, rest in (("one_thread_const", [5], "const"), ("one_group_const", [4, 5, 6, 7], "const"),
                                 ("one_group_distinct", [4, 5, 6, 7], "distinct")):
        slots = _owner_slots(N, residues)
        if len(slots) < k + 1:
            continue
        win = rng.permutation(slots)[:k + 1]
        row = np.full(N, 7.0, f32) if rest == "const" else 1.0 + rng.permutation(N).astype(f32)
        row[win] = -1.0 - rng.permutation(k + 1)
        c = _candidates(row, k)
        assert (c == N) if rest == "const" else (c <= K_CAND_MAX)
        add(name, row)
    # 8. special finite values: -0.0 and +0.0 compare equal, so the index decides among them; negative values and subnormals
    row = np.ones(N, f32)
    z = np.arange(0, N, 3)
    row[z] = np.where(rng.integers(0, 2, len(z)) == 1, f32(-0.0), f32(0.0))
    add("signed_zeros", row)
    row = (rng.permutation(N) - N // 2).astype(f32) * f32(2.0 ** -149)                    # distinct, both signs, all subnormal
    assert len(np.unique(row)) == N and np.abs(row).max() < np.finfo(f32).tiny
    add("subnormal", row)
    # 9. non-finite tails that leave at least k + 1 finite entries: exact (stable argsort puts +inf behind the finite entries in
    # index order and NaN last)
    nf = max(k + 1, N - max(1, N // 3))
    for name, fill in (("inf_tail", INF), ("nan_tail", NAN)):
        row = rng.permutation(N).astype(f32)
        row[nf:] = fill
        add(name, row)
    # ... and fewer than k + 1 finite entries, or none
    few = max(1, (k + 1) // 2)
    for name, fill in (("few_finite_nan", NAN), ("few_finite_inf", INF)):
        row = np.full(N, fill, f32)
        row[_spread(few, N)] = rng.permutation(few)
        add(name, row, finite=few)
    add("all_nan", np.full(N, NAN), finite=0)
    return kinds


@pytest.mark.parametrize("k", [1, 10, 40, 63])
@pytest.mark.parametrize("N", ["k+1", 255, 256, 257, 2048, 2049, 4999, 5120, 5121, 8192, 8193, 16384, 16385, 20001])
def test_selection_is_stable_argsort(N, k):
    """Every row kind of one (N, k) as the S rows of one call, B = 2 with the second pair's rows reversed (the (pair S + s) ld
    stride).  Kernel by size: k_knn_select_fast<8> N <= 2048, <20> <= 5120, <32> <= 8192, <64> <= 16384, k_knn_select_stream
    above; the candidate path of a row is `_candidates` (asserted where a row is built for one side of kCandMax)."""
    N = k + 1 if N == "k+1" else N
    assert k <= N - 1
    rng = np.random.default_rng([7, N, k])
    kinds = _row_kinds(N, k, rng)
    S, ld = len(kinds), _ld(N)
    rows = np.stack([r for _, r, _ in kinds])
    dist = np.full((2, S, ld), PAD, np.float32)
    dist[0, :, :N] = rows
    dist[1, :, :N] = rows[::-1]
    out = torch.full((2, S, k), -1, dtype=torch.int32, device=DEV)
    h, st = _h()
    dist_d = torch.from_numpy(dist).to(DEV)
    h.call("gmf_knn_from_distances", dist_d.data_ptr(), 2, N, S, k, out.data_ptr(), st)
    got = out.cpu().numpy()
    gmf_amd.check_status()
    want = _stable_knn(rows, k)
    for pair in (0, 1):
        for s, (name, _, finite) in enumerate(kinds):
            g = got[pair, s if pair == 0 else S - 1 - s]
            what = f"row kind {name}, N = {N}, k = {k}, pair {pair}"
            if finite is None:
                assert np.array_equal(g, want[s]), f"{what}: got {g}, want {want[s]}"
            else:
                n = max(0, finite - 1)
                assert np.array_equal(g[:n], want[s][:n]), f"{what}: prefix over the finite entries: got {g[:n]}, want {want[s][:n]}"
                assert (g >= 0).all() and (g < N).all(), f"{what}: index out of range: {g}"


# ---- 2. the feature-fed forms, exact -------------------------------------------------------------------------------------------
def _exact_unit_rows(N, rng, C=128, n_dup=12):
    """[N, C] float32 unit rows whose dot products are exact everywhere: four non-zero channels of +-0.5 each (norm 1; every
    partial sum of a dot product is a multiple of 0.25 of magnitude <= 1: the same in split-fp16 MFMA, fp32 MFMA and fmaf
    order).  Supports come from a pool of 24 over the first 16 channels, so the distances 2 - 2 <a, b> take nine values and
    rows tie heavily; n_dup rows are bitwise copies of another row (each pair is a duplicate at j < i for one row and at j > i
    for the other)."""
    pool = np.stack([rng.permutation(16)[:4] for _ in range(24)])
    sup = pool[rng.integers(0, len(pool), N)]
    F = np.zeros((N, C), np.float32)
    F[np.arange(N)[:, None], sup] = rng.choice(np.float32([-0.5, 0.5]), (N, 4))
    dup = rng.permutation(N)[:2 * n_dup]
    F[dup[:n_dup]] = F[dup[n_dup:]]
    return F, np.sort(dup)


def _feature_knn(F, rows, k):
    """Ranks 1 .. k under (2 - 2 F F^T in float64 - exact -, index) for the listed rows."""
    F64 = F.astype(np.float64)
    return _stable_knn(2.0 - 2.0 * (F64[rows] @ F64.T), k)


def _features_and_rows(N, n_rows, seed):
    """Two pairs of features, and per pair the listed rows: every duplicated row, filled up with spread ones (all rows if n_rows
    >= N)."""
    rng = np.random.default_rng([11, N, seed])
    F, rows = [], []
    for _ in range(2):
        f, dup = _exact_unit_rows(N, rng)
        F.append(f)
        rows.append(np.arange(N) if n_rows >= N else
                    np.concatenate([dup, _spread(max(0, n_rows - len(dup)), N, taken=dup)])[:n_rows])
    return np.stack(F), np.stack(rows).astype(np.int32)


def _call_knn_rows(F, rows, k):
    B, N, _ = F.shape
    out = torch.full((B, rows.shape[1], k), -1, dtype=torch.int32, device=DEV)
    h, st = _h()
    F_d, rows_d = torch.from_numpy(F).to(DEV), torch.from_numpy(rows).to(DEV)
    h.call("gmf_knn_rows", F_d.data_ptr(), rows_d.data_ptr(), B, N, rows.shape[1], k, out.data_ptr(), st)
    got = out.cpu().numpy()
    gmf_amd.check_status()
    return got


@pytest.mark.parametrize("k", [10, 63])
@pytest.mark.parametrize("N", [300, 2100, 16500])
def test_knn_rows_exact(N, k):
    """gmf_knn_rows, k <= 63: k_seed_dist (split-fp16 MFMA distance rows) + the register kernels, and the stream kernel at N = 16 500."""
    F, rows = _features_and_rows(N, 64, seed=k)
    got = _call_knn_rows(F, rows, k)
    for b in range(2):
        assert np.array_equal(got[b], _feature_knn(F[b], rows[b], k)), (N, k, b)


@pytest.mark.parametrize("k", [64, 100])
@pytest.mark.parametrize("N", [130, 2100])
def test_knn_rows_in_lds_exact(N, k):
    """gmf_knn_rows, k > 63: k_knn_seeds (fmaf distances into the LDS, k + 1 argmin rounds)."""
    F, rows = _features_and_rows(N, 64, seed=k)
    got = _call_knn_rows(F, rows, k)
    for b in range(2):
        assert np.array_equal(got[b], _feature_knn(F[b], rows[b], k)), (N, k, b)


def _plant_spread_winners(F, k, rng):
    """One row of F whose k + 1 nearest rows (itself included) have DISTINCT distances and lie in k + 1 DIFFERENT threads of
    the selection kernels (indices of different residues mod 256): the row becomes the unit vector of channel 64, k other rows
    get a distinct multiple of 2^-10 in (0, 1) there - its distance row is 0 for itself, 2 - 2 a for those, 2 elsewhere; every
    dot product in F stays exact.  Then the (k + 1)-th smallest of the 256 thread minima is the (k + 1)-th smallest entry itself,
    and a threshold taken one rank too low leaves exactly k candidates: the last neighbour would be missing.  (The tied rows
    cannot show that: their k-th and (k + 1)-th smallest thread minima are equal.)  Returns the row."""
    N = F.shape[0]
    res = rng.permutation(min(N, 256))[:k + 1]
    idx = res + 256 * rng.integers(0, (N - 1 - res) // 256 + 1)
    F[idx[0]] = 0.0
    F[idx[0], 64] = 1.0
    F[idx[1:], 64] = (1 + rng.permutation(1023)[:k]).astype(np.float32) / 1024
    row = (2.0 - 2.0 * F[:, 64].astype(np.float64))
    tmin = np.full(256, INF)
    np.minimum.at(tmin, np.arange(N) % 256, row)
    assert (row <= np.sort(tmin)[k]).sum() == k + 1 and (row <= np.sort(tmin)[k - 1]).sum() == k
    return idx[0]


@pytest.mark.parametrize("N", [300, 2100, 16500])
def test_pose_head_k64_neighbours_exact(N):
    """PointDSC(k = 64).pose_head with given seeds: k + 1 = 65 > 64 takes the threshold from the 256 THREAD minima, in
    k_knn_select_fast (N = 300, 2100) and in k_knn_select_stream (N = 16 500).  The first seed of each pair is a row whose 65
    nearest sit in 65 different threads (`_plant_spread_winners`), the others are the tied and duplicated rows.  Only
    aux["knn_idx"] is compared; the pose from such features means nothing."""
    m = gmf_amd.PointDSC(in_dim=6, num_layers=1, num_channels=128, num_iterations=10, ratio=0.02, inlier_threshold=0.10,
                         sigma_d=0.10, k=64, nms_radius=0.10)
    S = int(N * 0.02)
    F, rows = _features_and_rows(N, S, seed=64)
    rng = np.random.default_rng([13, N])
    for p in range(2):
        rows[p, 0] = _plant_spread_winners(F[p], 64, rng)
    b = synthetic.synthetic_batch([41, 42], N=N, T=1)
    logits = torch.zeros(2, N, device=DEV)
    _, _, aux = m.pose_head(torch.from_numpy(F).to(DEV), b["src_keypts"].to(DEV).contiguous(), b["tgt_keypts"].to(DEV).contiguous(),
                            logits, testing=True, seeds=torch.from_numpy(rows).to(DEV), return_aux=True, sigmas=(1.0, 0.10))
    got = aux["knn_idx"].cpu().numpy()
    gmf_amd.check_status()
    assert got.shape == (2, S, 64) and np.array_equal(aux["seeds"].cpu().numpy(), rows)
    for p in range(2):
        assert np.array_equal(got[p], _feature_knn(F[p], rows[p], 64)), (N, p)


def test_pose_head_ragged_neighbours_exact():
    """gmf_pose_head_ragged with knn_out / seeds_out: two pairs of 700 and 2300 correspondences in one launch sized and strided
    for the larger one (pair 0 runs k_knn_select_fast<20> on 700-element rows at the strides of 2300).  The first int(n ratio)
    seed rows of each pair equal the reference computed from the seeds the call returns; the slots behind them are zero."""
    n_points, ratio, k = [700, 2300], 0.1, 40
    rng = np.random.default_rng(23)
    F = [_exact_unit_rows(n, rng)[0] for n in n_points]
    scene = [synthetic.synthetic_batch([51 + i], N=n, T=1) for i, n in enumerate(n_points)]
    cat = lambda key: torch.cat([s[key][0] for s in scene]).to(DEV).contiguous()
    feat, src, tgt = torch.from_numpy(np.concatenate(F)).to(DEV), cat("src_keypts"), cat("tgt_keypts")
    total, B, S_max = sum(n_points), 2, int(max(n_points) * ratio)
    logits = torch.from_numpy(rng.permutation(total).astype(np.float32) / total).to(DEV)       # distinct scores
    pp = _lib.PoseParams()
    pp.num_seeds, pp.k, pp.num_iterations, pp.use_nms, pp.refine_iters = S_max, k, 10, 1, 20
    pp.sigma, pp.sigma_d, pp.inlier_threshold, pp.nms_radius, pp.refine_threshold = 1.0, 0.10, 0.10, 0.10, 0.10
    final_T, labels = torch.empty(B, 16, device=DEV), torch.empty(total, device=DEV)
    seeds = torch.full((B, S_max), -1, dtype=torch.int32, device=DEV)
    knn = torch.full((B, S_max, k), -1, dtype=torch.int32, device=DEV)
    h, st = _h()
    h.call("gmf_pose_head_ragged", pp, ratio, feat.data_ptr(), src.data_ptr(), tgt.data_ptr(), logits.data_ptr(),
           (ctypes.c_int * B)(*n_points), B, final_T.data_ptr(), labels.data_ptr(), seeds.data_ptr(), knn.data_ptr(), None, None, st)
    seeds, knn = seeds.cpu().numpy(), knn.cpu().numpy()
    gmf_amd.check_status()
    for p, n in enumerate(n_points):
        S = int(n * ratio)
        assert (seeds[p, :S] >= 0).all() and (seeds[p, :S] < n).all() and len(set(seeds[p, :S])) == S
        assert np.array_equal(knn[p, :S], _feature_knn(F[p], seeds[p, :S], k)), p
        assert not seeds[p, S:].any() and not knn[p, S:].any()


# ---- 3. the public knn on rows with bitwise duplicates ---------------------------------------------------------------------------
def _dup_sets():
    """(name, x [2, N, C] float32, normalized, float64 distances [2, N, N]) - all exact: unit 128-wide rows (gmf_knn_rows*), unit
    32-wide rows and unnormalised 33-wide integer rows (`_knn_general`, both distance forms), each with planted duplicates."""
    rng = np.random.default_rng(31)
    sets = []
    for name, C in (("unit128", 128), ("unit32", 32)):
        x = np.stack([_exact_unit_rows(300, rng, C=C)[0] for _ in range(2)])
        sets.append((name, x, True, 2.0 - 2.0 * np.einsum("bic,bjc->bij", x.astype(np.float64), x.astype(np.float64))))
    x = rng.integers(-2, 3, (2, 200, 33)).astype(np.float32) * rng.integers(1, 4, (2, 200, 1)).astype(np.float32)
    dup = rng.permutation(200)[:24]
    x[:, dup[:12]] = x[:, dup[12:]]
    x64 = x.astype(np.float64)
    sets.append(("int33", x, False, ((x64[:, :, None, :] - x64[:, None, :, :]) ** 2).sum(-1)))
    return sets


@pytest.fixture(scope="module")
def dup_sets():
    return {name: rest for name, *rest in _dup_sets()}


@pytest.mark.parametrize("ignore_self", [True, False])
@pytest.mark.parametrize("name,k", [("unit128", 20), ("unit128", 70), ("unit32", 20), ("int33", 9)])
def test_public_knn_with_duplicate_rows(dup_sets, name, k, ignore_self):
    """A row i with a bitwise duplicate j < i has d[i][j] == d[i][i], so rank 0 under (distance, index) is j, not i.
    ignore_self=True drops rank 0 whatever it is (the reference's topk(k + 1)[..., 1:]): ranks 1 .. k exactly.
    ignore_self=False: the row itself at position 0, and as a set the reference's top-k under (distance, index) - j included, i
    once.  k = 70 at 128 channels: more than 63 neighbours behind rank 0, the in-LDS selection."""
    x, normalized, d = dup_sets[name]
    B, N, _ = x.shape
    got = gmf_amd.knn(torch.from_numpy(x).to(DEV), k, ignore_self=ignore_self, normalized=normalized).cpu().numpy()
    gmf_amd.check_status()
    assert got.shape == (B, N, k) and got.min() >= 0 and got.max() < N
    order = np.argsort(d, axis=-1, kind="stable")
    own = np.arange(N)[None, :]
    assert (order[:, :, 0] != own).any(), "the set holds no row whose rank 0 is a duplicate: it would not show the defect"
    srt = np.sort(got, axis=-1)
    assert (srt[:, :, 1:] != srt[:, :, :-1]).all(), "an index occurs twice within a row"
    if ignore_self:
        assert np.array_equal(got, order[:, :, 1:k + 1])
    else:
        ref = order[:, :, :k]
        assert (ref == own[:, :, None]).any(-1).all()           # (fewer than k duplicates per row: the row is in its own top-k)
        assert np.array_equal(got[:, :, 0], np.broadcast_to(own, (B, N)))
        assert np.array_equal(srt, np.sort(ref, axis=-1))
