"""The shared high plane of the folded fp8 attention (csrc/kv_share_layout.hpp; PointDSC.py:56-64): under
"kv_fold" keys = values = f, so for a pair the "pv_fp8" guard lets through the linear kernel writes fp16(f) ONCE, in an image the
attention reads by rows for S = K Q'^T and transposed (ds_read_b64_tr_b16) for O^T += V^T P^T; the V tile carries its cross planes
only, and the attention's LDS holds a ring of four such planes.  A pair the guard trips keeps two full images.

Shapes: N in {32, 33, 95, 128, 160, 333} - 1, 2, 3, 4, 5 and 11 key tiles, i.e. the case without a pipelined tile, every wrap of
the four-slot ring, a last tile that is not full, workgroups with padding waves, more than one query block - and 333 / 700 with
"attn_key_splits" = 2 (items that start at a tile t != 0).  Pairs are passed as lists (a ragged call) with the small-grid forms
switched off, which is the two-launch plan at these sizes, "compat_16" = 2 and "kv_fold" = 1 (test_gpu_compat16.py's recipe).  Grids of fewer than "mid_grid_roles" (512) row blocks run the linear kernel as two roles,
which always writes a Q' image; every case therefore runs on both forms of the plan: WHOLE ("mid_grid_roles" = 0: k_linear_h2<3, true,
true> with its counted stage waits behind 24 or 32 image stores, Q' projected in the attention's prologue over the LDS that then
becomes the plane ring - the plan of the benchmark's grid - or, with "q_in_attention" = 0, k_linear_h2<3, false, true> and a q~ image)
and ROLES (k_linear_roles<true>).  The
guard's thresholds are set by pointing gmf_encoder_weights::pv_guard at a tensor of this file.  A wrong element of a value tile is an
O(1) error of the logits, so the 1e-4 distance to the fp32 oracle is a sharp check of every address."""
import ctypes

import pytest
import torch

import gmf_amd
from gmf_amd import _lib, synthetic
from oracle import gmf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORCE = dict(small_grid_roles=0, small_prologue_roles=0, attn_key_splits=1, ff_hidden_splits=1, compat_16=2, kv_fold=1)
PASS_ALL = [3.0e38] * 12
WHOLE, ROLES = dict(mid_grid_roles=0), dict(mid_grid_roles=512)
PLANS = pytest.mark.parametrize("plan", [WHOLE, ROLES], ids=["whole", "roles"])
KEYS = ("corr_pos", "src_keypts", "tgt_keypts")


@pytest.fixture(scope="module")
def sd_full():
    return synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 12, 128), seed=7)


def _model(sd, k):
    m = gmf_amd.PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1,
                         inlier_threshold=0.10, sigma_d=0.10, k=k, nms_radius=0.10)
    m.load_state_dict(sd, strict=False)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def model(sd_full):
    return _model(sd_full, 40)


K_SMALL = 16     # the pose head of a ragged batch wants more than k rows per pair: the pairs of 32 and 33 rows run with 16 neighbours


@pytest.fixture(scope="module")
def model_small_k(sd_full):
    return _model(sd_full, K_SMALL)


class _knobs:
    """set tuning knobs of the device's handle for a block, put back what was found"""
    def __init__(self, **kv):
        self.kv, self.h, self.old = kv, _lib.handle_for(0), {}

    def __enter__(self):
        for k, v in self.kv.items():
            cur = ctypes.c_int()
            self.h.call("gmf_get_tuning", k.encode(), ctypes.byref(cur))
            self.old[k] = cur.value
            self.h.call("gmf_set_tuning", k.encode(), v)
        return self.h

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.h.call("gmf_set_tuning", k.encode(), v)


class _thresholds:
    """the guard's per-layer thresholds (compared with max row |f_l|^2) replaced for a block: -1 trips, 3e38 lets through"""
    def __init__(self, model, values):
        self.pw = model._weights(torch.device(DEV))
        self.t = torch.tensor(values, dtype=torch.float32, device=DEV)

    def __enter__(self):
        torch.cuda.synchronize()
        self.saved = self.pw.struct.contents.pv_guard
        self.pw.struct.contents.pv_guard = self.t.data_ptr()

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.pw.struct.contents.pv_guard = self.saved


_pairs = {}      # (seed, n) -> [batch of one pair, fp32 oracle (logits, pose) or None, fp64 logits or None]


def _pair(seed, n):
    if (seed, n) not in _pairs:
        _pairs[seed, n] = [synthetic.synthetic_batch([seed], N=n, T=196), None, None]
    return _pairs[seed, n][0]


def _oracle32(sd, seed, n):
    """logits [1, n] and pose [1, 4, 4] of the fp32 oracle, computed once per pair (k as the model of that size has it)"""
    ent = _pairs[seed, n]
    if ent[1] is None:
        r = O.pointdsc_forward(sd, ent[0], k=40 if n > 40 else K_SMALL, testing=True)
        ent[1] = (r["logits"], r["final_trans"])
    return ent[1]


def _posed(sd, seed, n):
    """The first seed from `seed` on whose pair has a pose the REFERENCE determines: the fp32 and the fp64 evaluation of the oracle
    agree to 1e-5.  The pose head picks seeds and an argmax; on a near-tie the oracle's own two precisions give different poses (of
    the pairs of 33 rows about every second one: 1.5 apart at seed 2033 with logits 8e-6 apart), and a distance to such a pose checks
    nothing.  Decided from the oracle alone, before anything runs on the device."""
    while True:
        b = _pair(seed, n)
        k = 40 if n > 40 else K_SMALL
        sd64 = {kk: (v.double() if v.is_floating_point() else v) for kk, v in sd.items()}
        b64 = {kk: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for kk, v in b.items()}
        T64 = O.pointdsc_forward(sd64, b64, k=k, testing=True)["final_trans"]
        if float((_oracle32(sd, seed, n)[1].double() - T64).abs().max()) < 1e-5:
            return (seed, n)
        seed += 1


def _oracle64(sd, seed, n):
    ent = _pairs[seed, n]
    if ent[2] is None:
        b = ent[0]
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        b64 = {k: v.double() for k, v in b.items() if torch.is_tensor(v) and v.is_floating_point()}
        c64, _ = O.compat_matrix(b64["src_keypts"], b64["tgt_keypts"], 0.10)
        ent[2] = O.classifier(sd64, O.encoder(sd64, b64["corr_pos"], c64, b64["p_tokens"], b64["q_tokens"], 12))[0]
    return ent[2]


def _batch(spec, scale=None):
    """spec: [(seed, n), ...] -> the ragged input; scale: {index: factor on that pair's corr_pos}"""
    pairs = [_pair(s, n) for s, n in spec]
    rag = {k: [p[k][0].to(DEV).clone() for p in pairs] for k in KEYS}
    for i, f in (scale or {}).items():
        rag["corr_pos"][i] *= f
    rag.update(p_tokens=torch.cat([p["p_tokens"] for p in pairs]).to(DEV), q_tokens=torch.cat([p["q_tokens"] for p in pairs]).to(DEV),
               testing=True)
    return rag


def _run(model, data, **knobs):
    """(logits per pair, poses, labels per pair, guard bit) of one forward on the two-launch plan under the given knobs"""
    kv = dict(FORCE)
    kv.update(knobs)
    with _knobs(**kv) as h:
        h.status(clear=True)
        res = model(data)
        lg = [x.clone() for x in res["logits"]]
        lab = [x.clone() for x in res["final_labels"]]
        T = res["final_trans"].clone()
        torch.cuda.synchronize()
        flag = bool(h.status() & _lib.GMF_STATUS_PV_GUARDED)
        h.status(clear=True)
    return lg, T, lab, flag


def _pair_same(a, i, b, j):
    """pair i of run a and pair j of run b: the same logits, pose and labels, bit for bit"""
    return torch.equal(a[0][i], b[0][j]) and torch.equal(a[1][i], b[1][j]) and torch.equal(a[2][i], b[2][j])


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(_pair_same(a, i, b, i) for i in range(len(a[0])))


def _near_oracle(sd, spec, run, what):
    """per pair: logits and pose within 1e-4 of the fp32 oracle"""
    bad = []
    for i, (seed, n) in enumerate(spec):
        lg, T = _oracle32(sd, seed, n)
        el = float((run[0][i].cpu() - lg[0]).abs().max())
        eT = float((run[1][i].cpu() - T[0]).abs().max())
        print(f"{what}: pair (seed {seed}, N = {n}): logits {el:.2e}, pose {eT:.2e} from the fp32 oracle")
        if not (el < 1e-4 and eT < 1e-4):
            bad.append((seed, n, el, eT))
    assert not bad, (what, bad)


@pytest.mark.parametrize("n", [32, 33, 95, 128, 160, 333])
def test_every_ring_wrap_against_the_oracle(model, model_small_k, sd_full, n):
    """Two pairs of N rows with every layer let through: logits and pose within 1e-4 of the fp32 oracle and no guard bit; the first
    pair keeps its bits in another batch and slot (behind a pair of another size), and with the Q' projection in the linear kernel
    ("q_in_attention" = 0 on the whole kernel: the attention reads a q~ image) instead of in the attention's prologue, and with the
    linear kernel as two roles."""
    model = model if n > 40 else model_small_k
    spec = [_posed(sd_full, 1000 + n, n), _posed(sd_full, 2000 + n, n)]
    other = [(3000 + n, 95 if n != 95 else 160), spec[0]]
    with _thresholds(model, PASS_ALL):
        a = _run(model, _batch(spec), **WHOLE)
        b = _run(model, _batch(other), **WHOLE)
        q = _run(model, _batch(spec), q_in_attention=0, **WHOLE)
        r = _run(model, _batch(spec), **ROLES)
    gmf_amd.check_status()
    assert not a[3] and not b[3] and not q[3] and not r[3]
    _near_oracle(sd_full, spec, a, f"N = {n}")
    assert _pair_same(a, 0, b, 1)
    assert _same(a, q)
    assert _same(a, r)


@pytest.mark.parametrize("n", [333, 700])
def test_key_split_items(model, sd_full, n):
    """ "attn_key_splits" = 2: every item is two workgroups, the second of which starts at key tile t != 0 (ring slots and scale words
    follow the absolute tile index), and k_scattn_merge finishes.  Within 1e-4 of the fp32 oracle, the same bits in a second run and
    wherever Q' is projected.  (With key splits a pair's bits depend on the grid it shares - which items are split is a matter of
    the whole grid, test_gpu_compat16.py - so there is no second batch here.)"""
    spec = [_posed(sd_full, 1000 + n, n), _posed(sd_full, 2000 + n, n)]
    with _thresholds(model, PASS_ALL):
        a = _run(model, _batch(spec), attn_key_splits=2, **WHOLE)
        b = _run(model, _batch(spec), attn_key_splits=2, **WHOLE)
        q = _run(model, _batch(spec), attn_key_splits=2, q_in_attention=0, **WHOLE)
        r = _run(model, _batch(spec), attn_key_splits=2, **ROLES)
    gmf_amd.check_status()
    assert not a[3]
    _near_oracle(sd_full, spec, a, f"N = {n}, two key splits")
    assert _same(a, b)
    assert _same(a, q)
    assert _same(a, r)


@PLANS
def test_a_tripped_pair_between_shared_ones_over_stale_images(model, plan):
    """The guard decides per pair and layer, from the pair's largest row |f_l|^2 against the layer's threshold.  One pair of three
    with 40 x larger inputs trips its first layers (two full images) while its neighbours write and read the shared form, and the
    forward runs right after one of a different, larger batch, so every slot of the workspace holds another batch's images: the
    ordinary pairs keep the bits they have in a batch without the hot pair and the bits of the fp8 form without a guard ("pv_fp8" =
    2), the hot pair the bits it has in a batch of its own.  (The thresholds are per layer, so a single pair is tripped through
    its inputs, as in test_gpu_compat16.py.)
    With a threshold of -1 in every layer every pair trips: each then has the bits of "pv_fp8" = 0 on the fp32 cache (images without
    e4m3 planes), again over the stale images of a forward that used the shared form."""
    spec = [(1100, 333), (1101, 160), (1102, 95)]
    stale = _batch([(1110, 700), (1111, 333), (1112, 333)])

    def run(m, d, **kv):
        return _run(m, d, **kv, **plan)
    clean = run(model, _batch(spec))
    hot_alone = run(model, _batch(spec[1:2], scale={0: 40.0}))
    run(model, stale)
    hot = run(model, _batch(spec, scale={1: 40.0}))
    gmf_amd.check_status()
    assert hot[3] and hot_alone[3] and not clean[3]
    assert torch.isfinite(hot[0][1]).all() and not torch.equal(hot[0][1], clean[0][1])
    assert _pair_same(hot, 0, clean, 0) and _pair_same(hot, 2, clean, 2)
    assert _pair_same(hot, 1, hot_alone, 0)
    uncond = run(model, _batch(spec), pv_fp8=2)         # the fp8 form without a guard
    assert _pair_same(hot, 0, uncond, 0) and _pair_same(hot, 2, uncond, 2)
    plain = run(model, _batch(spec), pv_fp8=0, compat_16=0)
    run(model, stale)
    with _thresholds(model, [-1.0] * 12):
        tripped = run(model, _batch(spec))
    assert tripped[3] and not plain[3]
    assert _same(tripped, plain)
    assert not torch.equal(tripped[0][0], clean[0][0])


@PLANS
def test_layers_alternating_between_the_two_forms(model, sd_full, plan):
    """Thresholds -1, 3e38, -1, ...: a pair's V slot holds a full image in one layer and cross planes behind a stale high plane in
    the next.  Finite, inside the contract test_gpu_compat16.py sets for mixed pairs (1.5 x floor + 2e-5 from the fp64 evaluation,
    floor = the fp32 oracle's own distance from it, and 1e-4 from the fp32 oracle), and two runs are bit-equal."""
    spec = [(1200, 333), (1201, 95), (1202, 160)]
    data = _batch(spec)
    with _thresholds(model, [-1.0, 3.0e38] * 6):
        a = _run(model, data, **plan)
        b = _run(model, data, **plan)
    with _thresholds(model, [3.0e38, -1.0] * 6):
        c = _run(model, data, **plan)
        d = _run(model, data, **plan)
    gmf_amd.check_status()
    assert a[3] and c[3]
    assert _same(a, b) and _same(c, d)
    for run, what in ((a, "odd layers shared"), (c, "even layers shared")):
        for (seed, n), x in zip(spec, run[0]):
            assert torch.isfinite(x).all()
            o32, o64 = _oracle32(sd_full, seed, n)[0][0], _oracle64(sd_full, seed, n)
            floor = float((o32.double() - o64).abs().max())
            e64, e32 = float((x.cpu().double() - o64).abs().max()), float((x.cpu() - o32).abs().max())
            print(f"{what}: pair (seed {seed}, N = {n}): vs fp64 {e64:.2e} (floor {floor:.2e}, bound {1.5 * floor + 2e-5:.2e}), vs fp32 oracle {e32:.2e}")
            assert e64 <= 1.5 * floor + 2e-5, (what, seed, n, e64, floor)
            assert e32 < 1e-4, (what, seed, n, e32)
        assert torch.isfinite(run[1]).all()
