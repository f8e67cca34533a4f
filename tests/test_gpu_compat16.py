"""The guarded 16-bit compat cache of the two-launch plan (gmf_set_tuning "compat_16" = 1, the default; DESIGN section 4;
PointDSC.py:56-64, 216-221): per pair and layer the attention streams c as rint(65535 c) where the "pv_fp8" guard lets the fp8
products through, and an exact fp32 cache - built on the device for the pairs that trip, once per forward - where it trips.

Shapes: B = 2 or 3 pairs of N in {95, 128, 333, 700} (a last tile that is not full, exactly four tiles, a workgroup with padding
waves, more than one query block), passed as lists (a ragged call) with the small-grid forms switched off, which is the
two-launch plan at these sizes, and "compat_16" = 2, which grants the guarded cache on every grid of that plan (the default, 1,
asks for 256 row blocks); key and hidden splits are off unless a test asks for them, so a pair's bits do not depend on the grid it
shares.  The guard's thresholds are set by pointing gmf_encoder_weights::pv_guard at a tensor of this file."""
import ctypes

import pytest
import torch

import gmf_amd
from gmf_amd import _lib, synthetic
from oracle import gmf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORCE = dict(small_grid_roles=0, small_prologue_roles=0, attn_key_splits=1, ff_hidden_splits=1, compat_16=2)
# max |logit(kv_fold 1) - logit(kv_fold 0)| of the PARENT build (the fp32 cache) over 8 seeded pairs of each size of this file,
# measured once on MI355X with tests/tools/compat16_outputs.py --fold-parent (profiles/compat16_outputs.txt)
PARENT_FOLD_DIFF = 3.606e-05


@pytest.fixture(scope="module")
def sd_full():
    return synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 12, 128), seed=7)


@pytest.fixture(scope="module")
def model(sd_full):
    m = gmf_amd.PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1,
                         inlier_threshold=0.10, sigma_d=0.10, k=40, nms_radius=0.10)
    m.load_state_dict(sd_full, strict=False)
    return m.to(DEV).eval()


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


_pairs_cache = {}


def _pair(seed, n):
    """one seeded 3DMatch-shape pair with its fp32-oracle and fp64 logits (computed once per module)"""
    if (seed, n) not in _pairs_cache:
        b = synthetic.synthetic_batch([seed], N=n, T=196)
        _pairs_cache[seed, n] = [b, None]
    return _pairs_cache[seed, n][0]


def _refs(sd, seed, n):
    ent = _pairs_cache[seed, n]
    if ent[1] is None:
        b = ent[0]
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        b64 = {k: v.double() for k, v in b.items() if torch.is_tensor(v) and v.is_floating_point()}
        c64, _ = O.compat_matrix(b64["src_keypts"], b64["tgt_keypts"], 0.10)
        c32, _ = O.compat_matrix(b["src_keypts"], b["tgt_keypts"], 0.10)
        o64 = O.classifier(sd64, O.encoder(sd64, b64["corr_pos"], c64, b64["p_tokens"], b64["q_tokens"], 12))[0]
        o32 = O.classifier(sd, O.encoder(sd, b["corr_pos"], c32, b["p_tokens"], b["q_tokens"], 12))[0]
        ent[1] = (o32, o64)
    return ent[1]


def _batch(spec, scale=None):
    """spec: [(seed, n), ...] -> the ragged input; scale: {index: factor on that pair's corr_pos}"""
    pairs = [_pair(s, n) for s, n in spec]
    rag = {k: [p[k][0].to(DEV).clone() for p in pairs] for k in ("corr_pos", "src_keypts", "tgt_keypts")}
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


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def _maxdiff(a, b):
    return max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))


def _contract(sd, spec, lg, what):
    """logits within 1.5 x floor + 2e-5 of the fp64 evaluation (floor: the fp32 oracle against fp64) and within 1e-4 of the fp32 oracle"""
    for (seed, n), x in zip(spec, lg):
        o32, o64 = _refs(sd, seed, n)
        floor = float((o32.double() - o64).abs().max())
        e64, e32 = float((x.cpu().double() - o64).abs().max()), float((x.cpu() - o32).abs().max())
        print(f"{what}: pair (seed {seed}, N = {n}): vs fp64 {e64:.2e} (floor {floor:.2e}, bound {1.5 * floor + 2e-5:.2e}), vs fp32 oracle {e32:.2e}")
        assert e64 <= 1.5 * floor + 2e-5, (what, seed, n, e64, floor)
        assert e32 < 1e-4, (what, seed, n, e32)


@pytest.mark.parametrize("case", ["95x2", "128x3", "333x2", "700x2", "700x2-keysplit"])
def test_default_is_the_16bit_cache_inside_the_contract(model, sd_full, case):
    """Seeded well-conditioned weights, 3DMatch-shape pairs: the default is bit-identical (logits, poses, labels) to the
    unconditional 16-bit cache ("compat_format" = 2), other bits than the fp32 cache ("compat_16" = 0), inside the contract of the
    default numerics, and the status has no guard bit.  `keysplit`: the items divided by keys over two workgroups + k_scattn_merge."""
    n, B = (int(v) for v in case.split("-")[0].split("x"))
    extra = {"attn_key_splits": 2} if case.endswith("keysplit") else {}
    spec = [(900 + i, n) for i in range(B)]
    data = _batch(spec)
    d = _run(model, data, **extra)
    u = _run(model, data, compat_format=2, **extra)
    off = _run(model, data, compat_16=0, **extra)
    gmf_amd.check_status()
    print(f"{case}: default vs fp32 cache: max |dlogit| {_maxdiff(d[0], off[0]):.2e}")
    assert _same(d, u)
    assert not all(torch.equal(x, y) for x, y in zip(d[0], off[0]))
    assert not d[3] and not u[3]
    _contract(sd_full, spec, d[0], f"compat_16 default, {case}")


def test_knob_off_is_the_fp32_cache_and_deterministic(model):
    """"compat_16" = 0 twice in a row, the second time with "compat_format" = 0 spelled out: equal bits (the knob is inert when off,
    and the forward is deterministic); gmf_get_tuning returns what was set, the default is 1 (which leaves these small grids on the
    fp32 cache), values beyond 2 are refused."""
    data = _batch([(910, 333), (911, 700), (912, 128)])
    h = _lib.handle_for(0)
    cur = ctypes.c_int()
    h.call("gmf_get_tuning", b"compat_16", ctypes.byref(cur))
    assert cur.value == 1
    a = _run(model, data, compat_16=0)
    with _knobs(compat_16=0):
        h.call("gmf_get_tuning", b"compat_16", ctypes.byref(cur))
        assert cur.value == 0
    b = _run(model, data, compat_16=0, compat_format=0)
    c = _run(model, data)
    e = _run(model, data)
    s = _run(model, data, compat_16=1)
    assert _same(a, b) and _same(c, e) and _same(a, s)
    assert not all(torch.equal(x, y) for x, y in zip(a[0], c[0]))
    assert h.lib.gmf_set_tuning(h.h, b"compat_16", 3) == -1


def test_a_hot_pair_leaves_its_neighbour_alone(model):
    """One ordinary pair and one pair with 40 x larger inputs (its first layers trip the guard and stream the lazily built fp32
    cache): the status carries the guard bit, the hot pair's logits are finite, and the ordinary pair keeps the bits it has in the
    same batch with an ordinary neighbour AND in a batch of its own."""
    spec = [(920, 333), (921, 700)]
    cool = _run(model, _batch(spec))
    hot = _run(model, _batch(spec, scale={1: 40.0}))
    alone = _run(model, _batch(spec[:1]))
    assert hot[3] and not cool[3]
    assert torch.isfinite(hot[0][1]).all()
    assert not torch.equal(hot[0][1], cool[0][1])
    assert torch.equal(hot[0][0], cool[0][0]) and torch.equal(hot[2][0], cool[2][0]) and torch.equal(hot[1][0], cool[1][0])
    assert torch.equal(hot[0][0], alone[0][0]) and torch.equal(hot[2][0], alone[2][0]) and torch.equal(hot[1][0], alone[1][0])


@pytest.mark.parametrize("splits", [1, 2])
def test_every_layer_tripped_is_the_fp32_cache_bit_for_bit(model, splits):
    """Thresholds that trip every layer of every pair: every attention workgroup streams the lazily built fp32 cache, and the result
    is bit-identical to "compat_16" = 0 under the same thresholds - the lazy cache holds the bytes k_compat_build<0> writes.
    (splits = 2: through the key-split items and k_scattn_merge as well.)"""
    data = _batch([(930, 128), (931, 333), (932, 700)])
    with _thresholds(model, [-1.0] * 12):
        a = _run(model, data, attn_key_splits=splits)
        b = _run(model, data, compat_16=0, attn_key_splits=splits)
    assert a[3] and b[3]
    assert _same(a, b)


def test_tripping_from_layer_4_on(model, sd_full):
    """Thresholds that let layers 0-3 through and trip layers 4-11: the fp32 cache is first built before layer 4's attention and
    read by eight layers.  No arrangement of the knobs runs "16 bits in layers 0-3, an fp32 cache built up front afterwards", so
    the comparison is with the decision per layer through the contract: the logits are inside 1.5 x floor + 2e-5 of the fp64
    evaluation and 1e-4 of the fp32 oracle (a cache that was not built, or built for the wrong pair, is off by orders of
    magnitude), and they differ from the all-fp32-cache run only by what four layers of 16-bit c can give (printed)."""
    spec = [(940, 333), (941, 700), (942, 95)]
    data = _batch(spec)
    with _thresholds(model, [3.0e38] * 4 + [-1.0] * 8):
        a = _run(model, data)
        b = _run(model, data, compat_16=0)
    assert a[3] and b[3]
    print(f"tripping from layer 4 on: vs the fp32 cache under the same thresholds: max |dlogit| {_maxdiff(a[0], b[0]):.2e}")
    assert not all(torch.equal(x, y) for x, y in zip(a[0], b[0]))      # layers 0-3 did read 16 bits
    _contract(sd_full, spec, a[0], "tripping from layer 4 on")


def test_ragged_pairs_equal_their_uniform_batches(model):
    """333 and 700 rows in one launch: each pair is bit-identical to the same pair in a batch of two pairs of its own size."""
    rag = _run(model, _batch([(950, 333), (951, 700)]))
    u333 = _run(model, _batch([(950, 333), (952, 333)]))
    u700 = _run(model, _batch([(953, 700), (951, 700)]))
    assert torch.equal(rag[0][0], u333[0][0]) and torch.equal(rag[1][0], u333[1][0]) and torch.equal(rag[2][0], u333[2][0])
    assert torch.equal(rag[0][1], u700[0][1]) and torch.equal(rag[1][1], u700[1][1]) and torch.equal(rag[2][1], u700[2][1])


def test_fold_and_no_fold(model, sd_full):
    """"kv_fold" 1 and 0 under the default cache: both inside the contract, and no further apart than the two forms are on the
    parent build's fp32 cache (PARENT_FOLD_DIFF, measured once)."""
    spec = [(960, 95), (961, 128), (962, 333), (963, 700)]
    worst = 0.0
    for part in (spec[:2], spec[2:]):
        data = _batch(part)
        f1 = _run(model, data, kv_fold=1)
        f0 = _run(model, data, kv_fold=0)
        _contract(sd_full, part, f1[0], "kv_fold 1")
        _contract(sd_full, part, f0[0], "kv_fold 0")
        worst = max(worst, _maxdiff(f1[0], f0[0]))
    print(f"folded vs unfolded under the guarded 16-bit cache: max |dlogit| {worst:.2e} (parent build: {PARENT_FOLD_DIFF})")
    assert worst > 0.0
    assert worst <= PARENT_FOLD_DIFF, (worst, PARENT_FOLD_DIFF)
