"""The "kv_fold" form of the large-grid attention (gmf_set_tuning "kv_fold" = 1, the default on the two-launch plan; DESIGN
section 4; PointDSC.py:56-64): the key and value tiles are the layer input f itself, the K projection is composed into the query
side (q~ = (Wk^T Wq') f + Wk^T bq', every score accumulator starts from beta = (Wq'^T bk) . f + bk . bq') and the V projection into
fc_message's first layer.  All shapes are the smallest large-grid shapes the suite already uses: 33 x 1000 (264 row blocks: the
linear kernel as two roles, a partial last tile, padding waves), 9 x 3970 and the ragged sizes [700, 1531, 5000, 257]."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import _lib, synthetic
from oracle import gmf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("corr_pos", "src_keypts", "tgt_keypts", "p_tokens", "q_tokens")
RAGGED = [700, 1531, 5000, 257]


def _maxerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


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


def _uniform(seeds, N):
    b = synthetic.synthetic_batch(seeds, N=N, T=196)
    data = {k: b[k].to(DEV) for k in KEYS}
    data["testing"] = True
    return b, data


def _ragged(first_seed, sizes):
    pairs = [synthetic.synthetic_batch([first_seed + i], N=n, T=196) for i, n in enumerate(sizes)]
    rag = {k: [p[k][0].to(DEV) for p in pairs] for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    rag.update(p_tokens=torch.cat([p["p_tokens"] for p in pairs]).to(DEV), q_tokens=torch.cat([p["q_tokens"] for p in pairs]).to(DEV),
               testing=True)
    return pairs, rag


def _run(model, data, **knobs):
    """logits (list per pair), poses, labels (list per pair) of one forward under the given knobs"""
    with _knobs(**knobs):
        res = model(data)
        if isinstance(data["corr_pos"], list):
            lg = [x.clone() for x in res["logits"]]
            lab = [x.clone() for x in res["final_labels"]]
        else:
            lg = [x.clone() for x in model.last_logits]
            lab = [x.clone() for x in res["final_labels"]]
        T = res["final_trans"].clone()
    torch.cuda.synchronize()
    return lg, T, lab


@pytest.mark.parametrize("shape", ["33x1000", "9x3970", "ragged", "ragged_x2"])
def test_fold_against_the_oracle(model, sd_full, shape):
    """With "kv_fold" = 1 pair 0's logits and pose are within 1e-4 of the fp32 oracle (PointDSC.py:56-64 evaluated with the K and V
    projections as the reference writes them); the folded and the unfolded form give identical inlier labels on every pair."""
    if shape.startswith("ragged"):
        # (the four ragged sizes are 160 row blocks: the plan gives them the three-launch form of small grids, which does not fold -
        # the knob changes nothing there; twice the sizes, 320 row blocks, run the two-launch plan)
        pairs, data = _ragged(300, RAGGED * (2 if shape == "ragged_x2" else 1))
        b0 = pairs[0]
    else:
        B, N = (int(v) for v in shape.split("x"))
        b, data = _uniform(list(range(700, 700 + B)), N)
        b0 = {k: v[:1] for k, v in b.items()}
    lg1, T1, lab1 = _run(model, data, kv_fold=1)
    lg0, T0, lab0 = _run(model, data, kv_fold=0)
    gmf_amd.check_status()
    ref = O.pointdsc_forward(sd_full, b0, testing=True)
    dl, dT = _maxerr(lg1[0].cpu(), ref["logits"][0]), _maxerr(T1[0].cpu(), ref["final_trans"][0])
    d01 = max(_maxerr(a.cpu(), b_.cpu()) for a, b_ in zip(lg1, lg0))
    print(f"kv_fold {shape}: pair 0 vs fp32 oracle: logits {dl:.2e}, pose {dT:.2e}; folded vs unfolded, all pairs: {d01:.2e}")
    assert dl < 1e-4, dl
    assert dT < 1e-4, dT
    assert all(torch.equal(a, b_) for a, b_ in zip(lab1, lab0))
    assert (d01 > 0.0) == (shape != "ragged")      # (on the two-launch plan the knob selects another arithmetic)


def test_fold_on_the_stress_set():
    """Golden F22's stress pair (KITTI shape, N = 2000, the seeded weights as they are: the reference's own fp32 evaluation is 3e-4
    from fp64 there) in a large-grid batch of 17 copies, "kv_fold" = 1 under the default guard: no further from the fp64 evaluation
    than 1.5 x floor + 2e-5, floor = the fp32 oracle against fp64 (computed here)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f22_kitti_branch.npz"))
    N, seed = (int(v) for v in g["cases"][1])
    assert N == 2000
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 12, 128), seed=7, sigma_d=float(g["sigma_d"]))
    m = gmf_amd.PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1,
                         inlier_threshold=1.2, sigma_d=1.2, k=40, nms_radius=1.2)
    m.load_state_dict(sd, strict=False)
    m = m.to(DEV).eval()
    b = synthetic.synthetic_batch([seed], N=N, T=196, kind="kitti")
    copies = 17                                    # 17 x 16 row blocks = 272: the two-launch plan
    data = {k: b[k].to(DEV).expand(copies, *b[k].shape[1:]).contiguous() for k in KEYS}
    data["testing"] = True
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = {k: v.double() for k, v in b.items()}
    compat, _ = O.compat_matrix(b64["src_keypts"], b64["tgt_keypts"], 1.2)
    o64 = O.classifier(sd64, O.encoder(sd64, b64["corr_pos"], compat, b64["p_tokens"], b64["q_tokens"], 12))[0]
    compat32, _ = O.compat_matrix(b["src_keypts"], b["tgt_keypts"], 1.2)
    o32 = O.classifier(sd, O.encoder(sd, b["corr_pos"], compat32, b["p_tokens"], b["q_tokens"], 12))[0]
    floor = float((o32.double() - o64).abs().max())
    h = _lib.handle_for(0)
    h.status(clear=True)
    lg1, _, _ = _run(m, data, kv_fold=1)
    tripped = bool(h.status() & _lib.GMF_STATUS_PV_GUARDED)
    h.status(clear=True)
    lg0, _, _ = _run(m, data, kv_fold=0)
    h.status(clear=True)
    e1 = max(float((x.cpu().double() - o64).abs().max()) for x in lg1)
    e0 = max(float((x.cpu().double() - o64).abs().max()) for x in lg0)
    print(f"stress pair N = {N} x {copies}: vs fp64: folded {e1:.2e}, unfolded {e0:.2e}, fp32 oracle {floor:.2e} "
          f"(bound {1.5 * floor + 2e-5:.2e})")
    assert tripped                                 # the guard rule is the unfolded one: this network trips it
    assert all(torch.equal(x, lg1[0]) for x in lg1)              # copies of one pair: one result
    assert e1 < 1.5 * floor + 2e-5, (e1, floor)


def test_knob(model):
    """"kv_fold" = 0 is the unfolded form bit for bit: the same seeded batch run with 0, 1, 0 gives equal bits in the two runs with 0
    (logits, poses, labels) and other bits with 1; gmf_get_tuning returns what was set; other values are refused."""
    _, data = _uniform(list(range(40, 49)), 3970)
    h = _lib.handle_for(0)
    cur = ctypes.c_int()
    h.call("gmf_get_tuning", b"kv_fold", ctypes.byref(cur))
    assert cur.value == 1                          # the default
    a = _run(model, data, kv_fold=0)
    with _knobs(kv_fold=0):
        h.call("gmf_get_tuning", b"kv_fold", ctypes.byref(cur))
        assert cur.value == 0
    h.call("gmf_get_tuning", b"kv_fold", ctypes.byref(cur))
    assert cur.value == 1
    b = _run(model, data, kv_fold=1)
    c = _run(model, data, kv_fold=0)
    assert torch.equal(torch.stack(a[0]), torch.stack(c[0])) and torch.equal(a[1], c[1]) and torch.equal(torch.stack(a[2]), torch.stack(c[2]))
    assert not torch.equal(torch.stack(a[0]), torch.stack(b[0]))
    assert h.lib.gmf_set_tuning(h.h, b"kv_fold", 2) == -1
    # the forms the suite compares bit for bit fold together (this grid runs the linear kernel as two roles by default): the single
    # kernel with q~ projected in the attention prologue, and the single kernel writing a q~ image
    for extra in ({"mid_grid_roles": 0}, {"mid_grid_roles": 0, "q_in_attention": 0}):
        d = _run(model, data, kv_fold=1, **extra)
        assert torch.equal(torch.stack(b[0]), torch.stack(d[0])) and torch.equal(b[1], d[1]), extra


def test_guard_under_the_fold(model, sd_full):
    """The guard rule is the unfolded one (the statistic, the thresholds, the decision per pair AND per layer): an ordinary batch is
    bit-identical to the unconditional fp8 form ("pv_fp8" = 2), status bit clear; with one pair's inputs 40 x larger the bit is set,
    that pair leaves the fp8 form's bits and the other pairs keep theirs.
    A pair whose EVERY layer is guarded equals its three-product bits ("pv_fp8" = 0): weights whose projection biases alone pass the
    score bound, and a weights block without thresholds (pv_guard = NULL).  The 40 x pair itself does not: the guard decides per
    layer, only its first layers trip, and the later ones multiply on the fp8 pipe - 3.7e-5 from its "pv_fp8" = 0 logits with the
    fold, 4.7e-5 without it (measured; the unfolded form has the same property, which is asserted here)."""
    h = _lib.handle_for(0)
    B, N = 9, 3970
    _, data = _uniform(list(range(520, 520 + B)), N)
    hot = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()}
    hot["corr_pos"][1] *= 40.0

    def run(m, d, pv, fold=1):
        h.status(clear=True)
        lg = torch.stack(_run(m, d, kv_fold=fold, pv_fp8=pv)[0])
        flag = bool(h.status() & _lib.GMF_STATUS_PV_GUARDED)
        h.status(clear=True)
        return lg, flag
    lg1, t1 = run(model, data, 1)
    lg2, t2 = run(model, data, 2)
    assert torch.equal(lg1, lg2) and not t1 and not t2
    hg1, ht1 = run(model, hot, 1)
    hg2, ht2 = run(model, hot, 2)
    hg0, _ = run(model, hot, 0)
    assert ht1 and not ht2 and torch.isfinite(hg1).all()
    others = [i for i in range(B) if i != 1]
    assert not torch.equal(hg1[1], hg2[1])
    assert torch.equal(hg1[others], lg1[others]) and torch.equal(hg1[others], hg2[others])
    u1, _ = run(model, hot, 1, fold=0)
    u0, _ = run(model, hot, 0, fold=0)
    print(f"guard under the fold: hot pair, guarded vs three products: folded {_maxerr(hg1[1].cpu(), hg0[1].cpu()):.2e}, "
          f"unfolded {_maxerr(u1[1].cpu(), u0[1].cpu()):.2e}")
    assert torch.equal(hg1[1], hg0[1]) == torch.equal(u1[1], u0[1])      # (per-layer decision: the same property in both forms)
    # every layer guarded: the three-product bits
    sd = dict(sd_full)
    for layer in range(12):
        for proj in ("projection_q", "projection_k"):
            key = f"encoder.blocks.NonLocal_layer_{layer}.{proj}.bias"
            sd[key] = torch.full_like(sd[key], 20.0)
    m = gmf_amd.PointDSC(num_layers=12)
    m.load_state_dict(sd, strict=False)
    m = m.to(DEV).eval()
    g1, gt1 = run(m, data, 1)
    g0, _ = run(m, data, 0)
    g2, _ = run(m, data, 2)
    assert gt1 and torch.isfinite(g1).all()
    assert torch.equal(g1, g0) and not torch.equal(g1, g2)
    # pv_guard = NULL: the guarded default is the three-product form
    pw = model._weights(data["corr_pos"].device)
    saved = pw.struct.contents.pv_guard
    lg0, _ = run(model, data, 0)
    try:
        pw.struct.contents.pv_guard = None
        n1, nt1 = run(model, data, 1)
    finally:
        pw.struct.contents.pv_guard = saved
    assert torch.equal(n1, lg0) and not nt1


def test_ragged_fold_equals_per_pair_calls(model):
    """The ragged sizes with the knob on against each pair's own B = 1 call (small grid: the unfolded three-launch form), at the 5e-5
    of test_ragged_batch_equals_per_pair_calls: once as they are (160 row blocks: the plan's small-grid form, which the knob leaves
    alone) and once twice over (320 row blocks: the two-launch plan, folded; measured 1.3e-5 .. 3.6e-5)."""
    pairs, rag = _ragged(300, RAGGED)
    lg, T, _ = _run(model, rag, kv_fold=1)
    pairs2, rag2 = _ragged(300, RAGGED * 2)
    lg2, T2, _ = _run(model, rag2, kv_fold=1)
    gmf_amd.check_status()
    for i, b in enumerate(pairs):
        one = {k: b[k].to(DEV) for k in KEYS}
        one["testing"] = True
        r1 = model(one)
        dl = _maxerr(lg[i].cpu(), model.last_logits[0].cpu())
        dT = _maxerr(T[i].cpu(), r1["final_trans"][0].cpu())
        dl2 = _maxerr(lg2[i].cpu(), model.last_logits[0].cpu())          # (pairs 0..3 of the doubled batch are the same scenes)
        dT2 = _maxerr(T2[i].cpu(), r1["final_trans"][0].cpu())
        print(f"ragged pair {i} (N = {RAGGED[i]}) vs its B = 1 call: max |dlogit| {dl:.2e}, max |dT| {dT:.2e}; "
              f"in the doubled batch (folded) {dl2:.2e}, {dT2:.2e}")
        assert dl < 5e-5 and dl2 < 5e-5, (i, dl, dl2)
        assert dT < 1e-4 and dT2 < 1e-4, (i, dT, dT2)
