"""GPU tests of FCGF's training path - the narrow-input weight gradient, the row normalisation y / (||y|| + 1e-8), the
hardest-contrastive loss, gmf_amd.train.fcgf_train and one optimisation run - against the float64 restatements of
tests/fcgf_train_reference.py, with the bound of test_train_gradients.check_close (float64 reference, float32 floor x 4)."""
import os

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import fcgf
from gmf_amd import sparse as SP
from gmf_amd import train as T

import fcgf_reference as FR
import fcgf_train_reference as FTR
import sparse_reference as SR
import sparse_train_reference as STR
from test_train_gradients import check_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_coords(M, D, span, batches, seed):
    """test_gpu_sparse_train._random_coords: M unique rows (batch, c_1 .. c_D) with c in [-span, span), shuffled."""
    rng = np.random.default_rng(seed)
    rows = set()
    while len(rows) < M:
        rows.add((int(rng.choice(batches)),) + tuple(int(v) for v in rng.integers(-span, span, D)))
    out = np.array(sorted(rows), dtype=np.int64)
    return out[rng.permutation(M)]


_SETS = {}


def _set(name):
    if name not in _SETS:
        _SETS[name] = {"d3": lambda: _random_coords(700, 3, 7, [0, 1, 2], 11),           # test_gpu_sparse_train's "d3"
                       "d3_sparse": lambda: _random_coords(120, 3, 12, [0, 1], 13),
                       "d3_two": lambda: _random_coords(700, 3, 7, [0, 1], 14)}[name]()
    return _SETS[name]


# ---- narrow-input weight gradient --------------------------------------------------------------------------------------------

_MAPS = {}


def _conv1_map(set_name, k):
    """(plan with the one map (k, 0, 0), host map, DeviceMap) of a set, built once."""
    if (set_name, k) not in _MAPS:
        rows = _set(set_name)
        plan = SP.SparsePlan(torch.as_tensor(rows).to(DEV).int(), 1, [(k, 0, 0)])
        cmap = SR.map_between(SR.build_levels(rows, 1), k, 0, 0)
        _MAPS[(set_name, k)] = (plan, cmap, STR.DeviceMap(cmap, len(rows), DEV))
    return _MAPS[(set_name, k)]


def _wgrad_reference(x, dy, dmap, K, n):
    ref = {}
    for dt in (torch.float64, torch.float32):
        W = torch.zeros(K, x.shape[1], dy.shape[1], device=DEV, dtype=dt, requires_grad=True)
        STR.conv(x.to(DEV, dt), dmap, W, n).backward(dy.to(DEV, dt))
        ref[dt] = {"dW": W.grad}
    return ref


def _narrow_chunk_pairs(nnz):
    """The chunk length of gmf_sparse_conv_narrow_wgrad (include/gmf_hip.h): max(64, ceil(nnz / 2048))."""
    return max(64, -(-nnz // 2048))


@pytest.mark.parametrize("cin,cout", [(1, 32), (3, 32), (8, 64), (1, 20)])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_narrow_wgrad_against_float64_and_generic(k, cin, cout):
    plan, cmap, dmap = _conv1_map("d3", k)
    M, K = plan.M, k ** 3
    g = torch.Generator().manual_seed(100 * k + 10 * cin + cout)
    x = torch.randn(M, cin, generator=g)
    dy = torch.randn(M, cout, generator=g)
    ref = _wgrad_reference(x, dy, dmap, K, M)
    dW = SP.sparse_conv_narrow_wgrad(plan, 0, 0, x.to(DEV), dy.to(DEV))
    generic = SP.sparse_conv_wgrad(plan, 0, 0, x.to(DEV), dy.to(DEV))
    assert tuple(dW.shape) == (K, cin, cout)
    rn = check_close({"dW": dW}, ref[torch.float64], ref[torch.float32], what=f"narrow k={k} {cin}x{cout}: ")
    rg = check_close({"dW": generic}, ref[torch.float64], ref[torch.float32], what=f"generic k={k} {cin}x{cout}: ")
    assert float((dW - generic).abs().max()) <= rn["dW"][1] + rg["dW"][1]
    assert torch.equal(dW, SP.sparse_conv_narrow_wgrad(plan, 0, 0, x.to(DEV), dy.to(DEV)))      # bitwise repeatable
    if k == 3:
        # the centre offset (a pair per row) spans several chunks
        assert -(-M // _narrow_chunk_pairs(len(cmap[1]))) >= 2


def test_narrow_wgrad_offsets_without_pairs_are_zero():
    plan, cmap, dmap = _conv1_map("d3_sparse", 7)
    M, K = plan.M, 343
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, 1, generator=g)
    dy = torch.randn(M, 32, generator=g)
    empty = sorted(set(range(K)) - set(np.unique(cmap[1][:, 0]).tolist()))
    assert len(empty) > K // 2, "this set is meant to leave most offsets without pairs"
    dW = SP.sparse_conv_narrow_wgrad(plan, 0, 0, x.to(DEV), dy.to(DEV))
    assert torch.all(dW[torch.as_tensor(empty, device=DEV)] == 0)
    ref = _wgrad_reference(x, dy, dmap, K, M)
    check_close({"dW": dW}, ref[torch.float64], ref[torch.float32], what="narrow sparse: ")
    assert torch.equal(dW, SP.sparse_conv_narrow_wgrad(plan, 0, 0, x.to(DEV), dy.to(DEV)))


# ---- y / (||y|| + 1e-8) ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,C", [(37, 32), (5, 1)])
def test_normalize_rows_eps(rows, C):
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, C, generator=g)
    x[rows // 2] = 0
    dy = torch.randn(rows, C, generator=g)
    ref = {}
    for dt in (torch.float64, torch.float32):
        xr = x.to(DEV, dt).requires_grad_(True)
        y = FTR.normalize_eps(xr)
        y.backward(dy.to(DEV, dt))
        ref[dt] = {"y": y, "dx": xr.grad}
    xd = x.to(DEV).requires_grad_(True)
    y = T.normalize_rows_eps(xd)
    y.backward(dy.to(DEV))
    check_close({"y": y, "dx": xd.grad}, ref[torch.float64], ref[torch.float32], what=f"rownorm [{rows}, {C}]: ")
    assert torch.all(y[rows // 2] == 0) and torch.all(xd.grad[rows // 2] == 0)


# ---- hardest-contrastive loss ----------------------------------------------------------------------------------------------

def _loss_case(name):
    if name == "margin":                       # the case whose margins tests/test_fcgf_train_host.py asserts
        return FTR.margin_case()
    case = FTR.margin_case(seed=3, N0=40, N1=37, C=16, K=24, P=None, H=None)     # every row a candidate, every pair sampled
    g = torch.Generator(device=DEV).manual_seed(0)
    sel0, sel1, pos_sel = fcgf.sample_hardest_contrastive(40, 37, case["pairs"].shape[0], num_pos=1024, num_hn_samples=256,
                                                          generator=g)
    assert sel0.is_cuda and sel0.dtype == torch.int64
    assert sorted(sel0.tolist()) == list(range(40)) and sorted(sel1.tolist()) == list(range(37))      # H > N: clipped to N
    assert sorted(pos_sel.tolist()) == list(range(case["pairs"].shape[0]))
    # all pairs in the sampler's order = pos_sel None over the permuted pairs; the candidates in the sampler's order
    case.update(sel0=sel0.cpu(), sel1=sel1.cpu(), pairs=case["pairs"][pos_sel.cpu()], pos_sel=None)
    return case


def _device_loss(case):
    F0 = case["F0"].to(DEV).requires_grad_(True)
    F1 = case["F1"].to(DEV).requires_grad_(True)
    pos_sel = None if case["pos_sel"] is None else case["pos_sel"].to(DEV)
    pos, neg, aux = fcgf.hardest_contrastive_loss(F0, F1, case["pairs"].to(DEV), case["sel0"].to(DEV), case["sel1"].to(DEV),
                                                  pos_sel, case["pos_thresh"], case["neg_thresh"])
    (pos + 0.5 * neg).backward()                # distinct upstream gradients for the two losses
    return pos, neg, aux, F0.grad, F1.grad


@pytest.mark.parametrize("name", ["margin", "all_rows_c16"])
def test_hardest_contrastive_loss_against_float64(name):
    case = _loss_case(name)
    pos, neg, aux, dF0, dF1 = _device_loss(case)
    gmf_amd.check_status()
    args = [case[k] if case[k] is None else case[k].to(DEV) for k in ("pairs", "sel0", "sel1", "pos_sel")]
    ref = {}
    for dt in (torch.float64, torch.float32):
        F0 = case["F0"].to(DEV, dt).requires_grad_(True)
        F1 = case["F1"].to(DEV, dt).requires_grad_(True)
        kw = {}
        if dt == torch.float32:                 # the float32 floor on the float64 selection and masks
            a64 = ref[torch.float64]["aux"]
            kw = dict(h01=a64["h01"], h10=a64["h10"], masks=(a64["pos_arg"] > 0, a64["neg0_arg"] > 0, a64["neg1_arg"] > 0))
        p, n, a = FTR.hardest_contrastive_loss(F0, F1, *args, case["pos_thresh"], case["neg_thresh"], **kw)
        (p + 0.5 * n).backward()
        ref[dt] = {"pos": p, "neg": n, "dF0": F0.grad, "dF1": F1.grad, "D01": a["D01"], "D10": a["D10"], "aux": a}
    a64 = ref[torch.float64]["aux"]
    # the margins (asserted on the host for "margin", here for the sampler-ordered case): selection and masks are exact
    assert float((a64["D01_second"] - a64["D01"]).min()) >= 1e-4 and float((a64["D10_second"] - a64["D10"]).min()) >= 1e-4
    assert min(float(a64[k].abs().min()) for k in ("pos_arg", "neg0_arg", "neg1_arg")) >= 1e-4
    for k in ("h01", "h10", "keep0", "keep1"):
        assert torch.equal(aux[k], a64[k]), k
    assert aux["keep0"].dtype == torch.bool and not aux["D01"].requires_grad
    names = ("pos", "neg", "dF0", "dF1", "D01", "D10")
    got = {"pos": pos, "neg": neg, "dF0": dF0, "dF1": dF1, "D01": aux["D01"], "D10": aux["D10"]}
    check_close(got, {k: ref[torch.float64][k] for k in names}, {k: ref[torch.float32][k] for k in names}, what=f"loss {name}: ")
    # rows of F0 / F1 shared by several pairs and several hardest negatives: the same bits again
    _, _, _, dF0b, dF1b = _device_loss(case)
    assert torch.equal(dF0, dF0b) and torch.equal(dF1, dF1b)
    shared = torch.bincount(aux["h01"]) if name != "margin" else torch.bincount(case["pairs"][case["pos_sel"], 0])
    assert int((shared > 1).sum()) > 0


def test_hardest_contrastive_loss_no_kept_row_on_one_side():
    """sel1 holds one row, and every sampled row of F0 is paired with it: side 0 keeps nothing and gives 0, side 1 works."""
    g = torch.Generator().manual_seed(4)
    F0h, F1h = torch.randn(12, 8, generator=g), torch.randn(9, 8, generator=g)
    own = torch.stack([torch.arange(6), torch.arange(1, 7)], 1)
    pairs = torch.cat([own, torch.stack([torch.arange(6), torch.zeros(6, dtype=torch.int64)], 1)])
    pos_sel, sel0, sel1 = torch.arange(6), torch.arange(6, 12), torch.zeros(1, dtype=torch.int64)
    out = {}
    for dt in (None, torch.float64, torch.float32):
        F0 = F0h.to(DEV, dt or torch.float32).requires_grad_(True)
        F1 = F1h.to(DEV, dt or torch.float32).requires_grad_(True)
        fn = fcgf.hardest_contrastive_loss if dt is None else FTR.hardest_contrastive_loss
        pos, neg, aux = fn(F0, F1, pairs.to(DEV), sel0.to(DEV), sel1.to(DEV), pos_sel.to(DEV), 0.5, 6.0)
        (pos + neg).backward()
        out[dt] = ({"pos": pos, "neg": neg, "dF0": F0.grad, "dF1": F1.grad}, aux)
    got, aux = out[None]
    assert not aux["keep0"].any() and aux["keep1"].all()
    assert torch.isfinite(got["dF0"]).all() and torch.isfinite(got["dF1"]).all() and float(got["neg"].detach()) > 0
    check_close(got, out[torch.float64][0], out[torch.float32][0], what="loss one side empty: ")
    # nothing kept on either side: exactly 0, finite gradients
    F0 = F0h.to(DEV).requires_grad_(True)
    F1 = F1h.to(DEV).requires_grad_(True)
    every =torch.stack([torch.arange(6).repeat_interleave(7), torch.arange(7).repeat(6)], 1).to(DEV)
    pos, neg, aux = fcgf.hardest_contrastive_loss(F0, F1, every, torch.arange(6, device=DEV), torch.arange(7, device=DEV), None, 0.5,
                                                  6.0)
    neg.backward()
    assert not aux["keep0"].any() and not aux["keep1"].any() and float(neg.detach()) == 0
    assert torch.all(F0.grad == 0) and torch.all(F1.grad == 0)


def test_hardest_contrastive_loss_flags_a_bad_index():
    gmf_amd.check_status()
    F0, F1 = torch.randn(6, 8, device=DEV), torch.randn(5, 8, device=DEV)
    pairs = torch.tensor([[0, 1], [2, 3]], device=DEV)
    fcgf.hardest_contrastive_loss(F0, F1, pairs, torch.tensor([0, 6], device=DEV), torch.tensor([1], device=DEV))
    with pytest.raises(RuntimeError, match="row index outside"):
        gmf_amd.check_status()
    gmf_amd.check_status()


# ---- the whole network -----------------------------------------------------------------------------------------------------

def _recording_relu_masks(monkeypatch):
    """test_gpu_sparse_train._recording_relu_masks extended to the head: records, in forward order, the output mask (> 0) of the
    14 BatchNorm + ReLU of fcgf_train and then of the ReLU after conv1_tr.  The gradients are compared on the side of each ReLU
    kink that the device's forward took; the outputs and running statistics are compared without it."""
    masks = []
    orig_bn, orig_conv = T.batchnorm_masked, SP.sparse_conv_train

    def rec_bn(x, bn, plan, level, residual=None, relu=False):
        y = orig_bn(x, bn, plan, level, residual=residual, relu=relu)
        if relu:
            masks.append(y.detach() > 0)
        return y

    def rec_conv(plan, map_index, out_level, xa, W, xb=None, bias=None, relu=False):
        y = orig_conv(plan, map_index, out_level, xa, W, xb=xb, bias=bias, relu=relu)
        if relu:
            masks.append(y.detach() > 0)
        return y
    monkeypatch.setattr(T, "batchnorm_masked", rec_bn)
    monkeypatch.setattr(SP, "sparse_conv_train", rec_conv)
    return masks


def _reference_step(sd, lm, feats, normalize, dt, R, relu_masks=None):
    params = {k: v.to(DEV, dt).requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    buffers = {k: v.to(DEV, dt) for k, v in sd.items() if "running" in k}
    out, run = FTR.fcgf_train_forward(params, buffers, lm, feats.to(DEV, dt), normalize, relu_masks=relu_masks)
    (out * R.to(out)).sum().backward()
    return out, {k: p.grad for k, p in params.items()}, run


def _device_step(model, sd, coords, feats, R, monkeypatch, narrow):
    model.load_state_dict(sd)
    model.train()
    model.zero_grad(set_to_none=True)
    model.narrow_conv1 = narrow
    with monkeypatch.context() as mp:
        masks = _recording_relu_masks(mp)
        out = T.fcgf_train(model, coords, feats.to(DEV))
        (out * R.to(DEV)).sum().backward()
    assert len(masks) == 15
    return out, {k: p.grad for k, p in model.named_parameters()}, dict(model.named_buffers()), masks


@pytest.mark.parametrize("out_channels,k1,normalize", [(32, 7, True), (16, 5, False)])
def test_fcgf_train_against_float64(out_channels, k1, normalize, monkeypatch):
    rows = _set("d3_two")
    coords = torch.as_tensor(rows).to(DEV).int()
    M = len(rows)
    feats = torch.ones(M, 1)
    model = fcgf.ResUNetBN2C(1, out_channels, conv1_kernel_size=k1, normalize_feature=normalize, D=3)
    sd = FR.conditioned_state_dict(model, rows, feats)
    model = model.to(DEV)
    R = torch.randn(M, out_channels, generator=torch.Generator().manual_seed(9))
    lm = STR.device_levels_and_maps(rows, DEV, k1)
    tag = f"fcgf k1={k1} normalize={normalize}: "
    plain = {dt: _reference_step(sd, lm, feats, normalize, dt, R) for dt in (torch.float64, torch.float32)}
    for narrow in ((True, False) if normalize else (True,)):
        out, grads, bufs, masks = _device_step(model, sd, coords, feats, R, monkeypatch, narrow)
        assert len(grads) == 23 + 1 + 42 and all(g is not None for g in grads.values())
        ref = {dt: _reference_step(sd, lm, feats, normalize, dt, R, relu_masks=masks) for dt in (torch.float64, torch.float32)}
        check_close(grads, ref[torch.float64][1], ref[torch.float32][1], what=tag + f"narrow={narrow} ")
        # outputs and running statistics: the plain restatement
        check_close({"out": out}, {"out": plain[torch.float64][0]}, {"out": plain[torch.float32][0]}, what=tag)
        run64, run32 = plain[torch.float64][2], plain[torch.float32][2]
        assert len(run64) == 42
        check_close({k: bufs[k] for k in run64}, run64, run32, what=tag + "running ")
        assert all(int(v) == 1 for k, v in bufs.items() if k.endswith("num_batches_tracked"))
    if normalize:
        assert torch.allclose(out.norm(dim=1), torch.ones(M, device=DEV), atol=1e-5)


# ---- one optimisation run, end to end ----------------------------------------------------------------------------------------

def test_fcgf_training_run_lowers_the_loss():
    """The INTEGRATION.md step on the 3DMatch demo pair at 5 cm: voxel_select, matching_indices_batched (the clouds share a frame:
    the identity), fcgf_train on both clouds as one batch, the loss, Adam."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
    v = 0.05
    xyz = []
    for c in (z["cloud0"], z["cloud1"]):
        p = torch.as_tensor(c.astype(np.float32)).to(DEV)
        xyz.append(p[gmf_amd.voxel_select(p, v)])
    N0, N1 = len(xyz[0]), len(xyz[1])
    coords = torch.cat([torch.cat([torch.full((len(x), 1), b, dtype=torch.int32, device=DEV),           # fp64, as the voxel selection
                                   torch.floor(x.double() / v).to(torch.int32)], 1) for b, x in enumerate(xyz)])
    feats = torch.ones(N0 + N1, 1, device=DEV)
    eye = torch.eye(4, dtype=torch.float64, device=DEV)[None]
    pairs, _ = gmf_amd.matching_indices_batched(xyz[0], [0, N0], xyz[1], [0, N1], eye, 1.5 * v)
    assert pairs.shape[0] >= 256
    torch.manual_seed(0)
    model = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=7, normalize_feature=True, D=3).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    gen = torch.Generator(device=DEV).manual_seed(1)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        out = T.fcgf_train(model, coords, feats)
        sel0, sel1, pos_sel = fcgf.sample_hardest_contrastive(N0, N1, pairs.shape[0], generator=gen)
        pos, neg, _ = fcgf.hardest_contrastive_loss(out[:N0], out[N0:], pairs, sel0, sel1, pos_sel)
        loss = pos + neg
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    gmf_amd.check_status()
    losses = torch.stack(losses).cpu()
    assert torch.isfinite(losses).all(), losses
    assert float(losses[-1]) < float(losses[0]), losses
    # the eval forward follows the trained weights (the packed-weight cache is rebuilt)
    model.eval()
    y = model(coords, feats)
    assert torch.isfinite(y).all() and torch.allclose(y.norm(dim=1), torch.ones(N0 + N1, device=DEV), atol=1e-4)
