"""GPU tests of the sparse network's training path - the sparse-convolution backward, BatchNorm over a level's device-counted
rows, gmf_amd.train.resunet_train and gmf_amd.dgr.inlier_training_loss - against the float64 restatement of
tests/sparse_train_reference.py, with the bound of test_train_gradients.check_close (float64 reference, float32 floor x 4)."""
import os

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import sparse as SP
from gmf_amd import train as T
from gmf_amd.dgr import inlier_training_loss

import sparse_reference as SR
import sparse_train_reference as STR
from test_train_gradients import check_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_MAPS = SP._NET_MAPS


def _random_coords(M, D, span, batches, seed):
    rng = np.random.default_rng(seed)
    rows = set()
    while len(rows) < M:
        rows.add((int(rng.choice(batches)),) + tuple(int(v) for v in rng.integers(-span, span, D)))
    out = np.array(sorted(rows), dtype=np.int64)
    return out[rng.permutation(M)]


_SETS = {}


def _set(name):
    if name not in _SETS:
        _SETS[name] = {"d3": lambda: _random_coords(700, 3, 7, [0, 1, 2], 11),
                       "d6": lambda: _random_coords(900, 6, 3, [0, 1], 12),
                       "d6_sparse": lambda: _random_coords(120, 6, 4, [0, 1], 13)}[name]()
    return _SETS[name]


_DEMO = {}


def _demo():
    """DGR's 6-D correspondences of the 3DMatch demo fragments (as tests/test_gpu_sparse.py builds them), with the voxelised
    points and the pairs."""
    if "c" not in _DEMO:
        z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
        v = 0.05
        xyz, feat = [], []
        for c in (z["cloud0"], z["cloud1"]):
            x, f = gmf_amd.fpfh_descriptors(torch.as_tensor(c.astype(np.float32)).to(DEV), v, voxelize="select")
            xyz.append(x)
            feat.append(f)
        coords = [torch.cat([torch.zeros((len(x), 1), dtype=torch.int32, device=DEV), torch.floor(x / v).int()], 1) for x in xyz]
        idx1 = gmf_amd.find_knn_gpu(feat[0], feat[1], nn_max_n=-1, knn=1).reshape(-1)
        idx0 = torch.arange(len(idx1), device=DEV)
        _DEMO.update(c=gmf_amd.inlier_coordinates(coords[0], coords[1], idx0, idx1), xyz=xyz,
                     pairs=torch.stack([idx0, idx1.long()], 1))
    return _DEMO


# ---- one convolution's backward --------------------------------------------------------------------------------------------
# (name, set, map index or None, ca, cb, cout): same-level, down, transposed, two-source, identity, conv1 (cin 1, K = 729) and a
# kernel of more than 16 MiB (729 x 128 x 128 x 4 B); a sparse 6-D set leaves most offsets without pairs
FORMS = [("same_d3", "d3", 0, 32, 0, 32), ("down_d3", "d3", 4, 32, 0, 64), ("tr_two_d3", "d3", 7, 64, 32, 64),
         ("ident_two_d3", "d3", None, 64, 32, 64), ("same_d6", "d6", 1, 64, 0, 64), ("down_d6", "d6", 5, 64, 0, 128),
         ("tr_d6", "d6", 9, 256, 0, 128), ("tr_two_d6", "d6", 8, 128, 128, 64), ("conv1_d6", "d6", 0, 1, 0, 32),
         ("big_d6", "d6", 3, 128, 0, 128), ("ident_d6", "d6", None, 64, 0, 1), ("empty_offsets_d6", "d6_sparse", 0, 32, 0, 32),
         ("down23_demo", "demo", 6, 128, 0, 256), ("same2_demo", "demo", 2, 128, 0, 128), ("down12_demo", "demo", 5, 64, 0, 128),
         ("tr_two_demo", "demo", 8, 128, 128, 64)]


def _layer_case(name, set_name, m, ca, cb, cout):
    rows = _demo()["c"].cpu().numpy() if set_name == "demo" else _set(set_name)
    D = rows.shape[1] - 1
    plan = SP.SparsePlan(torch.as_tensor(rows).to(DEV).int(), 4, NET_MAPS)
    lv = SR.build_levels(rows, 4)
    k, o, i = (1, 0, 0) if m is None else NET_MAPS[m]
    n_in, n_out = len(lv[i]), len(lv[o])
    assert plan.counts.tolist() == [len(r) for r in lv]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    K = k ** D
    M = plan.M
    xa = torch.randn(M, ca, generator=g)
    xb = torch.randn(M, cb, generator=g) if cb else None
    W = torch.randn(K, ca + cb, cout, generator=g) / (K * (ca + cb)) ** 0.5
    dy = torch.randn(M, cout, generator=g)
    for t in (xa, xb, dy):                     # rows past the level counts hold garbage the kernels must not read
        if t is not None:
            t[n_in if t is not dy else n_out:] = 1e30
    cmap = None if m is None else SR.map_between(lv, k, o, i)
    return plan, lv, (k, o, i), (n_in, n_out, K), xa, xb, W, dy, cmap


def _hip_backward(plan, m, o, xa, xb, W, dy):
    xa_d = xa.to(DEV).requires_grad_(True)
    xb_d = None if xb is None else xb.to(DEV).requires_grad_(True)
    W_d = W.to(DEV).requires_grad_(True)
    y = SP.sparse_conv_train(plan, m, o, xa_d, W_d, xb=xb_d)
    y.backward(dy.to(DEV))
    return xa_d.grad, None if xb is None else xb_d.grad, W_d.grad


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_sparse_conv_backward_one_layer(form):
    name, set_name, m, ca, cb, cout = form
    plan, lv, (k, o, i), (n_in, n_out, K), xa, xb, W, dy, cmap = _layer_case(*form)
    dmap = None if cmap is None else STR.DeviceMap(cmap, n_out, DEV)
    ref = {}
    for dt in (torch.float64, torch.float32):
        x = torch.cat([xa[:n_in]] + ([xb[:n_in]] if xb is not None else []), 1).to(DEV, dt).requires_grad_(True)
        Wr = W.to(DEV, dt).requires_grad_(True)
        y = STR.conv(x, dmap, Wr, n_out)
        y.backward(dy[:n_out].to(DEV, dt))
        ref[dt] = {"dxa": x.grad[:, :ca], "dW": Wr.grad}
        if xb is not None:
            ref[dt]["dxb"] = x.grad[:, ca:]
    dxa, dxb, dW = _hip_backward(plan, m, o, xa, xb, W, dy)
    got = {"dxa": dxa[:n_in], "dW": dW}
    if xb is not None:
        got["dxb"] = dxb[:n_in]
    check_close(got, ref[torch.float64], ref[torch.float32], what=f"{name}: ")
    # rows past the input level's count are exactly 0
    assert torch.all(dxa[n_in:] == 0) and (dxb is None or torch.all(dxb[n_in:] == 0))
    # offsets without pairs: exactly 0
    if cmap is not None:
        empty = sorted(set(range(K)) - set(np.unique(cmap[1][:, 0]).tolist()))
        if empty:
            assert torch.all(dW[torch.as_tensor(empty, device=DEV)] == 0)
        if name == "empty_offsets_d6":
            assert empty, "this form is meant to cover offsets without pairs"
    # bitwise repeatable
    dxa2, dxb2, dW2 = _hip_backward(plan, m, o, xa, xb, W, dy)
    assert torch.equal(dW, dW2) and torch.equal(dxa, dxa2) and (dxb is None or torch.equal(dxb, dxb2))


# ---- BatchNorm over a level's device-counted rows --------------------------------------------------------------------------

@pytest.mark.parametrize("set_name,lvl,C", [("d3", 2, 48), ("demo", 1, 64), ("demo", 2, 128), ("demo", 3, 256)])
@pytest.mark.parametrize("variant", ["bn", "relu", "residual"])
def test_batchnorm_masked_against_batchnorm1d(variant, set_name, lvl, C):
    rows = _demo()["c"].cpu().numpy() if set_name == "demo" else _set(set_name)
    plan = SP.SparsePlan(torch.as_tensor(rows).to(DEV).int(), 4, NET_MAPS)
    n = int(plan.counts[lvl])
    M = plan.M
    assert 2 <= n < M
    g = torch.Generator().manual_seed(5)
    x = 3 + 2 * torch.randn(M, C, generator=g)
    res = torch.randn(M, C, generator=g) if variant == "residual" else None
    dy = torch.randn(M, C, generator=g)
    x[n:] = 1e30
    bn = torch.nn.BatchNorm1d(C).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * torch.randn(C, generator=g))
        bn.bias.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(1 + torch.rand(C, generator=g))
    outs = {}
    for dt in (torch.float64, torch.float32):
        b = torch.nn.BatchNorm1d(C).to(DEV, dt).train()
        b.load_state_dict({k: v.to(dt) if v.is_floating_point() else v for k, v in bn.state_dict().items()})
        xr = x[:n].to(DEV, dt).requires_grad_(True)
        rr = None if res is None else res[:n].to(DEV, dt).requires_grad_(True)
        y = b(xr)
        if rr is not None:
            y = y + rr
        if variant != "bn":
            y = torch.relu(y)
        y.backward(dy[:n].to(DEV, dt))
        outs[dt] = {"y": y, "dx": xr.grad, "dgamma": b.weight.grad, "dbeta": b.bias.grad, "running_mean": b.running_mean,
                    "running_var": b.running_var}
        if rr is not None:
            outs[dt]["dres"] = rr.grad
    xd = x.to(DEV).requires_grad_(True)
    rd = None if res is None else res.to(DEV).requires_grad_(True)
    y = T.batchnorm_masked(xd, bn, plan, lvl, residual=rd, relu=variant != "bn")
    y.backward(dy.to(DEV))
    got = {"y": y[:n], "dx": xd.grad[:n], "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
           "running_var": bn.running_var}
    if rd is not None:
        got["dres"] = rd.grad[:n]
        assert torch.all(rd.grad[n:] == 0)
    check_close(got, outs[torch.float64], outs[torch.float32], what=f"bn {variant}: ")
    assert torch.all(y[n:] == 0) and torch.all(xd.grad[n:] == 0)
    assert int(bn.num_batches_tracked) == 1


def test_batchnorm_masked_single_row_sets_status():
    gmf_amd.check_status()
    plan = SP.SparsePlan(torch.zeros((1, 4), dtype=torch.int32, device=DEV), 1, [])
    bn = torch.nn.BatchNorm1d(8).to(DEV).train()
    before = bn.running_mean.clone()
    T.batchnorm_masked(torch.randn(1, 8, device=DEV), bn, plan, 0)
    with pytest.raises(RuntimeError, match="fewer than 2"):
        gmf_amd.check_status()
    assert torch.equal(bn.running_mean, before)
    gmf_amd.check_status()


# ---- the whole network ---------------------------------------------------------------------------------------------------

def _trainable(model):
    return [n for n, _ in model.named_parameters() if not n.startswith("img_encoder.")]


def _network_case(set_name, pe, seed=0):
    if set_name == "demo":
        coords = _demo()["c"]
    else:
        coords = torch.as_tensor(_set("d6")).to(DEV).int()
    M = coords.shape[0]
    g = torch.Generator().manual_seed(seed)
    feats = torch.ones(M, 1)
    p_tok = torch.randn(1, 40, 128, generator=g)
    q_tok = torch.randn(1, 40, 128, generator=g)
    model = gmf_amd.ResUNetBN2C(in_channels=1, out_channels=1, D=6, pe=pe)
    sd = SR.conditioned_state_dict(model, coords.cpu().numpy(), feats, p_tok, q_tok, seed=seed)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    return model, sd, coords, feats, p_tok, q_tok


def _recording_relu_masks(monkeypatch):
    """Records, in forward order, the output mask (> 0) of every BatchNorm + ReLU of resunet_train.  The gradients are compared on
    the side of each ReLU kink that the device's forward took (a pre-activation within float32 rounding of 0 flips the
    derivative; on the 3DMatch demo pair a few of ~10^6 such activations do, see sparse_train_reference.resunet_train_forward);
    the outputs and running statistics are compared without it."""
    masks = []
    orig = T.batchnorm_masked

    def rec(x, bn, plan, level, residual=None, relu=False):
        y = orig(x, bn, plan, level, residual=residual, relu=relu)
        if relu:
            masks.append((y.detach() > 0))
        return y
    monkeypatch.setattr(T, "batchnorm_masked", rec)
    return masks


def _reference_step(sd, names, lm, feats, p_tok, q_tok, pe, dt, loss_fn, relu_masks=None):
    params = {k: (v.to(DEV, dt).requires_grad_(k in names)) for k, v in sd.items()
              if v.is_floating_point() and "running" not in k}
    buffers = {k: v.to(DEV, dt) for k, v in sd.items() if "running" in k}
    pt = p_tok.to(DEV, dt).requires_grad_(True)
    qt = q_tok.to(DEV, dt).requires_grad_(True)
    out, run = STR.resunet_train_forward(params, buffers, lm, feats.to(DEV, dt), pt, qt, pe, relu_masks=relu_masks)
    loss = loss_fn(out)
    loss.backward()
    grads = {k: params[k].grad for k in names}
    grads.update(dp_tokens=pt.grad, dq_tokens=qt.grad)
    return out, grads, run, loss


@pytest.mark.parametrize("set_name,pe", [("demo", False), ("demo", True), ("ragged", False), ("ragged", True)])
def test_resunet_train_against_float64(set_name, pe, monkeypatch):
    model, sd, coords, feats, p_tok, q_tok = _network_case(set_name, pe)
    names = _trainable(model)
    M = coords.shape[0]
    R = torch.randn(M, 1, generator=torch.Generator().manual_seed(9))
    lm = STR.device_levels_and_maps(coords.cpu().numpy(), DEV)
    masks = _recording_relu_masks(monkeypatch)
    pt = p_tok.to(DEV).requires_grad_(True)
    qt = q_tok.to(DEV).requires_grad_(True)
    out = T.resunet_train(model, coords, feats.to(DEV), p_tokens=pt, q_tokens=qt)
    (out * R.to(DEV)).sum().backward()
    assert len(masks) == 14
    loss = lambda y: (y * R.to(y)).sum()   # noqa: E731
    plain = {dt: _reference_step(sd, names, lm, feats, p_tok, q_tok, pe, dt, loss) for dt in (torch.float64, torch.float32)}
    ref = {dt: _reference_step(sd, names, lm, feats, p_tok, q_tok, pe, dt, loss, relu_masks=masks)
           for dt in (torch.float64, torch.float32)}
    for dt in ref:                       # outputs and running statistics: the plain restatement
        ref[dt] = (plain[dt][0], ref[dt][1], plain[dt][2], ref[dt][3])
    params = dict(model.named_parameters())
    got = {k: params[k].grad for k in names}
    got.update(dp_tokens=pt.grad, dq_tokens=qt.grad)
    tag = f"{set_name} pe={pe}: "
    check_close({"out": out}, {"out": ref[torch.float64][0]}, {"out": ref[torch.float32][0]}, what=tag)
    check_close(got, ref[torch.float64][1], ref[torch.float32][1], what=tag)
    bufs = dict(model.named_buffers())
    run64, run32 = ref[torch.float64][2], ref[torch.float32][2]
    assert len(run64) == 42
    check_close({k: bufs[k] for k in run64}, run64, run32, what=tag + "running ")


def test_resunet_train_image_path_equals_token_path():
    rows = torch.as_tensor(_random_coords(500, 3, 6, [0, 1], 21)).to(DEV).int()
    g = torch.Generator().manual_seed(3)
    model = gmf_amd.ResUNetBN2C(in_channels=1, out_channels=1, D=3).to(DEV).train()
    p_img = torch.randn(1, 3, 64, 80, generator=g).to(DEV)
    q_img = torch.randn(1, 3, 64, 80, generator=g).to(DEV)
    feats = torch.ones(rows.shape[0], 1, device=DEV)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    out_img = T.resunet_train(model, rows, feats, p_image=p_img, q_image=q_img)
    out_img.sum().backward()
    enc = [p.grad for n, p in model.named_parameters() if n.startswith("img_encoder.") and p.requires_grad]
    assert enc and all(gr is not None and torch.isfinite(gr).all() for gr in enc)
    assert any(float(gr.abs().max()) > 0 for gr in enc)
    model.load_state_dict(state)
    model.train()
    pt = model.img_encoder(p_img).flatten(2).permute(0, 2, 1).contiguous()
    qt = model.img_encoder(q_img).flatten(2).permute(0, 2, 1).contiguous()
    model.load_state_dict(state)                 # the token pass above moved the encoder's running statistics
    model.train()
    out_tok = T.resunet_train(model, rows, feats, p_tokens=pt, q_tokens=qt)
    assert torch.allclose(out_img, out_tok, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("balanced", [False, True])
def test_dgr_training_step_against_float64(balanced, monkeypatch):
    model, sd, coords, feats, p_tok, q_tok = _network_case("demo", True, seed=1)
    masks = _recording_relu_masks(monkeypatch)
    d = _demo()
    names = _trainable(model)
    M = coords.shape[0]
    is_correct = (torch.rand(M, generator=torch.Generator().manual_seed(4)) < 0.3).float()
    ang = 0.3
    T_gt = torch.tensor([[np.cos(ang), -np.sin(ang), 0, 0.2], [np.sin(ang), np.cos(ang), 0, -0.1], [0, 0, 1, 0.05], [0, 0, 0, 1]],
                        dtype=torch.float64)[None]
    xyz0s, xyz1s, pairs = [d["xyz"][0]], [d["xyz"][1]], [d["pairs"]]
    lm = STR.device_levels_and_maps(coords.cpu().numpy(), DEV)

    def ref_loss(y):
        return STR.inlier_training_loss(y, [x.to(y) for x in xyz0s], [x.to(y) for x in xyz1s], pairs, is_correct.to(DEV),
                                        T_gt.to(DEV), use_balanced_loss=balanced)[0]
    out = T.resunet_train(model, coords, feats.to(DEV), p_tokens=p_tok.to(DEV), q_tokens=q_tok.to(DEV))
    loss, stats = inlier_training_loss(out, xyz0s, xyz1s, pairs, is_correct.to(DEV), T_gt.to(DEV), use_balanced_loss=balanced)
    ref = {dt: _reference_step(sd, names, lm, feats, p_tok, q_tok, True, dt, ref_loss, relu_masks=masks)
           for dt in (torch.float64, torch.float32)}
    assert bool(stats["valid"].all())
    loss.backward()
    params = dict(model.named_parameters())
    check_close({"loss": loss}, {"loss": ref[torch.float64][3]}, {"loss": ref[torch.float32][3]}, what="dgr loss: ")
    got = {k: params[k].grad for k in names}
    ref64 = {k: v for k, v in ref[torch.float64][1].items() if k in names}
    ref32 = {k: v for k, v in ref[torch.float32][1].items() if k in names}
    check_close(got, ref64, ref32, what="dgr step: ")
    # an optimizer step, then the eval forward follows the updated weights (the packed-weight cache is rebuilt)
    torch.optim.SGD([p for n, p in model.named_parameters() if n in names], lr=1e-3).step()
    model.eval()
    p_t, q_t = p_tok.to(DEV), q_tok.to(DEV)
    y = model(coords, feats.to(DEV), p_tokens=p_t, q_tokens=q_t)
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    lmh = SR.levels_and_maps(coords.cpu().numpy())
    y64, _ = SR.resunet_forward(state, coords.cpu().numpy(), feats, p_tok, q_tok, True, levels_maps=lmh)
    y32, _ = SR.resunet_forward(state, coords.cpu().numpy(), feats, p_tok, q_tok, True, dtype=torch.float32, levels_maps=lmh)
    check_close({"eval": y}, {"eval": y64}, {"eval": y32}, what="after SGD: ")
