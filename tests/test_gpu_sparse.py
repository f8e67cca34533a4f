"""GPU tests of the sparse coordinate engine, the sparse convolution and ResUNetBN2C (gmf_amd/sparse.py) against the float64
restatement of tests/sparse_reference.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gmf_amd
from gmf_amd import sparse as SP
from gmf_amd import synthetic

import sparse_reference as R
from test_sparse_forms_host import random_coords as _random_coords      # shared with tests/test_gpu_sparse_forms.py

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_MAPS = SP._NET_MAPS
EPS32 = float(np.finfo(np.float32).eps)


def _g(x):
    return torch.as_tensor(x).to(DEV)


_SETS = {}


def _set(name):
    if name not in _SETS:
        _SETS[name] = {"d3": lambda: _random_coords(700, 3, 7, [0, 1, 2], 11),
                       "d6": lambda: _random_coords(900, 6, 3, [0, 1], 12)}[name]()
    return _SETS[name]


_DEMO = {}


def _demo_coords():
    """DGR's 6-D correspondences of the 3DMatch demo fragments: voxel_select at 5 cm, FPFH, find_knn_gpu, inlier_coordinates."""
    if "c" not in _DEMO:
        z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
        v = 0.05
        xyz, feat = [], []
        for c in (z["cloud0"], z["cloud1"]):
            x, f = gmf_amd.fpfh_descriptors(_g(c.astype(np.float32)), v, voxelize="select")
            xyz.append(x)
            feat.append(f)
        coords = [torch.cat([torch.zeros((len(x), 1), dtype=torch.int32, device=DEV), torch.floor(x / v).int()], 1) for x in xyz]
        idx1 = gmf_amd.find_knn_gpu(feat[0], feat[1], nn_max_n=-1, knn=1).reshape(-1)
        idx0 = torch.arange(len(idx1), device=DEV)
        _DEMO["c"] = gmf_amd.inlier_coordinates(coords[0], coords[1], idx0, idx1)
    return _DEMO["c"]


def _plan(rows, maps=NET_MAPS):
    return gmf_amd.SparsePlan(_g(rows).int(), 4, maps)


# ---- coordinate and kernel maps --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["d3", "d6"])
def test_levels_and_maps_equal_restatement(name):
    rows = _set(name)
    host = _plan(rows).to_host()
    lv = R.build_levels(rows, 4)
    assert host["counts"] == [len(r) for r in lv]
    for l in range(4):
        assert np.array_equal(host["levels"][l].numpy(), lv[l]), l
    for m, (k, o, i) in enumerate(NET_MAPS):
        rp, pairs = R.map_between(lv, k, o, i)
        assert np.array_equal(host["maps"][m][0].numpy(), rp), (m, k, o, i)
        assert np.array_equal(host["maps"][m][1].numpy(), pairs), (m, k, o, i)


def test_demo_correspondence_maps_equal_restatement():
    rows = _demo_coords().cpu().numpy()
    host = _plan(rows).to_host()
    lv = R.build_levels(rows, 4)
    assert host["counts"] == [len(r) for r in lv]
    for m, (k, o, i) in enumerate(NET_MAPS):
        rp, pairs = R.map_between(lv, k, o, i)
        assert np.array_equal(host["maps"][m][0].numpy(), rp) and np.array_equal(host["maps"][m][1].numpy(), pairs), m


def test_duplicate_row_raises_at_check_status():
    gmf_amd.check_status()
    rows = _set("d3").copy()
    rows[5] = rows[17]
    _plan(rows, [(3, 0, 0)])
    with pytest.raises(RuntimeError, match="duplicate"):
        gmf_amd.check_status()
    gmf_amd.check_status()                 # the bit was cleared


# ---- every convolution form against fp64 -------------------------------------------------------------------------------------
# (name, map index or None, out level, ca, cb, cout, epilogue): every (Cin, Cout) of ResUNetBN2C
FORMS = [("conv1", 0, 0, 1, 0, 32, "bn"), ("s0", 0, 0, 32, 0, 32, "res"), ("down01", 4, 1, 32, 0, 64, "bn"),
         ("s1", 1, 1, 64, 0, 64, "res"), ("down12", 5, 2, 64, 0, 128, "bn"), ("s2", 2, 2, 128, 0, 128, "res"),
         ("down23", 6, 3, 128, 0, 256, "bn"), ("s3", 3, 3, 256, 0, 256, "res"), ("tr32", 9, 2, 256, 0, 128, "bn"),
         ("tr21", 8, 1, 128, 128, 64, "bn"), ("tr10", 7, 0, 64, 64, 64, "bn"), ("k1cat", None, 0, 64, 32, 64, "relu"),
         ("final", None, 0, 64, 0, 1, "bias")]
_PLANS = {}


def _d6_plan():
    if "d6" not in _PLANS:
        rows = _set("d6")
        lv = R.build_levels(rows, 4)
        _PLANS["d6"] = (_plan(rows), lv, {m: R.map_between(lv, *NET_MAPS[m]) for m in range(len(NET_MAPS))})
    return _PLANS["d6"]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_conv_form_against_fp64(form):
    name, m, lvl, ca, cb, cout, epi = form
    plan, lv, maps = _d6_plan()
    in_lvl = lvl if m is None else NET_MAPS[m][2]
    K = 1 if m is None else plan.K[m]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    M = plan.M
    xa, xb = torch.randn(M, ca, generator=g), (torch.randn(M, cb, generator=g) if cb else None)
    W = torch.randn(K, ca + cb, cout, generator=g) / (ca + cb) ** 0.5
    scale = 1 + 0.2 * torch.randn(cout, generator=g) if epi in ("bn", "res") else None
    shift = 0.2 * torch.randn(cout, generator=g) if epi in ("bn", "res", "bias") else None
    res = torch.randn(M, cout, generator=g) if epi == "res" else None
    relu = epi in ("res", "relu")
    nsplit = SP.layer_nsplit(K, ca + cb, cout)
    y = SP.sparse_conv(plan, m, lvl, _g(xa), _g(W), xb=None if xb is None else _g(xb), scale=None if scale is None else _g(scale),
                       shift=None if shift is None else _g(shift), residual=None if res is None else _g(res), relu=relu,
                       nsplit=nsplit).cpu()
    n = len(lv[lvl])
    x_in = xa if xb is None else torch.cat([xa, xb], 1)
    x_in = x_in[:len(lv[in_lvl])]

    def restated(dtype):
        v = R.conv(x_in, None if m is None else maps[m], W, n, dtype)
        if scale is not None:
            v = v * scale.to(dtype)
        if shift is not None:
            v = v + shift.to(dtype)
        if res is not None:
            v = v + res[:n].to(dtype)
        return torch.relu(v) if relu else v
    y64, y32 = restated(torch.float64), restated(torch.float32)
    e_hip = (y[:n].double() - y64).abs().max().item()
    e_32 = (y32.double() - y64).abs().max().item()
    floor = 2 * EPS32 * y64.abs().max().item()
    assert e_hip <= 2 * e_32 + floor, (name, e_hip, e_32)
    # bitwise repeatable
    y2 = SP.sparse_conv(plan, m, lvl, _g(xa), _g(W), xb=None if xb is None else _g(xb), scale=None if scale is None else _g(scale),
                        shift=None if shift is None else _g(shift), residual=None if res is None else _g(res), relu=relu,
                        nsplit=nsplit).cpu()
    assert torch.equal(y[:n], y2[:n])


def test_dense_grid_on_device():
    ax = np.arange(-4, 4)
    g3 = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rows = np.concatenate([np.zeros((len(g3), 1), np.int64), g3], 1)[np.random.default_rng(5).permutation(len(g3))]
    plan = gmf_amd.SparsePlan(_g(rows).int(), 2, [(3, 0, 0), (3, 1, 0), (3, 0, 1)])
    lv = plan.to_host()["levels"]
    g = torch.Generator().manual_seed(6)
    x = torch.randn(len(rows), 8, generator=g)
    W = torch.randn(27, 8, 5, generator=g)
    X = torch.zeros((1, 8, 8, 8, 8), dtype=torch.float64)
    c = torch.as_tensor(rows[:, 1:] + 4)
    X[0, :, c[:, 0], c[:, 1], c[:, 2]] = x.double().t()
    w = W.double().reshape(3, 3, 3, 8, 5)
    wt = w.permute(4, 3, 2, 1, 0)
    at = lambda Y, r, step: Y[0, :, (r[:, 1] + 4) // step, (r[:, 2] + 4) // step, (r[:, 3] + 4) // step].t()   # noqa: E731
    y1 = SP.sparse_conv(plan, 0, 0, _g(x), _g(W)).cpu().double()
    assert torch.allclose(y1, at(F.conv3d(X, wt, padding=1), torch.as_tensor(rows), 1), rtol=1e-5, atol=1e-5)
    l1 = lv[1].long()
    y2 = SP.sparse_conv(plan, 1, 1, _g(x), _g(W)).cpu().double()[:len(l1)]
    assert torch.allclose(y2, at(F.conv3d(X, wt, stride=2, padding=1), l1, 2), rtol=1e-5, atol=1e-5)
    xc = torch.zeros(len(rows), 8)
    xc[:len(l1)] = torch.randn(len(l1), 8, generator=g)
    Xc = torch.zeros((1, 8, 4, 4, 4), dtype=torch.float64)
    cc = (l1[:, 1:] + 4) // 2
    Xc[0, :, cc[:, 0], cc[:, 1], cc[:, 2]] = xc[:len(l1)].double().t()
    Y = F.conv_transpose3d(Xc, w.permute(3, 4, 2, 1, 0), stride=2, padding=1, output_padding=1)
    y3 = SP.sparse_conv(plan, 2, 0, _g(xc), _g(W)).cpu().double()
    assert torch.allclose(y3, at(Y, torch.as_tensor(rows), 1), rtol=1e-5, atol=1e-5)


# ---- the whole network ------------------------------------------------------------------------------------------------------

def _tokens(T=80, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, T, 128, generator=g), torch.randn(1, T, 128, generator=g)


def _model(pe, coords, feats, p_tok, q_tok):
    torch.manual_seed(21)
    m = gmf_amd.ResUNetBN2C(1, 1, D=6, pe=pe).eval()
    sd = R.conditioned_state_dict(m, coords, feats, p_tok, q_tok)
    m.load_state_dict(sd)
    return m.to(DEV), sd


@pytest.mark.parametrize("pe", [False, True])
def test_network_d6_demo_against_fp64(pe):
    coords = _demo_coords().cpu().numpy()
    M = len(coords)
    feats = torch.ones(M, 1)
    p_tok, q_tok = _tokens()
    model, sd = _model(pe, coords, feats, p_tok, q_tok)
    out = model(_g(coords).int(), _g(feats), p_tokens=_g(p_tok), q_tokens=_g(q_tok)).cpu()
    gmf_amd.check_status()
    lm = R.levels_and_maps(coords)
    y64, _ = R.resunet_forward(sd, coords, feats, p_tok, q_tok, pe, levels_maps=lm)
    y32, _ = R.resunet_forward(sd, coords, feats, p_tok, q_tok, pe, dtype=torch.float32, levels_maps=lm)
    assert out.shape == (M, 1)
    e_hip = (out.double() - y64).abs().max().item()
    e_32 = (y32.double() - y64).abs().max().item()
    assert y64.abs().max().item() > 0.1                       # conditioned: O(1) logits
    assert e_hip <= 1e-4, e_hip
    assert e_hip <= 4 * e_32 + 4 * EPS32 * y64.abs().max().item(), (e_hip, e_32)


def test_network_images_equal_tokens():
    coords = _set("d6")
    feats = torch.ones(len(coords), 1)
    p_tok, q_tok = _tokens()
    model, _ = _model(False, coords, feats, p_tok, q_tok)
    img_p, img_q = synthetic.seeded_images(2, 120, 160).split(1)
    img_p, img_q = _g(img_p).contiguous(), _g(img_q).contiguous()
    with torch.no_grad():
        tp = model.img_encoder(img_p).flatten(2).permute(0, 2, 1).contiguous()
        tq = model.img_encoder(img_q).flatten(2).permute(0, 2, 1).contiguous()
    c, f = _g(coords).int(), _g(feats)
    a = model(c, f, p_image=img_p, q_image=img_q)
    b = model(c, f, p_tokens=tp, q_tokens=tq)
    assert torch.equal(a, b)


@pytest.mark.parametrize("pe", [False, True])
def test_network_properties(pe):
    coords = _set("d6")
    M = len(coords)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(M, 1, generator=g)
    p_tok, q_tok = _tokens()
    model, _ = _model(pe, coords, feats, p_tok, q_tok)
    c, f, pt, qt = _g(coords).int(), _g(feats), _g(p_tok), _g(q_tok)
    y = model(c, f, p_tokens=pt, q_tokens=qt)
    assert torch.equal(y, model(c, f, p_tokens=pt, q_tokens=qt))               # two calls
    perm = torch.as_tensor(np.random.default_rng(4).permutation(M), device=DEV)
    assert torch.equal(model(c[perm].contiguous(), f[perm].contiguous(), p_tokens=pt, q_tokens=qt), y[perm])
    # graph capture and replay
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model(c, f, p_tokens=pt, q_tokens=qt)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yg = model(c, f, p_tokens=pt, q_tokens=qt)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y)
    gmf_amd.check_status()


def test_ragged_batches_equal_per_batch_calls():
    rows = _set("d3")
    plan = _plan(rows)
    lv = plan.to_host()["levels"]
    g = torch.Generator().manual_seed(8)
    x = torch.randn(len(rows), 16, generator=g)
    W = torch.randn(27, 16, 24, generator=g)
    y0 = SP.sparse_conv(plan, 0, 0, _g(x), _g(W)).cpu()
    y1 = SP.sparse_conv(plan, 4, 1, _g(x), _g(W)).cpu()[:len(lv[1])]
    for b in np.unique(rows[:, 0]):
        sel = np.nonzero(rows[:, 0] == b)[0]
        pb = _plan(rows[sel])
        assert torch.equal(SP.sparse_conv(pb, 0, 0, _g(x[sel]), _g(W)).cpu(), y0[sel])
        s1 = (lv[1][:, 0] == int(b)).nonzero().reshape(-1)
        yb = SP.sparse_conv(pb, 4, 1, _g(x[sel]), _g(W)).cpu()[:len(s1)]
        assert torch.equal(yb, y1[s1])


def test_conv_slicing_and_row_groups():
    """The offset-major form with many slices (first-touch partial rows, slice-ordered reduction) against fp64, and bitwise
    equality of the same slicing on a plan whose rows are split into other row groups (the per-batch plan of one batch)."""
    rows = _set("d3")
    plan = _plan(rows)
    lv = R.build_levels(rows, 4)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(len(rows), 40, generator=g)
    W = torch.randn(27, 40, 72, generator=g) / 40 ** 0.5
    for nsplit in (1, 4, 27):
        y = SP.sparse_conv(plan, 4, 1, _g(x), _g(W), nsplit=nsplit).cpu()[:len(lv[1])]
        y64 = R.conv(x, R.map_between(lv, 3, 1, 0), W, len(lv[1]))
        y32 = R.conv(x, R.map_between(lv, 3, 1, 0), W, len(lv[1]), torch.float32)
        e_hip, e_32 = (y.double() - y64).abs().max().item(), (y32.double() - y64).abs().max().item()
        assert e_hip <= 2 * e_32 + 2 * EPS32 * y64.abs().max().item(), (nsplit, e_hip, e_32)


def test_out_must_not_alias_inputs():
    plan, _, _ = _d6_plan()
    x = torch.randn(plan.M, 32, device=DEV)
    W = torch.randn(plan.K[0], 32, 32, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps `xa`"):
        SP.sparse_conv(plan, 0, 0, x, W, out=x)
    res = torch.randn(plan.M, 32, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps `residual`"):
        SP.sparse_conv(plan, 0, 0, x, W, residual=res, out=res)


def test_packed_weights_follow_load_state_dict_and_inplace_edits():
    coords = _set("d6")
    feats = torch.ones(len(coords), 1)
    p_tok, q_tok = _tokens()
    model, sd = _model(False, coords, feats, p_tok, q_tok)
    c, f, pt, qt = _g(coords).int(), _g(feats), _g(p_tok), _g(q_tok)
    lm = R.levels_and_maps(coords)

    def check(state):
        out = model(c, f, p_tokens=pt, q_tokens=qt).cpu().double()
        y64, _ = R.resunet_forward(state, coords, feats, p_tok, q_tok, False, levels_maps=lm)
        assert (out - y64).abs().max().item() <= 1e-4
        return out
    a = check(sd)
    sd2 = dict(sd)
    g = torch.Generator().manual_seed(5)
    sd2["block2.conv1.kernel"] = sd["block2.conv1.kernel"] * (1 + 0.5 * torch.rand(sd["block2.conv1.kernel"].shape, generator=g))
    sd2["norm3.bn.running_mean"] = sd["norm3.bn.running_mean"] + 0.3
    model.load_state_dict(sd2)                          # a second load after a forward has packed the weights
    b = check(sd2)
    assert not torch.equal(a, b)
    with torch.no_grad():                               # an in-place edit of a packed parameter
        model.final.bias.add_(0.25)
    sd3 = dict(sd2, **{"final.bias": sd2["final.bias"] + 0.25})
    c3 = check(sd3)
    assert torch.allclose(c3, b + 0.25, atol=1e-5)
