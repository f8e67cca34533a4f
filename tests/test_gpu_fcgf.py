"""GPU tests of FCGF (gmf_amd/fcgf.py), its two kernels (sparse_conv_narrow, sparse_head_l2) and DGR's register()
(gmf_amd/dgr.py) against the float64 restatements of tests/fcgf_reference.py and tests/sparse_reference.py."""
import math
import os
import types

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import dgr, fcgf
from gmf_amd import sparse as SP

import fcgf_reference as FR
import sparse_reference as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(np.finfo(np.float32).eps)


def _g(x):
    return torch.as_tensor(x).to(DEV)


@pytest.fixture(autouse=True)
def _clean_status():
    yield
    gmf_amd.check_status()


_CLOUDS = {}


def _clouds():
    if "c" not in _CLOUDS:
        z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_demo_clouds.npz"))
        _CLOUDS["c"] = (z["cloud0"].astype(np.float32), z["cloud1"].astype(np.float32))
    return _CLOUDS["c"]


def _voxel_coords(xyz, v, batch):
    """DGR's preprocess on the device: voxel_select, floor(xyz / v) -> int32 [M, 4] rows (batch, x, y, z)."""
    x = _g(xyz)
    sel = gmf_amd.voxel_select(x, v)
    c = torch.floor(x[sel].double() / v).int()
    return torch.cat([torch.full((len(c), 1), batch, dtype=torch.int32, device=DEV), c], 1)


_PAIR = {}


def _pair_coords(v=0.05):
    """The two demo fragments at 5 cm as batches 0 and 1 of one coordinate set (about 4.6 k voxels each)."""
    if v not in _PAIR:
        c0, c1 = _clouds()
        _PAIR[v] = torch.cat([_voxel_coords(c0, v, 0), _voxel_coords(c1, v, 1)]).contiguous()
    return _PAIR[v]


_MODELS = {}


def _model(k, cin, normalize):
    """A conditioned FCGF on the demo pair (conditioning does not depend on normalize_feature)."""
    coords = _pair_coords().cpu().numpy()
    g = torch.Generator().manual_seed(100 * k + cin)
    feats = torch.ones(len(coords), 1) if cin == 1 else torch.randn(len(coords), cin, generator=g)
    if (k, cin) not in _MODELS:
        torch.manual_seed(7)
        m = fcgf.ResUNetBN2C(cin, 32, conv1_kernel_size=k, D=3)
        _MODELS[(k, cin)] = (FR.conditioned_state_dict(m, coords, feats), R.levels_and_maps(coords, k))
    sd, lm = _MODELS[(k, cin)]
    m = fcgf.ResUNetBN2C(cin, 32, conv1_kernel_size=k, normalize_feature=normalize, D=3)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd, lm, coords, feats


# ---- 1. the network against fp64 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_fcgf_pair_against_fp64(k, cin, normalize):
    model, sd, lm, coords, feats = _model(k, cin, normalize)
    out = model(_g(coords), _g(feats)).cpu()
    y64, _ = FR.fcgf_forward(sd, coords, feats, k, normalize, levels_maps=lm)
    y32, _ = FR.fcgf_forward(sd, coords, feats, k, normalize, dtype=torch.float32, levels_maps=lm)
    assert out.shape == (len(coords), 32)
    e_hip = (out.double() - y64).abs().max().item()
    e_32 = (y32.double() - y64).abs().max().item()
    ymax = y64.abs().max().item()
    assert ymax > 0.1
    assert e_hip <= 1e-5, e_hip
    assert e_hip <= 4 * e_32 + 4 * EPS32 * ymax, (e_hip, e_32)
    if normalize:
        assert (out.double().norm(dim=1) - 1).abs().max().item() <= 1e-6


def test_narrow_conv1_equals_generic_within_fp32():
    """The A/B switch: conv1 on the generic kernel gives the same network within fp32 rounding."""
    model, _, _, coords, feats = _model(7, 1, True)
    c, f = _g(coords), _g(feats)
    a = model(c, f)
    model.narrow_conv1 = False
    b = model(c, f)
    model.narrow_conv1 = True
    assert (a - b).abs().max().item() <= 1e-5


# ---- 2. the narrow-input kernel alone ------------------------------------------------------------------------------------------

def _random_rows(M, D, span, batches, seed):
    rng = np.random.default_rng(seed)
    rows = set()
    while len(rows) < M:
        rows.add((int(rng.choice(batches)),) + tuple(int(v) for v in rng.integers(-span, span, D)))
    out = np.array(sorted(rows), dtype=np.int64)
    return out[rng.permutation(M)]


NARROW = [(1, 3, 3, 32), (3, 3, 3, 64), (6, 3, 3, 13), (8, 3, 3, 64), (1, 5, 3, 32), (3, 5, 3, 64), (6, 5, 3, 7),
          (8, 5, 3, 64), (1, 7, 3, 32), (3, 7, 3, 64), (6, 7, 3, 13), (8, 7, 3, 64), (1, 3, 6, 32), (8, 3, 6, 20)]


@pytest.mark.parametrize("epi", [False, True])
@pytest.mark.parametrize("case", NARROW, ids=[f"cin{c}-k{k}-D{D}-cout{o}" for c, k, D, o in NARROW])
def test_narrow_kernel_against_fp64(case, epi):
    cin, k, D, cout = case
    rows = _random_rows(700, D, 7 if D == 3 else 3, [0, 1, 2], 11 + D)
    plan = gmf_amd.SparsePlan(_g(rows).int(), 2, [(k, 0, 0), (k, 1, 0)])
    lv = R.build_levels(rows, 2)
    K = k ** D
    g = torch.Generator().manual_seed(cin * 1000 + K + cout)
    x = torch.randn(len(rows), cin, generator=g)
    W = torch.randn(K, cin, cout, generator=g) / (27 * cin) ** 0.5
    scale = 1 + 0.2 * torch.randn(cout, generator=g) if epi else None
    shift = 0.2 * torch.randn(cout, generator=g) if epi else None
    for m, lvl in ((0, 0), (1, 1)):
        n = len(lv[lvl])
        res = torch.randn(len(rows), cout, generator=g) if epi else None
        out = torch.full((len(rows), cout), 7.0, device=DEV)
        y = SP.sparse_conv_narrow(plan, m, lvl, _g(x), _g(W), scale=None if scale is None else _g(scale),
                                  shift=None if shift is None else _g(shift), residual=None if res is None else _g(res),
                                  relu=epi, out=out).cpu()
        assert torch.all(y[n:] == 7.0)                               # rows past the level's count are untouched
        cmap = R.map_between(lv, k, lvl, 0)

        def restated(dtype):
            v = R.conv(x, cmap, W, n, dtype)
            if epi:
                v = torch.relu(v * scale.to(dtype) + shift.to(dtype) + res[:n].to(dtype))
            return v
        y64, y32 = restated(torch.float64), restated(torch.float32)
        e_hip = (y[:n].double() - y64).abs().max().item()
        e_32 = (y32.double() - y64).abs().max().item()
        assert e_hip <= 2 * e_32 + 2 * EPS32 * y64.abs().max().item(), (m, e_hip, e_32)
        y2 = SP.sparse_conv_narrow(plan, m, lvl, _g(x), _g(W), scale=None if scale is None else _g(scale),
                                   shift=None if shift is None else _g(shift), residual=None if res is None else _g(res),
                                   relu=epi).cpu()
        assert torch.equal(y[:n], y2[:n])


# ---- 3. the head alone ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [False, True])
def test_head_against_fp64(normalize):
    rows = _random_rows(900, 3, 9, [0, 1], 5)
    plan = gmf_amd.SparsePlan(_g(rows).int(), 2, [(3, 1, 0)])
    n1 = len(R.build_levels(rows, 2)[1])
    g = torch.Generator().manual_seed(9)
    M = len(rows)
    xa, xb = torch.relu(torch.randn(M, 64, generator=g)), torch.relu(torch.randn(M, 32, generator=g))
    xa[5], xb[5] = 0, 0                                              # an all-zero row
    W1, W2 = torch.randn(96, 64, generator=g) / 96 ** 0.5, torch.randn(64, 32, generator=g) / 64 ** 0.5
    bias = 0.1 * torch.randn(1, 32, generator=g)
    y = SP.sparse_head_l2(plan, 0, _g(xa), _g(W1), _g(W2), xb=_g(xb), bias=_g(bias), normalize=normalize).cpu()
    y64 = FR.head(xa, xb, W1, W2, bias, normalize)
    y32 = FR.head(xa, xb, W1, W2, bias, normalize, dtype=torch.float32)
    e_hip = (y.double() - y64).abs().max().item()
    e_32 = (y32.double() - y64).abs().max().item()
    assert e_hip <= 4 * e_32 + 4 * EPS32 * y64.abs().max().item(), (e_hip, e_32)
    if normalize:
        assert (y.double().norm(dim=1) - 1).abs().max().item() <= 1e-6
    # zero input and zero bias: zeros, not NaN
    z = SP.sparse_head_l2(plan, 0, _g(xa), _g(W1), _g(W2), xb=_g(xb), normalize=True).cpu()
    assert torch.equal(z[5], torch.zeros(32))
    assert torch.isfinite(z).all()
    # rows past the level's count are untouched
    out = torch.full((M, 32), 7.0, device=DEV)
    SP.sparse_head_l2(plan, 1, _g(xa), _g(W1), _g(W2), xb=_g(xb), bias=_g(bias), normalize=normalize, out=out)
    out = out.cpu()
    assert torch.all(out[n1:] == 7.0) and torch.equal(out[:n1], y[:n1])


# ---- 4. bitwise properties -------------------------------------------------------------------------------------------------------

def test_pair_permutation_repeat_and_graph_are_bitwise():
    model, _, _, coords, feats = _model(7, 1, True)
    c, f = _g(coords), _g(feats)
    y = model(c, f)
    assert torch.equal(y, model(c, f))                                              # two calls
    for b in (0, 1):                                                                  # the pair = two single-cloud calls
        sel = (c[:, 0] == b).nonzero().reshape(-1)
        assert torch.equal(model(c[sel].contiguous(), f[sel].contiguous()), y[sel])
    perm = torch.as_tensor(np.random.default_rng(4).permutation(len(coords)), device=DEV)
    assert torch.equal(model(c[perm].contiguous(), f[perm].contiguous()), y[perm])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model(c, f)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yg = model(c, f)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y)


def _quantized_cloud():
    return (np.round(_clouds()[0].astype(np.float64) * 1024) / 1024).astype(np.float32)


def test_shift_by_8_voxels_gives_identical_features():
    v = 0.0625
    xyz = _quantized_cloud()
    shift = np.array([8, -16, 24], np.float32) * v
    c0 = _voxel_coords(xyz, v, 0)
    c1 = _voxel_coords(xyz + shift, v, 1)
    assert torch.equal(c1[:, 1:], c0[:, 1:] + torch.as_tensor([8, -16, 24], dtype=torch.int32, device=DEV))
    torch.manual_seed(3)
    m = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=7, normalize_feature=True, D=3)
    coords = torch.cat([c0, c1]).contiguous()
    m.load_state_dict(FR.conditioned_state_dict(m, coords.cpu().numpy(), torch.ones(len(coords), 1)))
    m = m.to(DEV).eval()
    y = m(coords, torch.ones((len(coords), 1), device=DEV))
    assert torch.equal(y[:len(c0)], y[len(c0):])


# ---- 5. register() end to end ------------------------------------------------------------------------------------------------------

_NC = {"feat_model": "ResUNetBN2C", "feat_model_n_out": 32, "bn_momentum": 0.05, "feat_conv1_kernel_size": 7,
       "normalize_feature": True, "inlier_model": "ResUNetBN2C", "inlier_conv1_kernel_size": 3, "inlier_feature_type": "ones",
       "voxel_size": 0.0625, "nn_max_n": 500}
_STATE = {}


def _dgr(ftype="ones", clip=0.05):
    v = _NC["voxel_size"]
    if "fcgf" not in _STATE:
        xyz = _quantized_cloud()
        coords = torch.cat([_voxel_coords(xyz, v, 0), _voxel_coords(xyz + 0.5, v, 1)]).cpu().numpy()
        torch.manual_seed(5)
        m = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=7, normalize_feature=True, D=3)
        _STATE["fcgf"] = FR.conditioned_state_dict(m, coords, torch.ones(len(coords), 1))
    cin = dgr.inlier_in_channels(ftype, 32)
    torch.manual_seed(6)
    im = gmf_amd.ResUNetBN2C(cin, 1, D=6, pe=True)
    sd = im.state_dict()
    sd["final.kernel"] = torch.zeros_like(sd["final.kernel"])        # logit 4 on every row: the weights pass the threshold
    sd["final.bias"] = torch.full_like(sd["final.bias"], 4.0)
    state = {"config": types.SimpleNamespace(**dict(_NC, inlier_feature_type=ftype)), "state_dict": _STATE["fcgf"],
             "state_dict_inlier": sd}
    return dgr.DeepGlobalRegistration({"clip_weight_thresh": clip}, device=DEV, state=state)


def _tokens():
    g = torch.Generator().manual_seed(9)
    return _g(torch.randn(1, 80, 128, generator=g)), _g(torch.randn(1, 80, 128, generator=g))


def _pose_error(T, t_true):
    """(rotation angle from the identity in degrees, translation error in m).  atan2 of the skew and the trace parts: acos of the
    trace alone loses the angle's precision near zero."""
    R_ = T[:3, :3]
    re = math.degrees(math.atan2(np.linalg.norm(R_ - R_.T) / (2 * math.sqrt(2)), (np.trace(R_) - 1) / 2))
    return re, float(np.linalg.norm(T[:3, 3] - t_true))


@pytest.mark.parametrize("branch", ["global_registration", "safeguard"])
def test_register_recovers_a_voxel_shift(branch):
    xyz0 = _quantized_cloud()
    t_true = np.array([8, 16, -8], np.float64) * _NC["voxel_size"]
    xyz1 = xyz0 + t_true.astype(np.float32)
    d = _dgr(clip=0.05 if branch == "global_registration" else 1.0)
    pt, qt = _tokens()
    T = d.register(xyz0, xyz1, p_tokens=pt, q_tokens=qt)
    assert T.dtype == np.float64 and T.shape == (4, 4)
    assert d.last_stats["branch"] == branch, d.last_stats
    if branch == "safeguard":
        assert d.last_stats["wsum"] == 0.0 and d.last_stats["global_registration"] is None
    else:
        assert d.last_stats["wsum"] >= d.last_stats["wsum_threshold"]
    re, te = _pose_error(T, t_true)
    assert re < 0.01 and te < 1e-3, (re, te, d.last_stats)


def test_register_correspondences_equal_the_stages_by_hand():
    xyz0, xyz1 = _quantized_cloud(), _clouds()[1]
    d = _dgr()
    pt, qt = _tokens()
    T, p, q = d.register(xyz0, xyz1, p_tokens=pt, q_tokens=qt, use_corr=True)
    assert np.isfinite(T).all()
    v = _NC["voxel_size"]
    sel0, sel1 = gmf_amd.voxel_select(_g(xyz0), v), gmf_amd.voxel_select(_g(xyz1), v)
    x0, x1 = _g(xyz0)[sel0], _g(xyz1)[sel1]
    c = torch.cat([_voxel_coords(xyz0, v, 0), _voxel_coords(xyz1, v, 1)]).contiguous()
    F = d.fcgf_model(c, torch.ones((len(c), 1), device=DEV))
    idx1 = gmf_amd.find_knn_gpu(F[:len(x0)], F[len(x0):], nn_max_n=_NC["nn_max_n"], knn=1).reshape(-1)
    assert torch.equal(p, x0) and torch.equal(q, x1[idx1])


@pytest.mark.parametrize("ftype", ["ones", "feats", "coords"])
def test_register_runs_each_inlier_feature_type(ftype):
    xyz0 = _quantized_cloud()
    t_true = np.array([0, 8, 8], np.float64) * _NC["voxel_size"]
    d = _dgr(ftype)
    pt, qt = _tokens()
    T = d.register(xyz0, xyz0 + t_true.astype(np.float32), p_tokens=pt, q_tokens=qt)
    assert d.last_stats["branch"] == "global_registration"
    re, te = _pose_error(T, t_true)
    assert re < 0.01 and te < 1e-3, (ftype, re, te)
