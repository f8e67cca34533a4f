"""Host tests of FCGF (gmf_amd/fcgf.py) and DGR's pipeline (gmf_amd/dgr.py): the state_dict surface against the reference's,
the float64 restatement against a dense convolution, model lookup, config parsing and the argument checks.  No device needed."""
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gmf_amd
from gmf_amd import dgr, fcgf
from gmf_amd import sparse as SP

import fcgf_reference as FR
import sparse_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
_FUSION_PREFIXES = ("perceiver_io.", "img_encoder.", "image_fusion.")


def _ref_keys():
    with open(os.path.join(HERE, "golden", "dgr_inlier_state_dict_keys.json")) as f:
        ref = json.load(f)["pe=False"]
    return {k: v for k, v in ref.items() if not k.startswith(_FUSION_PREFIXES)}


def test_state_dict_matches_reference():
    """resunet.py and resunet_new.py build the same modules but for the three fusion attributes, so FCGF's keys are the inlier
    network's without them; built like the inlier network (Cin 1, Cout 1, D 6) the shapes agree too."""
    ref = _ref_keys()
    m6 = fcgf.ResUNetBN2C(1, 1, D=6)
    assert {k: list(v.shape) for k, v in m6.state_dict().items()} == ref
    m3 = fcgf.ResUNetBN2C(1, 32, bn_momentum=0.05, conv1_kernel_size=7, normalize_feature=True, D=3)
    sd = m3.state_dict()
    assert set(sd) == set(ref)
    assert tuple(sd["conv1.kernel"].shape) == (343, 1, 32)
    assert tuple(sd["conv1_tr.kernel"].shape) == (96, 64)
    assert tuple(sd["final.kernel"].shape) == (64, 32) and tuple(sd["final.bias"].shape) == (1, 32)
    m3.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)


def test_restatement_k7_cin1_equals_conv3d():
    ax = np.arange(-5, 5)
    g3 = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    keep = np.random.default_rng(0).random(len(g3)) < 0.6                # a sparse subset, in shuffled order
    g3 = g3[keep][np.random.default_rng(1).permutation(int(keep.sum()))]
    rows = np.concatenate([np.zeros((len(g3), 1), np.int64), g3], 1)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(len(rows), 1, generator=g, dtype=torch.float64)
    W = torch.randn(343, 1, 6, generator=g, dtype=torch.float64)
    lv = R.build_levels(rows, 1)
    y = R.conv(x, R.map_between(lv, 7, 0, 0), W, len(rows))
    X = torch.zeros((1, 1, 10, 10, 10), dtype=torch.float64)
    c = torch.as_tensor(rows[:, 1:] + 5)
    X[0, :, c[:, 0], c[:, 1], c[:, 2]] = x.t()
    w = W.reshape(7, 7, 7, 1, 6).permute(4, 3, 2, 1, 0)         # offset index: first spatial axis fastest
    ref = F.conv3d(X, w, padding=3)[0, :, c[:, 0], c[:, 1], c[:, 2]].t()
    assert torch.allclose(y, ref, rtol=0, atol=1e-12)


def test_head_restatement_normalises():
    g = torch.Generator().manual_seed(3)
    xa, xb = torch.randn(9, 64, generator=g), torch.randn(9, 32, generator=g)
    y = FR.head(xa, xb, torch.randn(96, 64, generator=g), torch.randn(64, 32, generator=g), torch.randn(32, generator=g), True)
    assert torch.allclose(y.norm(dim=1), torch.ones(9, dtype=torch.float64), atol=1e-12)
    z = FR.head(torch.zeros(2, 64), torch.zeros(2, 32), torch.randn(96, 64), torch.randn(64, 32), None, True)
    assert torch.equal(z, torch.zeros_like(z))


def test_argument_checks_without_device():
    m = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=7, D=3).eval()
    coords = torch.zeros((4, 4), dtype=torch.int32)
    feats = torch.ones((4, 1))
    with pytest.raises(RuntimeError, match="HIP device"):
        m(coords, feats)
    with pytest.raises(RuntimeError, match="int32"):
        m(coords.long(), feats)
    with pytest.raises(RuntimeError, match=r"\[M, 1 \+ D\]"):
        m(torch.zeros((4, 8), dtype=torch.int32), feats)
    with pytest.raises(RuntimeError, match="eval"):
        m.train()(coords, feats)
    with pytest.raises(ValueError, match="D must be"):
        fcgf.ResUNetBN2C(1, 32, D=0)
    with pytest.raises(NotImplementedError, match="kernel volume"):
        fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=11, D=3)
    with pytest.raises(ValueError, match="odd"):
        fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=4, D=3)
    with pytest.raises(NotImplementedError, match="out_channels"):
        fcgf.ResUNetBN2C(1, 65, D=3)
    with pytest.raises(NotImplementedError, match="hypercube"):
        fcgf.ResUNetBN2CX(1, 32, D=3)
    assert m.narrow_conv1 is True
    # the top-level name stays the inlier network
    assert gmf_amd.ResUNetBN2C is SP.ResUNetBN2C and gmf_amd.fcgf.ResUNetBN2C is fcgf.ResUNetBN2C
    with pytest.raises(RuntimeError, match="HIP device"):
        gmf_amd.sparse_head_l2(None, 0, torch.zeros(4, 64), torch.zeros(64, 64), torch.zeros(64, 32))


def test_load_model():
    assert dgr.load_model("ResUNetBN2C") is fcgf.ResUNetBN2C
    assert dgr.load_model("anything", corrs=True) is gmf_amd.ResUNetBN2C
    for name in ("ResUNetBN2B", "ResUNetBN2D", "ResUNetBN2E", "ResUNetIN2C", "ResUNetBN2CX", "SimpleNetBN2C", "PyramidNet",
                 "NoSuchNet"):
        with pytest.raises(NotImplementedError, match="built: ResUNetBN2C"):
            dgr.load_model(name)


_NC = {"feat_model": "ResUNetBN2C", "feat_model_n_out": 32, "bn_momentum": 0.05, "feat_conv1_kernel_size": 7,
       "normalize_feature": True, "inlier_model": "ResUNetBN2C", "inlier_conv1_kernel_size": 3, "inlier_feature_type": "ones",
       "voxel_size": 0.05, "nn_max_n": 500}


def test_config_parsing_dict_and_attribute_forms():
    want = dict(_NC)
    assert dgr.parse_network_config(_NC) == want
    assert dgr.parse_network_config(types.SimpleNamespace(**_NC)) == want
    legacy = {k: v for k, v in _NC.items() if not k.startswith("feat_")}
    legacy.update(model="ResUNetBN2C", model_n_out=16, conv1_kernel_size=5)
    got = dgr.parse_network_config(types.SimpleNamespace(**legacy))
    assert (got["feat_model"], got["feat_model_n_out"], got["feat_conv1_kernel_size"]) == ("ResUNetBN2C", 16, 5)
    assert dgr.parse_network_config(legacy) == got
    with pytest.raises(KeyError, match="voxel_size"):
        dgr.parse_network_config({k: v for k, v in _NC.items() if k != "voxel_size"})
    assert [dgr.inlier_in_channels(t, 32) for t in ("ones", "coords", "feats")] == [1, 6, 64]
    with pytest.raises(ValueError, match="inlier_feature_type"):
        dgr.inlier_in_channels("xyz", 32)


@pytest.mark.parametrize("ftype", ["ones", "coords", "feats"])
def test_pipeline_builds_from_a_checkpoint_mapping(ftype):
    nc = types.SimpleNamespace(**dict(_NC, inlier_feature_type=ftype))
    fm = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=7, normalize_feature=True, D=3)
    im = gmf_amd.ResUNetBN2C(dgr.inlier_in_channels(ftype, 32), 1, D=6, pe=True)
    state = {"config": nc, "state_dict": fm.state_dict(), "state_dict_inlier": im.state_dict()}
    cfg = {"clip_weight_thresh": 0.05, "weights": None}
    d = dgr.DeepGlobalRegistration(cfg, device="cpu", state=state)
    assert d.voxel_size == 0.05 and d.fcgf_model.conv1_kernel_size == 7 and d.fcgf_model.normalize_feature
    assert d.inlier_model.in_channels == dgr.inlier_in_channels(ftype, 32) and d.inlier_model.pe
    assert not d.fcgf_model.training and not d.inlier_model.training
    with pytest.raises(RuntimeError, match="HIP device"):
        d.register(np.zeros((10, 3)), np.zeros((10, 3)))
