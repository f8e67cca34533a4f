"""Host tests of the sparse inlier network (gmf_amd/sparse.py): the float64 restatement (tests/sparse_reference.py) against dense
torch convolutions, the state_dict surface against the reference's, and the argument checks.  No device needed."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gmf_amd
from gmf_amd import sparse as SP

import sparse_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _grid(lo, hi):
    ax = np.arange(lo, hi)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(3)
    g = g[rng.permutation(len(g))]                     # the level-0 order is the input order, whatever it is
    return np.concatenate([np.zeros((len(g), 1), np.int64), g], 1)


def _dense(rows, x, lo, n):
    X = torch.zeros((1, x.shape[1], n, n, n), dtype=torch.float64)
    c = torch.as_tensor(rows[:, 1:] - lo)
    X[0, :, c[:, 0], c[:, 1], c[:, 2]] = x.t()
    return X


def _at(Y, rows, lo, step=1):
    c = torch.as_tensor((rows[:, 1:] - lo) // step)
    return Y[0, :, c[:, 0], c[:, 1], c[:, 2]].t()


def _torch_weight(W, transpose=False):      # ME kernel [27, Cin, Cout], first axis fastest -> [Cout, Cin, kx, ky, kz]
    cin, cout = W.shape[1], W.shape[2]
    w = W.reshape(3, 3, 3, cin, cout)           # [kz, ky, kx, Cin, Cout]
    return w.permute(3, 4, 2, 1, 0) if transpose else w.permute(4, 3, 2, 1, 0)


def test_restatement_stride1_equals_conv3d():
    rows = _grid(-3, 3)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(len(rows), 5, generator=g, dtype=torch.float64)
    W = torch.randn(27, 5, 7, generator=g, dtype=torch.float64)
    lv = R.build_levels(rows, 1)
    y = R.conv(x, R.map_between(lv, 3, 0, 0), W, len(rows))
    ref = _at(F.conv3d(_dense(rows, x, -3, 6), _torch_weight(W), padding=1), rows, -3)
    assert torch.allclose(y, ref, rtol=0, atol=1e-12)


def test_restatement_stride2_equals_strided_conv3d():
    rows = _grid(-4, 4)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(len(rows), 4, generator=g, dtype=torch.float64)
    W = torch.randn(27, 4, 6, generator=g, dtype=torch.float64)
    lv = R.build_levels(rows, 2)
    assert len(lv[1]) == 64 and lv[1][:, 1:].min() == -4 and lv[1][:, 1:].max() == 2       # floor for negative coordinates
    y = R.conv(x, R.map_between(lv, 3, 1, 0), W, len(lv[1]))
    ref = _at(F.conv3d(_dense(rows, x, -4, 8), _torch_weight(W), stride=2, padding=1), lv[1], -4, 2)
    assert torch.allclose(y, ref, rtol=0, atol=1e-12)


def test_restatement_transposed_equals_conv_transpose3d():
    rows = _grid(-4, 4)
    g = torch.Generator().manual_seed(2)
    lv = R.build_levels(rows, 2)
    xc = torch.randn(len(lv[1]), 6, generator=g, dtype=torch.float64)
    W = torch.randn(27, 6, 3, generator=g, dtype=torch.float64)
    y = R.conv(xc, R.map_between(lv, 3, 0, 1), W, len(rows))
    Xc = torch.zeros((1, 6, 4, 4, 4), dtype=torch.float64)
    c = torch.as_tensor((lv[1][:, 1:] + 4) // 2)
    Xc[0, :, c[:, 0], c[:, 1], c[:, 2]] = xc.t()
    Y = F.conv_transpose3d(Xc, _torch_weight(W, transpose=True), stride=2, padding=1, output_padding=1)
    assert torch.allclose(y, _at(Y, rows, -4), rtol=0, atol=1e-12)


def test_restatement_k1_is_matmul():
    rows = _grid(-2, 2)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(len(rows), 9, generator=g, dtype=torch.float64)
    W = torch.randn(9, 5, generator=g, dtype=torch.float64)
    lv = R.build_levels(rows, 1)
    assert torch.allclose(R.conv(x, R.map_between(lv, 1, 0, 0), W, len(rows)), x @ W, rtol=0, atol=1e-12)
    assert torch.equal(R.conv(x, None, W, len(rows)), x @ W)


def test_kernel_conventions_agree():
    for k, D in ((3, 3), (3, 6), (5, 2), (1, 4)):
        assert np.array_equal(np.array(SP.kernel_offsets(k, D)).reshape(-1, D), R.kernel_offsets(k, D))
    assert SP.kernel_offsets(3, 2)[:4] == [(-1, -1), (0, -1), (1, -1), (-1, 0)]      # first spatial axis fastest
    assert SP.kernel_shape(1, 6, 96, 64) == (96, 64)
    assert SP.kernel_shape(3, 6, 1, 32) == (729, 1, 32)


@pytest.mark.parametrize("pe", [False, True])
def test_state_dict_matches_reference(pe):
    with open(os.path.join(HERE, "golden", "dgr_inlier_state_dict_keys.json")) as f:
        ref = json.load(f)[f"pe={pe}"]
    m = gmf_amd.ResUNetBN2C(1, 1, D=6, pe=pe)
    ours = {k: list(v.shape) for k, v in m.state_dict().items()}
    unused = {k for k in ref if k.startswith(SP._UNUSED_IMAGE_KEYS)}
    assert unused and all(k.startswith("img_encoder.backbone.") for k in unused)
    assert ours == {k: v for k, v in ref.items() if k not in unused}
    # a strict load of a reference-shaped state_dict (the unused encoder stages included) succeeds
    sd = {k: torch.zeros(v) for k, v in ref.items()}
    for k, v in m.state_dict().items():
        if not torch.is_floating_point(v):
            sd[k] = v
    m.load_state_dict(sd, strict=True)


def test_trunk_table_is_in_the_packed_layer_order():
    """sparse.TRUNK names the 23 convolutions in the order of kResunetLayers (csrc/gmf_api.cpp), which is the order of
    `pack_resunet`'s list that the forwards index, and in the order the modules are registered; every entry's map writes its
    level."""
    import re
    from gmf_amd import fcgf
    with open(os.path.join(HERE, "..", "gmf_amd", "csrc", "gmf_api.cpp")) as f:
        src = f.read()
    table = src[src.index("kResunetLayers[GMF_SPARSE_RESUNET_LAYERS] = {"):]
    c_order = re.findall(r'\{"([\w.]+)", "([\w.]*)", "[\w.]*"\}', table[:table.index("};")])
    assert len(SP.TRUNK) == len(c_order) == 23
    assert [(conv, norm or "") for conv, norm, _, _ in SP.TRUNK] == c_order
    assert (SP.TRUNK[SP.CONV1_TR][0], SP.TRUNK[SP.FINAL][0]) == ("conv1_tr", "final")
    for m in (gmf_amd.ResUNetBN2C(1, 1, D=3, pe=True), fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=7, D=3)):
        keys = list(m.state_dict())
        assert [k[:-len(".kernel")] for k in keys if k.endswith(".kernel")] == [conv for conv, _, _, _ in SP.TRUNK]
        assert [k[:-len(".bn.weight")] for k in keys if k.endswith(".bn.weight")] == [n for _, n, _, _ in SP.TRUNK if n]
    for conv, _, mi, lvl in SP.TRUNK:
        assert (mi is None and lvl == 0) or SP._NET_MAPS[mi][1] == lvl, conv
    # the strided convolutions: down over map (3, l + 1, l), up over its transpose
    assert {c: SP._NET_MAPS[mi] for c, _, mi, _ in SP.TRUNK if mi is not None and "block" not in c} == {
        "conv1": (3, 0, 0), "conv2": (3, 1, 0), "conv3": (3, 2, 1), "conv4": (3, 3, 2), "conv4_tr": (3, 2, 3), "conv3_tr": (3, 1, 2),
        "conv2_tr": (3, 0, 1)}


def test_argument_checks_without_device():
    m = gmf_amd.ResUNetBN2C(1, 1, D=6).eval()
    coords = torch.zeros((4, 7), dtype=torch.int32)
    feats = torch.ones((4, 1))
    tok = torch.zeros((1, 10, 128))
    with pytest.raises(RuntimeError, match="HIP device"):
        m(coords, feats, p_tokens=tok, q_tokens=tok)
    with pytest.raises(RuntimeError, match="int32"):
        m(coords.long(), feats, p_tokens=tok, q_tokens=tok)
    with pytest.raises(RuntimeError, match=r"\[M, 1 \+ D\]"):
        m(torch.zeros((4, 8), dtype=torch.int32), feats, p_tokens=tok, q_tokens=tok)
    with pytest.raises(RuntimeError, match="one image pair"):
        m(coords, feats, p_tokens=torch.zeros((2, 10, 128)), q_tokens=torch.zeros((2, 10, 128)))
    with pytest.raises(RuntimeError, match="one image pair"):
        m(coords, feats, p_image=torch.zeros((2, 3, 32, 32)), q_image=torch.zeros((2, 3, 32, 32)))
    with pytest.raises(RuntimeError, match="p_image and q_image"):
        m(coords, feats)
    with pytest.raises(RuntimeError, match="eval"):
        m.train()(coords, feats, p_tokens=tok, q_tokens=tok)
    with pytest.raises(ValueError, match="D must be"):
        gmf_amd.ResUNetBN2C(1, 1, D=7)
    with pytest.raises(NotImplementedError, match="kernel volume"):
        gmf_amd.ResUNetBN2C(1, 1, D=6, conv1_kernel_size=5)
    with pytest.raises(NotImplementedError, match="hypercube"):
        gmf_amd.ResUNetBN2CX(1, 1, D=6)
    with pytest.raises(NotImplementedError, match="normalize_feature"):
        gmf_amd.ResUNetBN2C(1, 1, D=6, normalize_feature=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        gmf_amd.SparsePlan(coords, 4, [(3, 0, 0)])
    with pytest.raises(NotImplementedError, match="kernel volume"):
        SP._check_map_desc([(5, 0, 0)], 6, 1, "SparsePlan")
    with pytest.raises(RuntimeError, match="differ by at most one"):
        SP._check_map_desc([(3, 2, 0)], 3, 4, "SparsePlan")


def test_inlier_coordinates():
    c0 = torch.tensor([[0, 1, 2, 3], [0, -4, 5, 6], [0, 7, 8, -9]], dtype=torch.int32)
    c1 = torch.tensor([[0, 10, 11, 12], [0, 13, -14, 15]], dtype=torch.int32)
    i0, i1 = torch.tensor([2, 0, 1]), torch.tensor([1, 1, 0])
    out = gmf_amd.inlier_coordinates(c0, c1, i0, i1)
    assert out.dtype == torch.int32 and out.shape == (3, 7)
    assert out.tolist() == [[0, 7, 8, -9, 13, -14, 15], [0, 1, 2, 3, 13, -14, 15], [0, -4, 5, 6, 10, 11, 12]]
