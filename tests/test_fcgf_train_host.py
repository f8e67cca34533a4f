"""Host tests of FCGF's training path (gmf_amd.train.fcgf_train, gmf_amd.fcgf.hardest_contrastive_loss): the margins of the loss
case that the GPU test holds the device to, the restatement's own properties, the argument checks and the C header.  No device
needed."""
import os
import re

import pytest
import torch

import gmf_amd
from gmf_amd import fcgf
from gmf_amd import train as T

import fcgf_train_reference as FTR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-4


def _reference64(case, **kw):
    return FTR.hardest_contrastive_loss(case["F0"].double(), case["F1"].double(), case["pairs"], case["sel0"], case["sel1"],
                                        case["pos_sel"], case["pos_thresh"], case["neg_thresh"], **kw)


def test_loss_case_margins():
    """In float64: every hinge argument at least 1e-4 from 0, every mined row's runner-up at least 1e-4 farther than its minimum,
    at least 4 rows per side dropped by `keep` and 4 kept, every hinge active on at least a quarter of its rows and inactive on at
    least a quarter.  With that a float32 device must reproduce the selection and the masks exactly."""
    case = FTR.margin_case()
    assert tuple(case["F0"].shape) == (300, 32) and tuple(case["F1"].shape) == (257, 32)
    assert case["pos_sel"].shape[0] == 64 and case["sel0"].shape[0] == 50 and case["sel1"].shape[0] == 50
    assert case["F0"].dtype == torch.float32
    _, _, aux = _reference64(case)
    for name in ("pos_arg", "neg0_arg", "neg1_arg"):
        assert float(aux[name].abs().min()) >= MARGIN, name
    assert float((aux["D01_second"] - aux["D01"]).min()) >= MARGIN
    assert float((aux["D10_second"] - aux["D10"]).min()) >= MARGIN
    P = case["pos_sel"].shape[0]
    for keep, arg in ((aux["keep0"], aux["neg0_arg"]), (aux["keep1"], aux["neg1_arg"])):
        kept = int(keep.sum())
        assert kept >= 4 and P - kept >= 4
        active = int((arg[keep] > 0).sum())              # the hinge's rows: the kept ones
        assert active * 4 >= kept and (kept - active) * 4 >= kept
    active = int((aux["pos_arg"] > 0).sum())
    assert active * 4 >= P and (P - active) * 4 >= P


def test_small_loss_case_margins():
    """The GPU test's second case (C = 16, every pair sampled, every row a candidate; the sampler only permutes them): the same
    margins, and hardest negatives that several rows share."""
    case = FTR.margin_case(seed=3, N0=40, N1=37, C=16, K=24, P=None, H=None)
    assert case["pos_sel"] is None and case["sel0"].shape[0] == 40 and case["sel1"].shape[0] == 37
    _, _, aux = _reference64(case)
    for name in ("pos_arg", "neg0_arg", "neg1_arg"):
        assert float(aux[name].abs().min()) >= MARGIN, name
    assert float((aux["D01_second"] - aux["D01"]).min()) >= MARGIN
    assert float((aux["D10_second"] - aux["D10"]).min()) >= MARGIN
    assert aux["keep0"].any() and aux["keep1"].any() and not aux["keep0"].all() and not aux["keep1"].all()
    big = FTR.margin_case()
    for h in (aux["h01"], aux["h10"], big["pairs"][big["pos_sel"], 0]):
        assert int((torch.bincount(h) > 1).sum()) > 0


def test_loss_restatement_takes_given_rows_and_masks():
    """The reference with its own h01 / h10 and hinge masks handed back in gives the same losses and gradients."""
    case = FTR.margin_case()
    out = []
    for given in (False, True):
        F0 = case["F0"].double().requires_grad_(True)
        F1 = case["F1"].double().requires_grad_(True)
        kw = {}
        if given:
            _, _, aux = _reference64(case)
            kw = dict(h01=aux["h01"], h10=aux["h10"], masks=(aux["pos_arg"] > 0, aux["neg0_arg"] > 0, aux["neg1_arg"] > 0))
        pos, neg, _ = FTR.hardest_contrastive_loss(F0, F1, case["pairs"], case["sel0"], case["sel1"], case["pos_sel"],
                                                   case["pos_thresh"], case["neg_thresh"], **kw)
        (pos + neg).backward()
        out.append((pos.detach(), neg.detach(), F0.grad, F1.grad))
    for a, b in zip(*out):
        assert torch.allclose(a, b, rtol=0, atol=1e-14)
    assert float(out[0][0]) > 0 and float(out[0][1]) > 0


def test_loss_restatement_mean_over_no_rows_is_zero():
    """Every candidate a true partner: no kept row on either side, neg_loss 0 with finite (zero) gradients from it."""
    g = torch.Generator().manual_seed(1)
    F0 = torch.randn(6, 4, generator=g, dtype=torch.float64, requires_grad=True)
    F1 = torch.randn(5, 4, generator=g, dtype=torch.float64, requires_grad=True)
    pairs = torch.tensor([[i, j] for i in range(6) for j in range(5)])
    pos, neg, aux = FTR.hardest_contrastive_loss(F0, F1, pairs, torch.arange(6), torch.arange(5))
    assert not aux["keep0"].any() and not aux["keep1"].any() and float(neg.detach()) == 0
    neg.backward()
    assert torch.equal(F0.grad, torch.zeros_like(F0)) and torch.equal(F1.grad, torch.zeros_like(F1))


def test_normalize_eps_restatement():
    y = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1e-3, 0.0]], dtype=torch.float64, requires_grad=True)
    out = FTR.normalize_eps(y)
    assert torch.allclose(out[0], torch.tensor([0.6, 0.8], dtype=torch.float64), atol=1e-8)
    assert torch.equal(out[1], torch.zeros(2, dtype=torch.float64))
    (out * torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=torch.float64)).sum().backward()
    assert torch.isfinite(y.grad).all() and torch.equal(y.grad[1], torch.zeros(2, dtype=torch.float64))
    # d/dy (y / (|y| + e)) along a perpendicular direction: 1 / (|y| + e)
    assert abs(float(y.grad[2, 1]) - 6.0 / (1e-3 + 1e-8)) < 1e-6


def test_fcgf_train_argument_checks_without_device():
    m = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=7, normalize_feature=True, D=3)
    coords = torch.zeros((4, 4), dtype=torch.int32)
    feats = torch.ones((4, 1))
    with pytest.raises(RuntimeError, match=r"eval\(\) mode"):
        T.fcgf_train(m.eval(), coords, feats)
    m.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="autograd is disabled"):
        T.fcgf_train(m, coords, feats)
    with pytest.raises(RuntimeError, match="int32"):
        T.fcgf_train(m, coords.long(), feats)
    with pytest.raises(RuntimeError, match=r"\[M, 1 \+ D\]"):
        T.fcgf_train(m, torch.zeros((4, 8), dtype=torch.int32), feats)
    with pytest.raises(RuntimeError, match="HIP device"):
        T.fcgf_train(m, coords, feats)
    with pytest.raises(RuntimeError, match="fcgf.ResUNetBN2C"):
        T.fcgf_train(gmf_amd.ResUNetBN2C(1, 1, D=3).train(), coords, feats)
    # the module's own forward keeps raising in train()
    with pytest.raises(RuntimeError, match="only the eval-mode forward is built"):
        m(coords, feats)
    with pytest.raises(RuntimeError, match="HIP device"):
        T.normalize_rows_eps(torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        gmf_amd.sparse_conv_narrow_wgrad(None, 0, 0, torch.zeros(4, 1), torch.zeros(4, 32))
    assert callable(gmf_amd.train.fcgf_train) and "sparse_conv_narrow_wgrad" in gmf_amd.__all__


def test_loss_argument_checks_without_device():
    loss = fcgf.hardest_contrastive_loss
    F0, F1 = torch.zeros(6, 8), torch.zeros(5, 8)
    pairs = torch.zeros((3, 2), dtype=torch.int64)
    sel = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="float32"):
        loss(F0.double(), F1, pairs, sel, sel)
    with pytest.raises(RuntimeError, match=r"\[N, C\]"):
        loss(F0.reshape(-1), F1, pairs, sel, sel)
    with pytest.raises(RuntimeError, match="same width"):
        loss(F0, torch.zeros(5, 7), pairs, sel, sel)
    with pytest.raises(NotImplementedError, match="1..64"):
        loss(torch.zeros(6, 65), torch.zeros(5, 65), pairs, sel, sel)
    with pytest.raises(RuntimeError, match="int64"):
        loss(F0, F1, pairs.int(), sel, sel)
    with pytest.raises(RuntimeError, match=r"`positive_pairs` must be \[n, 2\]"):
        loss(F0, F1, torch.zeros((3, 3), dtype=torch.int64), sel, sel)
    with pytest.raises(RuntimeError, match="int64"):
        loss(F0, F1, pairs, sel.int(), sel)
    with pytest.raises(RuntimeError, match=r"`pos_sel` must be \[n\]"):
        loss(F0, F1, pairs, sel, sel, pos_sel=pairs)
    with pytest.raises(RuntimeError, match="at least one candidate"):
        loss(F0, F1, pairs, sel[:0], sel)
    with pytest.raises(RuntimeError, match="HIP device"):
        loss(F0, F1, pairs, sel, sel)


def test_header_lists_the_entry_points():
    with open(os.path.join(ROOT, "include", "gmf_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+GMF_ABI_VERSION\s+5\b", header)          # added entry points: the version stays
    from gmf_amd import _lib
    for name in ("gmf_sparse_conv_narrow_wgrad", "gmf_rownorm_eps", "gmf_hardest_contrastive_forward",
                 "gmf_hardest_contrastive_backward", "gmf_rows_sum_by_dest"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+GMF_STATUS_LOSS_INDEX\s+32\b", header) and _lib.GMF_STATUS_LOSS_INDEX == 32
