"""Host tests of the sparse network's training path (no device): the transposed-map relation the data gradient relies on, the
gradients restated through it against float64 autograd, and the argument checks of the new entry points."""
import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import sparse as SP
from gmf_amd import train as T

import sparse_reference as SR
import sparse_train_reference as STR

NET_MAPS = SP._NET_MAPS


def _coords(M, D, span, batches, seed):
    rng = np.random.default_rng(seed)
    rows = set()
    while len(rows) < M:
        rows.add((int(rng.choice(batches)),) + tuple(int(v) for v in rng.integers(-span, span, D)))
    out = np.array(sorted(rows), dtype=np.int64)
    return out[rng.permutation(M)]


SETS = {"d3": (300, 3, 5, [0, 1, 2], 3), "d6": (250, 6, 2, [0, 1], 4)}


def _sigma(k, o, i, K):
    return (lambda d: K - 1 - d) if o == i else (lambda d: d)


@pytest.mark.parametrize("name", ["d3", "d6"])
def test_transposed_map_is_the_reverse_map_under_sigma(name):
    rows = _coords(*SETS[name])
    D = rows.shape[1] - 1
    lv = SR.build_levels(rows, 4)
    for k, o, i in NET_MAPS:
        K = k ** D
        s = _sigma(k, o, i, K)
        fwd = SR.map_between(lv, k, o, i)
        rev = SR.map_between(lv, k, i, o)
        a = STR.transpose_map(fwd, len(lv[i]))
        # (d, o) pairs of every input row of map (k, o, i), offsets mapped by sigma, equal map (k, i, o)'s pairs
        rp, pairs = a
        mapped = np.stack([np.array([s(int(d)) for d in pairs[:, 0]], dtype=np.int64), pairs[:, 1]], 1)
        rows_of = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        srt = np.lexsort((mapped[:, 0], rows_of))
        assert np.array_equal(rp, rev[0]), (k, o, i)
        assert np.array_equal(mapped[srt], rev[1]), (k, o, i)


@pytest.mark.parametrize("name,m,two", [("d3", 0, False), ("d3", 4, False), ("d3", 8, True), ("d6", 1, False),
                                        ("d6", 9, False), ("d6", 7, True)])
def test_gradients_via_transposed_map_equal_autograd(name, m, two):
    rows = _coords(*SETS[name])
    D = rows.shape[1] - 1
    lv = SR.build_levels(rows, 4)
    k, o, i = NET_MAPS[m]
    K = k ** D
    n_in, n_out = len(lv[i]), len(lv[o])
    g = torch.Generator().manual_seed(m)
    ca, cb, cout = 5, (3 if two else 0), 4
    x = torch.randn(n_in, ca + cb, generator=g, dtype=torch.float64, requires_grad=True)
    W = torch.randn(K, ca + cb, cout, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(n_out, cout, generator=g, dtype=torch.float64)
    fwd = SR.map_between(lv, k, o, i)
    y = SR.conv(x, fwd, W, n_out)
    y.backward(dy)
    # dx: the forward convolution over map (k, i, o) with W'[d] = W[sigma(d)]^T
    s = _sigma(k, o, i, K)
    Wt = torch.stack([W.detach()[s(d)].t() for d in range(K)])
    dx = SR.conv(dy, SR.map_between(lv, k, i, o), Wt, n_in)
    assert torch.allclose(dx, x.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dx[:, :ca], x.grad[:, :ca]) and torch.allclose(dx[:, ca:], x.grad[:, ca:])
    # dW: per-offset sums x[i]^T dy[o]
    rp, pairs = fwd
    orow = np.repeat(np.arange(n_out), np.diff(rp))
    dW = torch.zeros_like(W)
    for d in range(K):
        sel = pairs[:, 0] == d
        if sel.any():
            dW[d] = x.detach()[torch.as_tensor(pairs[sel, 1])].t() @ dy[torch.as_tensor(orow[sel])]
    assert torch.allclose(dW, W.grad, rtol=1e-12, atol=1e-12)


def test_new_entry_points_reject_cpu_tensors():
    x = torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        SP.sparse_conv_wgrad(None, None, 0, x, x)
    model = gmf_amd.ResUNetBN2C(in_channels=1, out_channels=1, D=3).train()
    with pytest.raises(RuntimeError, match="HIP device"):
        T.resunet_train(model, torch.zeros((8, 4), dtype=torch.int32), torch.ones(8, 1),
                        p_tokens=torch.zeros(1, 4, 128), q_tokens=torch.zeros(1, 4, 128))


def test_resunet_train_rejects_eval_mode_and_no_grad():
    model = gmf_amd.ResUNetBN2C(in_channels=1, out_channels=1, D=3)
    tok = torch.zeros(1, 4, 128)
    c = torch.zeros((8, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="eval"):
        T.resunet_train(model.eval(), c, torch.ones(8, 1), p_tokens=tok, q_tokens=tok)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no_grad"):
        T.resunet_train(model.train(), c, torch.ones(8, 1), p_tokens=tok, q_tokens=tok)


def test_forward_in_train_mode_names_resunet_train():
    model = gmf_amd.ResUNetBN2C(in_channels=1, out_channels=1, D=3).train()
    tok = torch.zeros(1, 4, 128)
    with pytest.raises(RuntimeError, match="eval") as e:
        model(torch.zeros((8, 4), dtype=torch.int32), torch.ones(8, 1), p_tokens=tok, q_tokens=tok)
    assert "resunet_train" in str(e.value)


def test_inlier_training_loss_restatement_is_finite_and_differentiable():
    g = torch.Generator().manual_seed(0)
    x0, x1 = torch.randn(50, 3, generator=g, dtype=torch.float64), torch.randn(60, 3, generator=g, dtype=torch.float64)
    pairs = torch.stack([torch.arange(40), torch.randint(0, 60, (40,), generator=g)], 1)
    logits = (2 + torch.randn(40, generator=g, dtype=torch.float64)).requires_grad_(True)
    loss, st = STR.inlier_training_loss(logits, [x0], [x1], [pairs], torch.randint(0, 2, (40,), generator=g),
                                        torch.eye(4, dtype=torch.float64)[None])
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(logits.grad).all()
