"""GPU test of the library calls the three sparse U-Net forwards issue (gmf_amd.ResUNetBN2C, gmf_amd.fcgf.ResUNetBN2C,
gmf_amd.train.resunet_train): entry points in order, with each convolution's shape, epilogue and offset slices.  The expected
lists below are written out from a run of the forwards as they were before they shared one trunk definition; they are data, not
derived from gmf_amd.sparse.TRUNK."""
import pytest
import torch

import gmf_amd
from gmf_amd import _lib, fcgf
from gmf_amd import train as T

from test_gpu_sparse import _random_coords

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _recorded(monkeypatch):
    """Every Handle.call from here on, in order: the entry point's name, with the arguments that say which layer it is."""
    calls = []
    orig = _lib.Handle.call

    def call(self, name, *a):
        if name == "gmf_sparse_conv":           # K, ca, cb, cout, scale given, residual given, relu, nsplit
            calls.append((name, a[4], a[8], a[10], a[12], a[13] is not None, a[15] is not None, a[16], a[17]))
        elif name == "gmf_sparse_conv_wgrad":   # K, ca, cb, cout
            calls.append((name, a[4], a[7], a[9], a[11]))
        elif name == "gmf_sparse_conv_narrow":  # K, cin, cout
            calls.append((name, a[2], a[6], a[8]))
        elif name == "gmf_sparse_head_l2":      # ca, cb, hid, cout
            calls.append((name, a[3], a[5], a[7], a[9]))
        elif name == "gmf_batchnorm_masked_forward":    # C, residual given, relu
            calls.append((name, a[6], a[1] is not None, a[9]))
        else:
            calls.append(name)
        return orig(self, name, *a)
    monkeypatch.setattr(_lib.Handle, "call", call)
    return calls


def _coords(D):
    span = 6 if D == 3 else 3
    return torch.as_tensor(_random_coords(500, D, span, [0, 1], 31 + D)).to(DEV).int()


def _tokens():
    g = torch.Generator().manual_seed(5)
    return torch.randn(1, 40, 128, generator=g).to(DEV), torch.randn(1, 40, 128, generator=g).to(DEV)


def inlier_calls(monkeypatch, D, k, pe):
    torch.manual_seed(1)
    model = gmf_amd.ResUNetBN2C(1, 1, D=D, conv1_kernel_size=k, pe=pe).to(DEV).eval()
    coords = _coords(D)
    pt, qt = _tokens()
    calls = _recorded(monkeypatch)
    model(coords, torch.ones(len(coords), 1, device=DEV), p_tokens=pt, q_tokens=qt)
    return list(calls)


def fcgf_calls(monkeypatch, k, narrow):
    torch.manual_seed(2)
    model = fcgf.ResUNetBN2C(1, 32, conv1_kernel_size=k, normalize_feature=True, D=3).to(DEV).eval()
    model.narrow_conv1 = narrow
    coords = _coords(3)
    calls = _recorded(monkeypatch)
    model(coords, torch.ones(len(coords), 1, device=DEV))
    return list(calls)


def train_calls(monkeypatch):
    torch.manual_seed(3)
    model = gmf_amd.ResUNetBN2C(1, 1, D=3).to(DEV).train()
    coords = _coords(3)
    pt, qt = _tokens()
    calls = _recorded(monkeypatch)
    out = T.resunet_train(model, coords, torch.ones(len(coords), 1, device=DEV), p_tokens=pt.requires_grad_(True),
                          q_tokens=qt.requires_grad_(True))
    n_forward = len(calls)
    out.sum().backward()
    return list(calls[:n_forward]), list(calls[n_forward:])


# ---- the expected sequences ------------------------------------------------------------------------------------------------

def C(K, ca, cb, cout, scale, residual, relu, nsplit):
    return ("gmf_sparse_conv", K, ca, cb, cout, bool(scale), bool(residual), relu, nsplit)


def B(channels, residual, relu):
    return ("gmf_batchnorm_masked_forward", channels, bool(residual), relu)


def G(K, ca, cb, cout):
    return ("gmf_sparse_conv_wgrad", K, ca, cb, cout)


PLAN, FUSION = "gmf_sparse_build_plan", "gmf_fusion_layer_forward"

# eval, D = 3 (K = 27, every layer in 9 offset slices): block1 .. block4, then conv4_tr .. block2_tr
ENCODER_D3 = [C(27, 32, 0, 32, 1, 0, 1, 9), C(27, 32, 0, 32, 1, 1, 1, 9),
              C(27, 32, 0, 64, 1, 0, 0, 9), C(27, 64, 0, 64, 1, 0, 1, 9), C(27, 64, 0, 64, 1, 1, 1, 9),
              C(27, 64, 0, 128, 1, 0, 0, 9), C(27, 128, 0, 128, 1, 0, 1, 9), C(27, 128, 0, 128, 1, 1, 1, 9),
              C(27, 128, 0, 256, 1, 0, 0, 9), C(27, 256, 0, 256, 1, 0, 1, 9), C(27, 256, 0, 256, 1, 1, 1, 9)]
DECODER_D3 = [C(27, 256, 0, 128, 1, 0, 0, 9), C(27, 128, 0, 128, 1, 0, 1, 9), C(27, 128, 0, 128, 1, 1, 1, 9),
              C(27, 128, 128, 64, 1, 0, 0, 9), C(27, 64, 0, 64, 1, 0, 1, 9), C(27, 64, 0, 64, 1, 1, 1, 9),
              C(27, 64, 64, 64, 1, 0, 0, 9), C(27, 64, 0, 64, 1, 0, 1, 9), C(27, 64, 0, 64, 1, 1, 1, 9)]
INLIER_HEAD = [C(1, 64, 32, 64, 0, 0, 1, 1), C(1, 64, 0, 1, 0, 0, 0, 1)]           # conv1_tr + ReLU, final + bias
FCGF_HEAD = [("gmf_sparse_head_l2", 64, 32, 64, 32)]

# conv1 by kernel size: the identity map (K = 1, one slice), map 0, a map of its own
INLIER_CONV1 = {1: C(1, 1, 0, 32, 1, 0, 0, 1), 3: C(27, 1, 0, 32, 1, 0, 0, 9), 5: C(125, 1, 0, 32, 1, 0, 0, 9)}
FCGF_CONV1 = {(1, True): ("gmf_sparse_conv_narrow", 1, 1, 32), (1, False): C(1, 1, 0, 32, 1, 0, 0, 1),
              (7, True): ("gmf_sparse_conv_narrow", 343, 1, 32), (7, False): C(343, 1, 0, 32, 1, 0, 0, 9)}

# eval, D = 6 (K = 729): the kernels of more than 16 MiB run in 64 .. 256 slices
INLIER_D6 = [PLAN, FUSION,
             C(729, 1, 0, 32, 1, 0, 0, 9), C(729, 32, 0, 32, 1, 0, 1, 9), C(729, 32, 0, 32, 1, 1, 1, 9),
             C(729, 32, 0, 64, 1, 0, 0, 9), C(729, 64, 0, 64, 1, 0, 1, 9), C(729, 64, 0, 64, 1, 1, 1, 9),
             C(729, 64, 0, 128, 1, 0, 0, 128), C(729, 128, 0, 128, 1, 0, 1, 128), C(729, 128, 0, 128, 1, 1, 1, 128),
             C(729, 128, 0, 256, 1, 0, 0, 64), C(729, 256, 0, 256, 1, 0, 1, 64), C(729, 256, 0, 256, 1, 1, 1, 64),
             FUSION,
             C(729, 256, 0, 128, 1, 0, 0, 128), C(729, 128, 0, 128, 1, 0, 1, 128), C(729, 128, 0, 128, 1, 1, 1, 128),
             C(729, 128, 128, 64, 1, 0, 0, 256), C(729, 64, 0, 64, 1, 0, 1, 9), C(729, 64, 0, 64, 1, 1, 1, 9),
             C(729, 64, 64, 64, 1, 0, 0, 256), C(729, 64, 0, 64, 1, 0, 1, 9), C(729, 64, 0, 64, 1, 1, 1, 9),
             C(1, 64, 32, 64, 0, 0, 1, 1), C(1, 64, 0, 1, 0, 0, 0, 1)]

# training, D = 3: one fusion layer's forward and backward (gmf_amd.train._FusionLayerTrain, pe=False)
FUSION_TRAIN = ["gmf_layernorm_forward", "gmf_layernorm_forward", "gmf_gemm_f32", "gmf_gemm_f32", "gmf_gemm_f32", "gmf_softmax_rows",
                "gmf_gemm_f32", "gmf_gemm_f32", "gmf_layernorm_forward", "gmf_gemm_f32", "gmf_geglu", "gmf_gemm_f32"]
FUSION_TRAIN_BACKWARD = ["gmf_gemm_f32", "gmf_colsum", "gmf_gemm_f32", "gmf_geglu", "gmf_gemm_f32", "gmf_colsum", "gmf_gemm_f32",
                         "gmf_colsum", "gmf_layernorm_backward", "gmf_gemm_f32", "gmf_colsum", "gmf_gemm_f32", "gmf_gemm_f32",
                         "gmf_gemm_f32", "gmf_softmax_rows", "gmf_gemm_f32", "gmf_gemm_f32", "gmf_gemm_f32", "gmf_gemm_f32",
                         "gmf_gemm_f32", "gmf_gemm_f32", "gmf_colsum", "gmf_layernorm_backward", "gmf_colsum",
                         "gmf_layernorm_backward"]
BN_BACKWARD = "gmf_batchnorm_masked_backward"
# every convolution plain (no scale, residual or ReLU: they are the BatchNorm's), each followed by its BatchNorm
TRAIN_FORWARD = [PLAN] + FUSION_TRAIN + [
    C(27, 1, 0, 32, 0, 0, 0, 9), B(32, 0, 0), C(27, 32, 0, 32, 0, 0, 0, 9), B(32, 0, 1), C(27, 32, 0, 32, 0, 0, 0, 9), B(32, 1, 1),
    C(27, 32, 0, 64, 0, 0, 0, 9), B(64, 0, 0), C(27, 64, 0, 64, 0, 0, 0, 9), B(64, 0, 1), C(27, 64, 0, 64, 0, 0, 0, 9), B(64, 1, 1),
    C(27, 64, 0, 128, 0, 0, 0, 9), B(128, 0, 0), C(27, 128, 0, 128, 0, 0, 0, 9), B(128, 0, 1),
    C(27, 128, 0, 128, 0, 0, 0, 9), B(128, 1, 1),
    C(27, 128, 0, 256, 0, 0, 0, 9), B(256, 0, 0), C(27, 256, 0, 256, 0, 0, 0, 9), B(256, 0, 1),
    C(27, 256, 0, 256, 0, 0, 0, 9), B(256, 1, 1)] + FUSION_TRAIN + [
    C(27, 256, 0, 128, 0, 0, 0, 9), B(128, 0, 0), C(27, 128, 0, 128, 0, 0, 0, 9), B(128, 0, 1),
    C(27, 128, 0, 128, 0, 0, 0, 9), B(128, 1, 1),
    C(27, 128, 128, 64, 0, 0, 0, 9), B(64, 0, 0), C(27, 64, 0, 64, 0, 0, 0, 9), B(64, 0, 1), C(27, 64, 0, 64, 0, 0, 0, 9), B(64, 1, 1),
    C(27, 64, 64, 64, 0, 0, 0, 9), B(64, 0, 0), C(27, 64, 0, 64, 0, 0, 0, 9), B(64, 0, 1), C(27, 64, 0, 64, 0, 0, 0, 9), B(64, 1, 1),
    C(1, 64, 32, 64, 0, 0, 1, 1), C(1, 64, 0, 1, 0, 0, 0, 1)]
# per convolution, last to first: the weight gradient, then the data gradient (a sparse_conv over the transposed map, Cout -> Cin)
TRAIN_BACKWARD = [
    G(1, 64, 0, 1), "gmf_colsum", C(1, 1, 0, 64, 0, 0, 0, 1), "gmf_relu_backward", G(1, 64, 32, 64), C(1, 64, 0, 96, 0, 0, 0, 1),
    BN_BACKWARD, G(27, 64, 0, 64), C(27, 64, 0, 64, 0, 0, 0, 9), BN_BACKWARD, G(27, 64, 0, 64), C(27, 64, 0, 64, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 64, 64, 64), C(27, 64, 0, 128, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 64, 0, 64), C(27, 64, 0, 64, 0, 0, 0, 9), BN_BACKWARD, G(27, 64, 0, 64), C(27, 64, 0, 64, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 128, 128, 64), C(27, 64, 0, 256, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 128, 0, 128), C(27, 128, 0, 128, 0, 0, 0, 9), BN_BACKWARD, G(27, 128, 0, 128), C(27, 128, 0, 128, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 256, 0, 128), C(27, 128, 0, 256, 0, 0, 0, 9)] + FUSION_TRAIN_BACKWARD + [
    BN_BACKWARD, G(27, 256, 0, 256), C(27, 256, 0, 256, 0, 0, 0, 9), BN_BACKWARD, G(27, 256, 0, 256), C(27, 256, 0, 256, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 128, 0, 256), C(27, 256, 0, 128, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 128, 0, 128), C(27, 128, 0, 128, 0, 0, 0, 9), BN_BACKWARD, G(27, 128, 0, 128), C(27, 128, 0, 128, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 64, 0, 128), C(27, 128, 0, 64, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 64, 0, 64), C(27, 64, 0, 64, 0, 0, 0, 9), BN_BACKWARD, G(27, 64, 0, 64), C(27, 64, 0, 64, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 32, 0, 64), C(27, 64, 0, 32, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 32, 0, 32), C(27, 32, 0, 32, 0, 0, 0, 9), BN_BACKWARD, G(27, 32, 0, 32), C(27, 32, 0, 32, 0, 0, 0, 9),
    BN_BACKWARD, G(27, 1, 0, 32)] + FUSION_TRAIN_BACKWARD


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {i}: {g}, expected {w}"


@pytest.mark.parametrize("k", [1, 3, 5])
def test_inlier_eval_d3_calls(k, monkeypatch):
    _same(inlier_calls(monkeypatch, 3, k, False),
          [PLAN, FUSION, INLIER_CONV1[k]] + ENCODER_D3 + [FUSION] + DECODER_D3 + INLIER_HEAD)


def test_inlier_eval_d6_pe_calls(monkeypatch):
    _same(inlier_calls(monkeypatch, 6, 3, True), INLIER_D6)


@pytest.mark.parametrize("narrow", [True, False])
@pytest.mark.parametrize("k", [1, 7])
def test_fcgf_calls(k, narrow, monkeypatch):
    _same(fcgf_calls(monkeypatch, k, narrow), [PLAN, FCGF_CONV1[(k, narrow)]] + ENCODER_D3 + DECODER_D3 + FCGF_HEAD)


def test_resunet_train_calls(monkeypatch):
    forward, backward = train_calls(monkeypatch)
    _same(forward, TRAIN_FORWARD)
    _same(backward, TRAIN_BACKWARD)
    assert sum(c[0] == "gmf_batchnorm_masked_forward" and c[3] for c in forward) == 14       # the BatchNorms with a ReLU
    gmf_amd.check_status()
