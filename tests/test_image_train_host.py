"""CPU checks behind tests/test_gpu_image_train.py: the new entry points exist in the library, the header and the ctypes table;
the float64 restatements of the kernels' index formulas (image_train_reference.py) equal torch's autograd, so the GPU tests
stand on checked formulas; the max-pool's first-maximum rule is torch's."""
import ctypes
import os
import re

import pytest
import torch

import image_train_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gmf_conv2d_forward_f32", "gmf_conv2d_dgrad", "gmf_conv2d_wgrad", "gmf_maxpool3x3s2_forward",
               "gmf_maxpool3x3s2_backward", "gmf_batchnorm_residual_forward"]


def _header():
    with open(os.path.join(ROOT, "include", "gmf_hip.h")) as f:
        return f.read()


def test_new_symbols_exported_and_declared():
    from gmf_amd import _lib
    header = _header()
    so = os.path.join(ROOT, "gmf_amd", "libgmf_hip.so")
    lib = ctypes.CDLL(so) if os.path.exists(so) else None
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        if lib is not None:
            assert hasattr(lib, name), name
    assert lib is not None, "libgmf_hip.so is not built"


def test_abi_version_stays_5():
    assert re.search(r"#define\s+GMF_ABI_VERSION\s+5\b", _header())


def test_encoder_exposes_native_train():
    import gmf_amd
    from gmf_amd import train
    assert gmf_amd.ImageEncoder.native_train is True
    for name in ("_Conv2dTrain", "_MaxPoolTrain", "_BatchNormTrain", "image_encoder_train"):
        assert hasattr(train, name), name


def test_call_converts_arguments(monkeypatch):
    """train._call with a stub handle: tensor -> data_ptr(), None -> NULL, bool -> 0 / 1, numbers and raw pointers untouched,
    the stream last, the handle taken from the tensor named first."""
    from gmf_amd import train

    class Stub:
        def call(self, *a):
            self.args = a
    stub, asked = Stub(), []
    monkeypatch.setattr(train, "handle_and_stream", lambda t: (asked.append(t), (stub, 77))[1])
    on, t = torch.zeros(3), torch.ones(2, 2)
    raw = t.data_ptr() + 8
    train._call("gmf_name", on, t, None, True, False, 5, 0.25, raw)
    assert len(asked) == 1 and asked[0] is on
    assert stub.args == ("gmf_name", t.data_ptr(), None, 1, 0, 5, 0.25, raw, 77)
    assert [type(a) for a in stub.args[3:8]] == [int, int, int, float, int]


SIZES = {1: [(3, 9, 11)], 2: [(3, 9, 11), (3, 10, 12)]}
STEM_SIZES = [(2, 37, 51), (2, 40, 56)]


@pytest.mark.parametrize("cin,cout,ks,stride", T.CONV_SHAPES)
def test_index_formulas_equal_autograd(cin, cout, ks, stride):
    """dgrad-as-gather and the wgrad sum, float64, against F.conv2d autograd at the odd and even sizes of the GPU tests."""
    for B, H, W in (STEM_SIZES if cin == 3 else SIZES[stride]):
        c = T.conv_train_case(cin, cout, ks, stride, B, H, W, seed=11 * H + W)
        ref = c["ref"]
        dW = T.wgrad_sum(c["x"], c["dy"], ks, stride)
        assert float((dW - ref["dW"]).abs().max()) <= 1e-12 * float(ref["dW"].abs().max()), (H, W)
        dx = T.dgrad_gather(c["dy"], c["W"], H, W, stride)
        assert float((dx - ref["dx"]).abs().max()) <= 1e-12 * float(ref["dx"].abs().max()), (H, W)
        if ks == 1:                      # the input pixels no output reads
            assert float(dx[:, :, 1::2].abs().max()) == 0.0 and float(dx[:, :, :, 1::2].abs().max()) == 0.0


@pytest.mark.parametrize("B,H,W,ties", [(3, 19, 26, False), (2, 20, 28, False), (2, 20, 28, True)])
def test_maxpool_first_maximum_is_torchs_rule(B, H, W, ties):
    x, dy = T.maxpool_case(B, H, W, 8, seed=H + W, ties=ties)
    ref = T.maxpool_autograd(x, dy, torch.float64)
    y, arg = T.maxpool_first_max(x.double())
    assert torch.equal(y, ref["y"])
    assert torch.equal(T.maxpool_backward_gather(x.double(), dy), ref["dx"])
    if ties:
        # output (1, 1): the maximum 5 stands at (1, 2) and (2, 3) - the first wins; output (2, 3): an all-zero window - its first element
        assert bool((y[:, :, 1, 1] == 5).all()) and bool((arg[:, :, 1, 1] == 1 * W + 2).all())
        assert bool((y[:, :, 2, 3] == 0).all()) and bool((arg[:, :, 2, 3] == 3 * W + 5).all())
