"""Host-side checks of the image encoder (no GPU): the weight images of packing.conv_image / packing.stem_image unpacked by the unit
formulas of the kernels' header comments (gmf_amd/csrc/image_kernels.hip), the dispatcher's rules as the GPU tests recompute
them, and the accuracy bound of the split-fp16 activations on a CPU emulation of the arithmetic - so that the bound the GPU
tests assert (image_reference.split_bound) does not rest on the kernels it judges."""
import pytest
import torch

from gmf_amd import packing

import image_reference as R

SCALES = [2.0 ** 9, 1.0, 2.0 ** -4, 2.0 ** -10]


def _assert_planes(hi, lo, W256, what):
    """hi + lo = 256 W to 2^-22 of the largest weight, and element by element to 2^-22 max(|256 w|, 2^-3): hi leaves at most
    2^-11 |x|, lo = fp16 of that keeps it to 2^-11 again while it is a normal fp16 number (|x| >= 2^-3), half a subnormal
    quantum (2^-25 = 2^-22 2^-3) below."""
    err = (hi + lo - W256).abs()
    assert float(err.max()) <= 2.0 ** -22 * float(W256.abs().max()), what
    assert bool((err <= 2.0 ** -22 * W256.abs().clamp_min(2.0 ** -3)).all()), what
    assert bool((hi == W256.float().to(torch.float16).double()).all()), what           # hi is the nearest fp16


@pytest.mark.parametrize("cout,cin,ks,stride,cbt", [(64, 64, 3, 1, True), (128, 128, 3, 1, True), (128, 64, 3, 2, False),
                                                    (128, 64, 1, 2, False)])
def test_conv_image_unpacks_by_the_unit_formula(cout, cin, ks, stride, cbt):
    gen = torch.Generator().manual_seed(cout + cin + ks)
    Wt = torch.randn(cout, cin, ks, ks, generator=gen) / (cin * ks * ks) ** 0.5
    Wt[0, 0, 0, 0], Wt[-1, -1, -1, -1] = 0.75, 2.0 ** -13 * 1.3     # a large weight and one whose lo plane is subnormal
    hi, lo = R.unpack_conv_image(packing.conv_image(Wt, stride), cout, cin, ks, cbt)
    _assert_planes(hi, lo, Wt.double() * 256.0, (cout, cin, ks, stride))
    if ks == 3:
        # the other k order must NOT reproduce the weights: the two orders are told apart by this test
        hi2, lo2 = R.unpack_conv_image(packing.conv_image(Wt, stride), cout, cin, ks, not cbt)
        assert float((hi2 + lo2 - Wt.double() * 256.0).abs().max()) > 1.0


def test_stem_image_unpacks_by_the_unit_formula():
    Wt, _ = R.stem_weights()
    hi, lo = R.unpack_stem_image(packing.stem_image(Wt))
    W256 = torch.zeros(64, 176, dtype=torch.float64)
    for ky in range(7):
        for kx in range(7):
            for c in range(3):
                W256[:, 24 * ky + 3 * kx + c] = Wt[:, c, ky, kx].double() * 256.0
    _assert_planes(hi, lo, W256, "stem")
    # the padded k slots are exactly zero in both planes: three behind each kernel row's 21 values, and k = 168 .. 175
    pad = torch.zeros(176, dtype=torch.bool)
    for ky in range(7):
        pad[24 * ky + 21:24 * ky + 24] = True
    pad[168:] = True
    assert int(pad.sum()) == 29
    assert bool((hi[:, pad] == 0).all()) and bool((lo[:, pad] == 0).all())
    assert bool((hi[:, ~pad] != 0).all())


def test_dispatch_rules_of_the_cases():
    """The counts the GPU cases rely on, recomputed from launch_conv_nhwc_h2 / launch_stem_h2."""
    assert R.conv_workgroups(200, 9, 37, 64, 3, 1) == 521
    assert R.expected_conv_kernel(200, 9, 37, 64, 64, 3, 1) == ("k_conv3x3_patch_h2", (64, 64, 3, 40, False, 3))
    assert R.expected_conv_kernel(205, 8, 41, 64, 64, 3, 1) == ("k_conv3x3_patch_h2", (64, 64, 4, 48, True, 2))
    assert R.expected_conv_kernel(40, 5, 48, 128, 128, 3, 1) == ("k_conv3x3_patch_h2", (128, 128, 4, 48, True, 2))
    assert R.expected_conv_kernel(40, 5, 49, 128, 128, 3, 1) == ("k_conv_nhwc_h2", (128, 128, 3, 1, True))
    assert R.expected_conv_kernel(300, 9, 11, 64, 128, 1, 2) == ("k_conv_nhwc_h2", (64, 128, 1, 2, False))
    for shape in R.CONV_SHAPES:                       # three images of every unit-test shape: the small kernel by default
        assert R.expected_conv_kernel(3, *shape[4:], *shape[:4])[0] == "k_conv_small_h2", shape
        assert R.expected_conv_kernel(3, *shape[4:], *shape[:4], small_grid=0)[0] != "k_conv_small_h2", shape
    assert R.stem_workgroups(8, 125, 131) == 160 and R.expected_stem_kernel(8, 125, 131) == ("k_stem_h2", (8,))
    assert R.expected_stem_kernel(1, 97, 131) == ("k_stem_h2", (4,))
    assert R.stem_out_size(1, 1) == (1, 1) and R.stem_out_size(125, 131) == (32, 33)


def test_kernel_names_parse():
    key = "void gmf::k_conv3x3_patch_h2<64, 64, 3, 40, false, 3>(float const*, float const*, float*, int)"
    assert R.parse_kernel(key) == ("k_conv3x3_patch_h2", (64, 64, 3, 40, False, 3))
    assert R.parse_kernel("void gmf::k_stem_h2<8>(float const*, long)") == ("k_stem_h2", (8,))
    assert R.parse_kernel("gmf::k_conv_nhwc_h2<64, 128, 1, 2, (bool)0>(float const*)") == ("k_conv_nhwc_h2", (64, 128, 1, 2, 0))
    assert R.parse_kernel("gmf::k_bias_relu_nhwc(float*, float const*)") == ("k_bias_relu_nhwc", None)
    assert R.parse_kernel("void at::native::vectorized_elementwise_kernel<4>()") is None


@pytest.mark.parametrize("scale", SCALES)
def test_emulated_split_stays_inside_the_bound(scale):
    """The split-fp16 arithmetic, emulated with fp32 accumulation, meets err <= 4 floor + 2^-25 max_co sum |W[co]| at every
    input scale, for the 64 -> 64 3x3 convolution and for the stem (image_reference, "small-operand bound")."""
    c = R.conv_case(64, 64, 3, 1, 2, 9, 11, seed=64, scale=scale)
    emu = R.emulate_conv(c["x"], c["W"], c["b"], 1, 1)
    err, floor, term = R.maxerr(emu, c["ref"]), R.maxerr(c["f32"], c["ref"]), R.split_bound(c["W"])
    print(f"conv   scale {scale:g}: err {err:.3e} floor {floor:.3e} split term {term:.3e}  err / bound {err / (4 * floor + term):.3f}")
    assert err <= 4.0 * floor + term
    Wt, b = R.stem_weights()
    x = torch.rand(2, 3, 33, 37, generator=torch.Generator().manual_seed(3)) * scale
    bs = b * scale
    ref, f32 = R.stem_ref(x, Wt, bs), R.stem_ref(x, Wt, bs, torch.float32)
    err, floor, term = R.maxerr(R.emulate_stem(x, Wt, bs), ref), R.maxerr(f32, ref), R.split_bound(Wt)
    print(f"stem   scale {scale:g}: err {err:.3e} floor {floor:.3e} split term {term:.3e}  err / bound {err / (4 * floor + term):.3f}")
    assert err <= 4.0 * floor + term


def test_emulation_is_exact_where_the_split_is():
    """Inputs that are fp16 numbers with fp16-exact products lose nothing: the emulation in float64 equals the reference."""
    gen = torch.Generator().manual_seed(9)
    x = torch.randint(-8, 9, (1, 64, 5, 6), generator=gen).float() / 8
    Wt = torch.randint(-8, 9, (64, 64, 3, 3), generator=gen).float() / 64
    b = torch.zeros(64)
    emu = R.emulate_conv(x, Wt, b, 1, 1, acc=torch.float64)
    assert torch.equal(emu, torch.nn.functional.conv2d(x.double(), Wt.double(), None, 1, 1))
