"""The image encoder's kernels (gmf_amd/csrc/image_kernels.hip) against torch's float64 operators on the CPU, in every form the
dispatcher can choose, and every case asserts - from the torch profiler's kernel names - that the form it means to test ran:
  k_conv_small_h2        grids below 128 workgroups of the 128-pixel kernels (a few images);
  k_conv_nhwc_h2         the gather kernel, in (tap, cin) order (stride 2, 1x1) and in (channel block, tap) order (stride-1 3x3);
  k_conv3x3_patch_h2     <64, 64, 4, 48, true, 2>, <128, 128, 4, 48, true, 2> and the three-workgroup form <64, 64, 3, 40, false, 3>;
  k_stem_h2<4>, <8>      7x7/2 convolution + bias + ReLU + 3x3/2 max-pool.
Tolerance (image_reference): err < max(4 floor, 4e-6), floor = torch's float32 evaluation against float64; for scaled inputs the
derived bound err <= 4 floor + 2^-25 max_co sum |W[co]|, which test_image_encoder_host.py checks on a CPU emulation.
The tuning knobs change only inside `_knobs`, which restores the defaults; everything runs eagerly (a captured graph keeps the
knobs it was captured with)."""
import contextlib
import copy
import functools

import pytest
import torch

import gmf_amd
from gmf_amd import _lib, packing, synthetic

import image_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def _knobs(small_grid=1, lds_patch=1):
    h = _lib.handle_for(0)
    try:
        h.call("gmf_set_tuning", b"conv_small_grid", small_grid)
        h.call("gmf_set_tuning", b"conv_lds_patch", lds_patch)
        yield h
    finally:
        h.call("gmf_set_tuning", b"conv_lds_patch", 1)
        h.call("gmf_set_tuning", b"conv_small_grid", 1)


def _nhwc(t):
    """[B, C, H, W] on the host -> dense [B, H, W, C] on the device."""
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


GUARD = 1024                                         # floats in front of and behind y
SENTINEL = -7.25


def _run_conv(h, c, xg, wimg, bg, rg, relu):
    """One gmf_conv_nhwc call into the middle of a larger tensor -> ([B, C, Ho, Wo] on the host, the guards kept the sentinel)."""
    B, cin, H, W = c["x"].shape
    cout, ks = c["W"].shape[0], c["W"].shape[2]
    _, _, Ho, Wo = c["ref"].shape
    n = B * Ho * Wo * cout
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    y = buf[GUARD:GUARD + n]
    h.call("gmf_conv_nhwc", xg.data_ptr(), wimg.data_ptr(), bg.data_ptr(), None if rg is None else rg.data_ptr(), y.data_ptr(),
           B, H, W, cin, cout, ks, c["stride"], relu, torch.cuda.current_stream().cuda_stream)
    guards_ok = bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
    return _nchw(y.view(B, Ho, Wo, cout)), guards_ok


@functools.lru_cache(maxsize=None)
def _case(cin, cout, ks, stride, B, H, W, scale=1.0):
    """The seeded case, its references (computed once, shared by every form) and its device tensors."""
    c = R.conv_case(cin, cout, ks, stride, B, H, W, seed=cin + cout + ks + H + 1000 * B, scale=scale)
    c["dev"] = (_nhwc(c["x"]), packing.conv_image(c["W"], stride).to(DEV), c["b"].to(DEV), _nhwc(c["res"]))
    return c


# ---- 2. forced forms at B = 3 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_patch", [1, 2, 0])
@pytest.mark.parametrize("small_grid", [1, 0])
@pytest.mark.parametrize("cin,cout,ks,stride,H,W", R.CONV_SHAPES)
def test_conv_forms_match_fp64(cin, cout, ks, stride, H, W, small_grid, lds_patch):
    """Three images of every layer1 / layer2 shape at odd sizes under all six knob combinations: the K-split kernel, and with
    conv_small_grid = 0 the two-workgroup patch kernel (stride-1 3x3, W <= 48, conv_lds_patch 1 or 2), the gather kernel in
    (channel block, tap) order (the other stride-1 3x3 cases) and in (tap, cin) order (stride 2, 1x1).  A 128-pixel tile spans
    images (7 x 5, 3 x 50, 1 x 1: all three in one tile), P % 128 != 0 everywhere, and every image has taps outside it."""
    B = 3
    c = _case(cin, cout, ks, stride, B, H, W)
    xg, wimg, bg, rg = c["dev"]
    expected = R.expected_conv_kernel(B, H, W, cin, cout, ks, stride, small_grid, lds_patch)
    if not small_grid:                               # the forms the issue names for conv_small_grid = 0
        if ks == 3 and stride == 1 and W <= 48 and lds_patch:
            assert expected == ("k_conv3x3_patch_h2", (cin, cin, 4, 48, True, 2))
        else:
            assert expected == ("k_conv_nhwc_h2", (cin, cout, ks, stride, ks == 3 and stride == 1))
    else:
        assert expected[0] == "k_conv_small_h2"
    with _knobs(small_grid, lds_patch) as h:
        outs, names = R.launched(lambda: [_run_conv(h, c, xg, wimg, bg, rg if with_res else None, relu)
                                          for with_res, relu in ((False, 0), (True, 1))])
    R.assert_ran(names, expected, count=2)
    for (y, guards_ok), (with_res, relu) in zip(outs, ((False, 0), (True, 1))):
        want, floor = R.conv_want(c, with_res, relu)
        err = R.maxerr(y, want)
        print(f"{expected}: residual {with_res} relu {relu}: err {err:.3e} floor {floor:.3e}")
        assert guards_ok
        assert err < max(4.0 * floor, 4e-6), (err, floor)


# ---- 3. default dispatch on grids of 128 workgroups or more ------------------------------------------------------------------------
PATCH3 = ("k_conv3x3_patch_h2", (64, 64, 3, 40, False, 3))
PATCH2 = ("k_conv3x3_patch_h2", (64, 64, 4, 48, True, 2))
PATCH128 = ("k_conv3x3_patch_h2", (128, 128, 4, 48, True, 2))
LARGE = [  # cin, cout, ks, stride, H, W, B, expected kernel, also with residual and ReLU off
    (64, 64, 3, 1, 9, 37, 200, PATCH3, True),        # 66 600 pixels: 521 workgroups, W <= 40
    (64, 64, 3, 1, 8, 41, 205, PATCH2, False),       # 526 workgroups, but W > 40
    (64, 64, 3, 1, 3, 48, 120, PATCH2, False),       # 135 full workgroups, the widest patch
    (64, 64, 3, 1, 3, 48, 121, PATCH2, False),       # ... and with a partial last one
    (64, 64, 3, 1, 3, 49, 120, ("k_conv_nhwc_h2", (64, 64, 3, 1, True)), True),
    (128, 128, 3, 1, 5, 48, 40, PATCH128, False),    # 75 x 2 full workgroups
    (128, 128, 3, 1, 5, 48, 41, PATCH128, False),    # 77 x 2, the last pair partial
    (128, 128, 3, 1, 5, 49, 40, ("k_conv_nhwc_h2", (128, 128, 3, 1, True)), False),
    (64, 128, 3, 2, 9, 11, 300, ("k_conv_nhwc_h2", (64, 128, 3, 2, False)), False),     # 5 x 6 outputs: 71 x 2 workgroups
    (64, 128, 1, 2, 9, 11, 300, ("k_conv_nhwc_h2", (64, 128, 1, 2, False)), False),
]


@pytest.mark.parametrize("cin,cout,ks,stride,H,W,B,expected,also_plain", LARGE)
def test_conv_default_dispatch_on_large_grids(cin, cout, ks, stride, H, W, B, expected, also_plain):
    """No knob touched: many tiny images, so that the grid has at least 128 workgroups, every 128-pixel tile spans several images
    (and, in the patch kernels, its input range starts and ends in other images), and the last tile is partial (except at
    120 images of 3 x 48 and 40 of 5 x 48, which fill their tiles: each has a neighbour with one image more).  All pixels
    against float64; the elements around y keep their sentinel."""
    P = B * R.conv_out_size(H, W, ks, stride)[0] * R.conv_out_size(H, W, ks, stride)[1]
    assert R.conv_workgroups(B, H, W, cout, ks, stride) >= 128 and (P % 128 != 0 or (W, B) in ((48, 120), (48, 40)))
    assert R.expected_conv_kernel(B, H, W, cin, cout, ks, stride) == expected
    c = _case(cin, cout, ks, stride, B, H, W)
    xg, wimg, bg, rg = c["dev"]
    h = _lib.handle_for(0)
    for with_res, relu in ((True, 1), (False, 0)) if also_plain else ((True, 1),):
        (y, guards_ok), names = R.launched(lambda: _run_conv(h, c, xg, wimg, bg, rg if with_res else None, relu))
        R.assert_ran(names, expected)
        want, floor = R.conv_want(c, with_res, relu)
        err = R.maxerr(y, want)
        print(f"{expected} B={B} {H}x{W}: residual {with_res} relu {relu}: err {err:.3e} floor {floor:.3e}")
        assert guards_ok
        assert err < max(4.0 * floor, 4e-6), (err, floor)


# ---- 4. the stem ------------------------------------------------------------------------------------------------------------------
STEM_SIZES = [(1, 1, 1), (2, 2, 3), (1, 5, 7), (2, 31, 33), (1, 32, 32), (1, 33, 65), (1, 97, 131), (3, 64, 17), (8, 125, 131)]


@functools.lru_cache(maxsize=None)
def _stem_dev():
    Wt, b = R.stem_weights()
    return Wt, b, packing.stem_image(Wt).to(DEV), b.to(DEV)


def _run_stem(h, xg, wimg, bg):
    """gmf_stem_forward on a device view of any strides -> [B, 64, Hp, Wp] on the host, guards intact."""
    B, _, H, W = xg.shape
    Hp, Wp = R.stem_out_size(H, W)
    n = B * Hp * Wp * 64
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    y = buf[GUARD:GUARD + n]
    h.call("gmf_stem_forward", xg.data_ptr(), xg.stride(0), xg.stride(1), xg.stride(2), xg.stride(3), wimg.data_ptr(),
           bg.data_ptr(), y.data_ptr(), B, H, W, torch.cuda.current_stream().cuda_stream)
    guards_ok = bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
    return _nchw(y.view(B, Hp, Wp, 64)), guards_ok


def _stem_images(B, H, W):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(1000 * B + 10 * H + W))


@pytest.mark.parametrize("B,H,W", STEM_SIZES)
def test_stem_matches_fp64(B, H, W):
    """Both forms of the stem against max_pool2d(relu(conv2d(x, w, b, 2, 3)), 3, 2, 1) in float64: odd H and W with odd Hc / Wc,
    pool windows cut by the right and bottom edges (97 x 131: Hc = 49, Wc = 66; 125 x 131: Hc = 63), images smaller than one
    tile of either form, images in [0, 1] and in [-0.5, 0.5], channels the ReLU zeroes entirely."""
    Wt, b, wimg, bg = _stem_dev()
    grids = (1, 0) if R.stem_workgroups(B, H, W) < 128 else (1,)
    if (B, H, W) == (8, 125, 131):
        assert R.stem_workgroups(B, H, W) == 160 and R.stem_out_size(H, W) == (32, 33)    # partial 8 x 8 tiles on the right edge
    img = _stem_images(B, H, W)
    for x in (img, img - 0.5):
        ref, f32 = R.stem_ref(x, Wt, b), R.stem_ref(x, Wt, b, torch.float32)
        floor = R.maxerr(f32, ref)
        dead = (ref.amax((0, 2, 3)) == 0)
        assert 0 < int(dead.sum()) < 64                # some channels are zero everywhere, the others are not
        xg = x.to(DEV)
        for small_grid in grids:
            expected = R.expected_stem_kernel(B, H, W, small_grid)
            assert expected[1] == ((4,) if small_grid and len(grids) == 2 else (8,))
            with _knobs(small_grid) as h:
                (y, guards_ok), names = R.launched(lambda: _run_stem(h, xg, wimg, bg))
            R.assert_ran(names, expected)
            assert y.shape == ref.shape
            err = R.maxerr(y, ref)
            print(f"k_stem_h2<{expected[1][0]}> {B}x{H}x{W}: err {err:.3e} floor {floor:.3e}")
            assert guards_ok
            assert err < max(4.0 * floor, 4e-6), (err, floor)


@pytest.mark.parametrize("layout", ["nchw", "channels_last", "width_slice"])
def test_stem_reads_through_strides(layout):
    """The stem reads x[b, c, y, x] through the four element strides it is given: NCHW-contiguous, a channels-last view, and a
    width-sliced view with a storage offset - the same values each time, so the same float64 reference."""
    Wt, b, wimg, bg = _stem_dev()
    B, H, W = 2, 31, 33
    x = _stem_images(B, H, W)
    ref, f32 = R.stem_ref(x, Wt, b), R.stem_ref(x, Wt, b, torch.float32)
    floor = R.maxerr(f32, ref)
    if layout == "nchw":
        xg = x.to(DEV).contiguous()
        assert xg.stride() == (3 * H * W, H * W, W, 1)
    elif layout == "channels_last":
        xg = x.to(DEV).contiguous(memory_format=torch.channels_last)
        assert xg.stride() == (3 * H * W, 1, 3 * W, 3)
    else:
        big = torch.full((B, 3, H, W + 12), 1e3, device=DEV)       # a misread neighbour would be off by hundreds
        big[..., 5:5 + W] = x.to(DEV)
        xg = big[..., 5:5 + W]
        assert xg.storage_offset() == 5 and xg.stride() == (3 * H * (W + 12), H * (W + 12), W + 12, 1)
    for small_grid in (1, 0):
        with _knobs(small_grid) as h:
            (y, guards_ok), names = R.launched(lambda: _run_stem(h, xg, wimg, bg))
        R.assert_ran(names, R.expected_stem_kernel(B, H, W, small_grid))
        err = R.maxerr(y, ref)
        assert guards_ok and y.shape == ref.shape
        assert err < max(4.0 * floor, 4e-6), (layout, err, floor)


# ---- 5. small-magnitude operands -----------------------------------------------------------------------------------------------------
SCALES = [2.0 ** 9, 1.0, 2.0 ** -4, 2.0 ** -10]


@pytest.mark.parametrize("scale", SCALES)
def test_conv_small_operands_meet_the_split_bound(scale):
    """64 -> 64 3x3 with input, bias and residual scaled by s: err <= 4 floor + 2^-25 max_co sum |W[co]| in the K-split, the
    patch and the gather kernel.  A denormal flush of the lo plane (in the conversion, in LDS or in the MFMA) would leave
    2^-12 |x| per element instead of 2^-25: at s = 2^-10 about 40 times the bound."""
    cin = cout = 64
    B, H, W = 2, 9, 11
    c = _case(cin, cout, 3, 1, B, H, W, scale)
    xg, wimg, bg, rg = c["dev"]
    term = R.split_bound(c["W"])
    for form, (small_grid, lds_patch) in (("small", (1, 1)), ("patch", (0, 1)), ("gather", (0, 0))):
        with _knobs(small_grid, lds_patch) as h:
            (y, guards_ok), names = R.launched(lambda: _run_conv(h, c, xg, wimg, bg, None, 0))
        R.assert_ran(names, R.expected_conv_kernel(B, H, W, cin, cout, 3, 1, small_grid, lds_patch))
        want, floor = R.conv_want(c, False, 0)
        err = R.maxerr(y, want)
        print(f"conv {form} scale {scale:g}: err {err:.3e} floor {floor:.3e} split term {term:.3e}: err / bound {err / (4.0 * floor + term):.3f}, err / term {err / term:.3f}")
        assert guards_ok
        assert err <= 4.0 * floor + term, (form, scale, err, floor, term)


@pytest.mark.parametrize("scale", SCALES)
def test_stem_small_operands_meet_the_split_bound(scale):
    """The stem on images (and a bias) scaled by s, both forms, same bound."""
    Wt, b, wimg, _ = _stem_dev()
    B, H, W = 2, 33, 37
    x = _stem_images(B, H, W) * scale
    bs = b * scale
    ref, f32 = R.stem_ref(x, Wt, bs), R.stem_ref(x, Wt, bs, torch.float32)
    floor, term = R.maxerr(f32, ref), R.split_bound(Wt)
    xg, bg = x.to(DEV), bs.to(DEV)
    for small_grid in (1, 0):
        with _knobs(small_grid) as h:
            (y, guards_ok), names = R.launched(lambda: _run_stem(h, xg, wimg, bg))
        expected = R.expected_stem_kernel(B, H, W, small_grid)
        R.assert_ran(names, expected)
        err = R.maxerr(y, ref)
        print(f"stem <{expected[1][0]}> scale {scale:g}: err {err:.3e} floor {floor:.3e} split term {term:.3e}: err / bound {err / (4.0 * floor + term):.3f}, err / term {err / term:.3f}")
        assert guards_ok
        assert err <= 4.0 * floor + term, (small_grid, scale, err, floor, term)


# ---- 7. the whole encoder at sizes that are no multiples of 8 ----------------------------------------------------------------------------
IMAGE_SEED = 111                                     # the seed of golden F11 / F15, which test_gpu_parity's _image_model loads


@functools.lru_cache(maxsize=None)
def _encoder():
    enc = gmf_amd.ImageEncoder()
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict(synthetic.seeded_state_dict(shapes, seed=IMAGE_SEED, gain=1.0))
    stock = copy.deepcopy(enc.backbone).double().eval()
    return enc.to(DEV).eval(), stock


@pytest.mark.parametrize("shape", [(2, 3, 97, 131), (1, 3, 50, 70)])
def test_encoder_matches_stock_backbone_in_fp64(shape):
    """_FusedResNet, eager, against the stock ResNet-34 -> layer2 modules in float64 on the CPU, within 1e-4 of the largest token
    (golden F11's rule); the output shape is the stock module's (13 x 17 and 7 x 9: not (H // 8) x (W // 8))."""
    enc, stock = _encoder()
    img = synthetic.seeded_images(*shape[:1], *shape[2:])
    with torch.no_grad():
        ref = stock(img.double())
    assert ref.shape[2:] != (shape[2] // 8, shape[3] // 8)
    fused = enc.fused()
    with torch.no_grad():
        out, names = R.launched(lambda: fused(img.to(DEV)))
    assert out.shape == ref.shape
    ran = {k[0] for k in names}
    assert {"k_stem_h2", "k_conv_small_h2"} <= ran and sum(names.values()) == 16, dict(names)     # the stem and 15 convolutions
    scale = max(1.0, float(ref.abs().max()))
    err = R.maxerr(out.cpu(), ref)
    print(f"encoder {shape}: err {err:.3e}, largest token {scale:.2f}")
    assert err < 1e-4 * scale


def test_graphed_encoder_over_ten_shapes_equals_eager():
    """ImageEncoder's graph cache holds at most nine shapes and is cleared beyond: ten distinct shapes, then the first again
    (captured a second time) - every result is the eager result of its shape, bit for bit."""
    enc, _ = _encoder()
    shapes = [(1 + i % 2, 3, 17 + 8 * i, 40 - 3 * i) for i in range(10)]
    assert len(set(shapes)) == 10
    fused = enc.fused()
    try:
        enc.__dict__.pop("_graphs", None)
        for n, _, H, W in shapes + shapes[:1]:
            img = synthetic.seeded_images(n, H, W).to(DEV)
            enc.graph = False
            with torch.no_grad():
                eager = enc(img).clone()
                assert torch.equal(eager, fused(img))
                enc.graph = True
                graphed = enc(img)
                replay = enc(img)
            assert enc.__dict__["_graphs"][(tuple(img.shape), tuple(img.stride()), img.device, enc._fused_version)] is not False
            assert torch.equal(graphed, eager) and torch.equal(replay, eager), (n, H, W)
            assert len(enc.__dict__["_graphs"]) <= 9
        assert len(enc.__dict__["_graphs"]) == 2      # cleared at the tenth shape; the first came back after it
    finally:
        enc.__dict__.pop("_graphs", None)
        if "graph" in enc.__dict__:
            del enc.__dict__["graph"]
    gmf_amd.check_status()
