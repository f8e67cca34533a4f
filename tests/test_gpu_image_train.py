"""The image encoder's training kernels (gmf_amd/csrc/image_train_kernels.hip) and the train-mode ImageEncoder built from them,
entry by entry against torch autograd in float64 on the CPU.  Tolerance: `check_close` of tests/test_train_gradients.py,
|hip - ref64| <= max(4 floor, 2e-5 max|ref64|) + 3e-6 gmax, floor = the same computation in float32 on the CPU.  Every case
asserts from the profiler's kernel names that the kernels it means to test ran; outputs are written into NaN-filled buffers
between sentinel guards."""
import copy
import functools

import pytest
import torch

import gmf_amd
from gmf_amd import _lib, synthetic
from gmf_amd import train as TR
from oracle import gmf_oracle as O

import image_reference as R
import image_train_reference as T
from test_train_gradients import check_close, LAYERS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 1024, -7.25
IMAGE_SEED = 4242


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n):
    """A NaN-filled buffer of n floats between two sentinel guards -> (whole buffer, the n floats)."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n]


def _guards_ok(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _nchw(t, B, H, W):
    return t.view(B, H, W, -1).permute(0, 3, 1, 2).cpu()


def _names(names):
    return {k[0] for k in names}


def _report(rep):
    worst = max(rep.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print(f"worst err / tol: {worst[0]}: {worst[1][0]:.3e} / {worst[1][1]:.3e} = {worst[1][0] / worst[1][1]:.3f}")


# ---- 1. each convolution shape, each pass ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_case(cin, cout, ks, stride, B, H, W):
    return T.conv_train_case(cin, cout, ks, stride, B, H, W, seed=cin + cout + 7 * ks + H + 1000 * B + W)


def _conv_passes(c, x_dev, strides, with_dgrad):
    """forward, wgrad and (layer shapes) dgrad with and without dx_add through the C ABI -> ({name: result}, kernel names)."""
    B, cin, H, W = c["x"].shape
    cout, ks = c["W"].shape[0], c["W"].shape[2]
    st, Ho, Wo = c["stride"], c["Ho"], c["Wo"]
    h = _lib.handle_for(0)
    wg, dyg = c["W"].to(DEV), _nhwc(c["dy"])
    geom = (B, H, W, cin, cout, ks, st)
    got, bufs = {}, []

    def run():
        ny, nx, nw = B * Ho * Wo * cout, B * H * W * cin, c["W"].numel()
        by, y = _guarded(ny)
        h.call("gmf_conv2d_forward_f32", x_dev.data_ptr(), *strides, wg.data_ptr(), y.data_ptr(), *geom, _stream())
        bw, dw = _guarded(nw)
        h.call("gmf_conv2d_wgrad", x_dev.data_ptr(), *strides, dyg.data_ptr(), dw.data_ptr(), *geom, _stream())
        got["y"], got["dW"] = _nchw(y, B, Ho, Wo), dw.view(c["W"].shape).cpu()
        bufs.extend([(by, ny), (bw, nw)])
        if with_dgrad:
            addg = _nhwc(c["dx_add"])
            for key, add in (("dx", None), ("dx_added", addg)):
                bx, dx = _guarded(nx)
                h.call("gmf_conv2d_dgrad", dyg.data_ptr(), wg.data_ptr(), None if add is None else add.data_ptr(), dx.data_ptr(),
                       *geom, _stream())
                got[key] = _nchw(dx, B, H, W)
                bufs.append((bx, nx))
    _, names = R.launched(run)
    assert all(_guards_ok(b, n) for b, n in bufs)
    return got, names


def _check_conv(c, got):
    ref = {k: c["ref"][k] for k in got}
    assert not any(bool(torch.isnan(v).any()) for v in got.values()), "an output entry was not written"
    for k in got:                                # each tensor is its own group: gmax = its own largest entry
        _report(check_close({k: got[k]}, {k: ref[k]}, {k: c["f32"][k]}, what=f"conv {k}: "))


LAYER_CASES = [(64, 64, 3, 1, 3, 9, 11), (128, 128, 3, 1, 3, 9, 11),
               (64, 128, 3, 2, 3, 9, 11), (64, 128, 3, 2, 3, 10, 12), (64, 128, 1, 2, 3, 9, 11), (64, 128, 1, 2, 3, 10, 12)]
BIG_CASES = [(64, 64, 3, 1, 5, 30, 40), (128, 128, 3, 1, 5, 30, 40), (64, 128, 3, 2, 5, 30, 40)]


@pytest.mark.parametrize("cin,cout,ks,stride,B,H,W", LAYER_CASES + BIG_CASES)
def test_conv_passes_match_fp64(cin, cout, ks, stride, B, H, W):
    """Forward, dgrad (with and without dx_add) and wgrad of the four layer shapes: 3 images of 9 x 11 (297 pixels: no multiple
    of a tile, border taps on all four sides), the stride-2 shapes also at 10 x 12 (other last rows, other dx entries without a
    tap), and 5 images of 30 x 40 where the wgrad runs several pixel chunks and forward / dgrad several workgroups."""
    c = _conv_case(cin, cout, ks, stride, B, H, W)
    got, names = _conv_passes(c, _nhwc(c["x"]), (H * W * cin, 1, W * cin, cin), True)
    assert names[("k_conv2d_f32", (cin, cout, ks, stride, False))] == 1, dict(names)
    assert names[("k_conv2d_f32", (cout, cin, ks, stride, True))] == 2, dict(names)
    assert names[("k_conv2d_wgrad", (cin, cout, ks, stride))] == 1, dict(names)
    assert _names(names) == {"k_conv2d_f32", "k_conv2d_wgrad", "k_conv_wgrad_reduce", "k_conv_wperm"}, dict(names)
    P_out, P_in = B * c["Ho"] * c["Wo"], B * H * W
    if (B, H, W) == (5, 30, 40):
        assert T.wgrad_slabs(cin, cout, ks, P_out) > 1
        assert T.conv_workgroups(P_out, cout) > 1 and T.conv_workgroups(P_in, cin) > 1
    _check_conv(c, got)
    if ks == 1:                                  # the input pixels no output reads: exactly 0, and exactly dx_add
        assert float(got["dx"][:, :, 1::2].abs().max()) == 0.0 and float(got["dx"][:, :, :, 1::2].abs().max()) == 0.0
        assert torch.equal(got["dx_added"][:, :, 1::2], c["dx_add"][:, :, 1::2])


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("B,H,W", [(2, 37, 51), (2, 40, 56)])
def test_stem_passes_match_fp64(B, H, W, layout):
    """Forward and wgrad of the 3 -> 64 7x7 stride-2 stem, the image read through its strides: NCHW and a channels-last view."""
    c = _conv_case(3, 64, 7, 2, B, H, W)
    x = c["x"].to(DEV)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    assert x.is_contiguous() == (layout == "nchw")
    got, names = _conv_passes(c, x, tuple(x.stride()), False)
    assert _names(names) == {"k_stem_f32", "k_stem_wgrad", "k_conv_wgrad_reduce", "k_conv_wperm"}, dict(names)
    assert T.wgrad_slabs(3, 64, 7, B * c["Ho"] * c["Wo"]) > 1
    _check_conv(c, got)


# ---- 2. max-pool --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,ties", [(3, 19, 26, False), (2, 20, 28, False), (2, 20, 28, True)])
def test_maxpool_matches_fp64(B, H, W, ties):
    """Forward and backward against F.max_pool2d autograd in float64 on the CPU; with planted ties (two equal positive maxima in
    one window, an all-zero window) the gradient lands where torch's CPU backward puts it."""
    x, dy = T.maxpool_case(B, H, W, 64, seed=H + W, ties=ties)
    ref, f32 = T.maxpool_autograd(x, dy, torch.float64), T.maxpool_autograd(x, dy, torch.float32)
    Hp, Wp = ref["y"].shape[2:]
    xg, dyg = _nhwc(x), _nhwc(dy)
    h = _lib.handle_for(0)
    by, y = _guarded(B * Hp * Wp * 64)
    bx, dx = _guarded(B * H * W * 64)

    def run():
        h.call("gmf_maxpool3x3s2_forward", xg.data_ptr(), y.data_ptr(), B, H, W, 64, _stream())
        h.call("gmf_maxpool3x3s2_backward", xg.data_ptr(), dyg.data_ptr(), dx.data_ptr(), B, H, W, 64, _stream())
    _, names = R.launched(run)
    assert _names(names) == {"k_maxpool_fwd", "k_maxpool_bwd"}, dict(names)
    assert _guards_ok(by, y.numel()) and _guards_ok(bx, dx.numel())
    got = {"y": _nchw(y, B, Hp, Wp), "dx": _nchw(dx, B, H, W)}
    assert torch.equal(got["y"].double(), ref["y"])                        # a maximum is exact
    for k in got:
        check_close({k: got[k]}, {k: ref[k]}, {k: f32[k]}, what=f"maxpool {k}: ")
    if ties:
        assert torch.equal((got["dx"] != 0), (ref["dx"] != 0))


# ---- 3. residual BatchNorm + ReLU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,relu", [pytest.param(64, True, id="64"), pytest.param(128, True, id="128"),
                                    pytest.param(64, False, id="64-norelu"), pytest.param(128, False, id="128-norelu")])
def test_batchnorm_residual_matches_fp64(C, relu):
    """relu?(bn(x) + identity) in training mode at 297 rows, forward and backward, running statistics included: the residual
    instance of k_bn_apply and not the plain one; without the ReLU no k_relu_bwd, and the residual's gradient is dy's bits."""
    c = T.bn_residual_case(297, C, seed=C)
    ref, f32 = T.bn_residual_autograd(c, torch.float64, relu), T.bn_residual_autograd(c, torch.float32, relu)
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]); bn.bias.copy_(c["beta"]); bn.running_mean.copy_(c["rm"]); bn.running_var.copy_(c["rv"])
    bn = bn.to(DEV).train()
    x, res = c["x"].to(DEV).requires_grad_(True), c["res"].to(DEV).requires_grad_(True)

    def run():
        y = TR.batchnorm_train(x, bn, relu=relu, residual=res)
        y.backward(c["dy"].to(DEV))
        return y
    y, names = R.launched(run)
    assert ("k_bn_apply", (True,)) in names and ("k_bn_apply", (False,)) not in names, dict(names)
    assert "k_bn_bwd" in _names(names) and ("k_relu_bwd" in _names(names)) == relu, dict(names)
    if not relu:
        assert torch.equal(res.grad, c["dy"].to(DEV))
    got ={"y": y.detach(), "dx": x.grad, "dres": res.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    for k in got:
        _report(check_close({k: got[k]}, {k: ref[k]}, {k: f32[k]}, what=f"bn residual C={C} {k}: "))
    assert int(bn.num_batches_tracked) == 1


# ---- 4-6. the whole encoder in train() ----------------------------------------------------------------------------------------------
def _encoder():
    enc = gmf_amd.ImageEncoder()
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict(synthetic.seeded_state_dict(shapes, seed=IMAGE_SEED, gain=1.0))
    return enc


def _images_and_projections(enc, shape):
    B, _, H, W = shape
    imgs = synthetic.seeded_images(2 * B, H, W)
    images = [imgs[:B], imgs[B:]]
    with torch.no_grad():
        out_shape = copy.deepcopy(enc.backbone).eval()(images[0]).shape
    gen = torch.Generator().manual_seed(H * W)
    return images, [torch.randn(out_shape, generator=gen) for _ in images]


@functools.lru_cache(maxsize=None)
def _encoder_reference(shape):
    enc = _encoder()
    images, projs = _images_and_projections(enc, shape)
    return (images, projs, T.stock_encoder_step(enc.backbone, images, projs, torch.float64),
            T.stock_encoder_step(enc.backbone, images, projs, torch.float32))


def _all_kernels(fn):
    """(fn(), every device kernel's name) from the torch profiler."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.key for e in prof.key_averages() if e.device_time_total > 0]


def _hip_encoder_step(shape, images, projs):
    enc = _encoder().to(DEV).train()
    outs = {}
    loss = 0
    for n, (img, proj) in enumerate(zip(images, projs)):
        y = enc(img.to(DEV))
        outs[f"out{n}"] = y.detach()
        loss = loss + (y * proj.to(DEV)).sum()
    loss.backward()
    grads = {k: p.grad for k, p in enc.backbone.named_parameters()}
    stats = {k: v.detach().clone() for k, v in enc.backbone.state_dict().items() if "running" in k or "num_batches" in k}
    return outs, grads, stats


ENCODER_SHAPES = [(2, 3, 37, 51), (3, 3, 64, 80)]


@pytest.mark.parametrize("shape", ENCODER_SHAPES)
def test_encoder_train_matches_stock_backbone_fp64(shape):
    """Two calls (p and q images), loss = a fixed random projection of both outputs: both outputs, all 48 parameter gradients,
    every running mean and variance against the stock backbone in float64, num_batches_tracked advanced by 2, and - from the profiler -
    no MIOpen / aten convolution, pooling or batch-norm kernel: the new kernels ran instead."""
    images, projs, (o64, g64, s64), (o32, g32, s32) = _encoder_reference(shape)
    (outs, grads, stats), keys = _all_kernels(lambda: _hip_encoder_step(shape, images, projs))
    ours = {R.parse_kernel(k)[0] for k in keys if R.parse_kernel(k)}
    foreign = [k for k in keys if not R.parse_kernel(k)]
    bad = [k for k in foreign if any(w in k.lower() for w in ("miopen", "conv", "pool", "batch_norm", "batchnorm", "gemm", "cijk"))]
    assert not bad, bad
    for name in ("k_stem_f32", "k_stem_wgrad", "k_conv2d_f32", "k_conv2d_wgrad", "k_conv_wgrad_reduce", "k_maxpool_fwd",
                 "k_maxpool_bwd", "k_bn_apply", "k_bn_bwd"):
        assert name in ours, (name, sorted(ours))
    instances = {R.parse_kernel(k) for k in keys if R.parse_kernel(k)}
    assert {("k_bn_apply", (True,)), ("k_bn_apply", (False,))} <= instances, sorted(instances, key=str)
    assert len(g64) == 48
    assert o64["out0"].shape == outs["out0"].shape
    _report(check_close(outs, o64, o32, what="output "))
    _report(check_close(grads, g64, g32, what="grad "))
    run64 = {k: v for k, v in s64.items() if "running" in k}
    _report(check_close(stats, run64, {k: s32[k] for k in run64}, what="stat "))
    before = _encoder().backbone.state_dict()          # (the seeded state starts every counter above zero)
    for k, v in stats.items():
        if "num_batches" in k:
            assert int(v) == int(before[k]) + 2 == int(s64[k]), k


def test_encoder_train_is_deterministic():
    images, projs, _, _ = _encoder_reference(ENCODER_SHAPES[0])
    a = _hip_encoder_step(ENCODER_SHAPES[0], images, projs)
    b = _hip_encoder_step(ENCODER_SHAPES[0], images, projs)
    for part_a, part_b in zip(a, b):
        for k in part_a:
            assert torch.equal(part_a[k], part_b[k]), k


def test_encoder_train_captures_in_a_graph():
    """Forward + backward of the (2, 3, 37, 51) case under torch.cuda.graph after two eager warm-ups: the replay equals the eager
    result bit for bit (no host read, no allocation outside torch's allocator and the workspace in the pass)."""
    shape = ENCODER_SHAPES[0]
    images, projs, _, _ = _encoder_reference(shape)
    eager_out, eager_grads, _ = _hip_encoder_step(shape, images[:1], projs[:1])
    enc = _encoder().to(DEV).train()
    img, proj = images[0].to(DEV), projs[0].to(DEV)

    def step():
        enc.zero_grad(set_to_none=True)
        y = enc(img)
        (y * proj).sum().backward()
        return y
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    enc.zero_grad(set_to_none=True)
    with torch.cuda.graph(g):
        y = step()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager_out["out0"])
    for k, p in enc.backbone.named_parameters():
        assert torch.equal(p.grad, eager_grads[k]), k


# ---- 7. the training step from raw images -------------------------------------------------------------------------------------------
def _step_inputs():
    B, N = 2, 256
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, LAYERS, 128), seed=7)
    b = synthetic.synthetic_batch([300 + i for i in range(B)], N=N, T=40)
    imgs = synthetic.seeded_images(2 * B, 64, 80)
    return sd, b, imgs[:B], imgs[B:]


def _oracle_image_step(sd, b, p_img, q_img, backbone, dtype):
    """The stock backbone in `dtype` on the CPU feeding oracle.training_losses (test_train_gradients.oracle_step, from images)."""
    bb = copy.deepcopy(backbone).to("cpu", dtype).train()
    sdx = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    data = {k: b[k].to(dtype) for k in ("corr_pos", "src_keypts", "tgt_keypts", "gt_labels")}
    data["p_tokens"] = bb(p_img.to(dtype)).flatten(2).permute(0, 2, 1)
    data["q_tokens"] = bb(q_img.to(dtype)).flatten(2).permute(0, 2, 1)
    _, _, cl, sm = O.training_losses(sdx, data, LAYERS, False)
    (cl + sm).backward()
    return {"encoder.image_encoder.backbone." + k: p.grad for k, p in bb.named_parameters()}


@functools.lru_cache(maxsize=None)
def _step_reference():
    sd, b, p_img, q_img = _step_inputs()
    bb = _encoder().backbone
    return (_oracle_image_step(sd, b, p_img, q_img, bb, torch.float64), _oracle_image_step(sd, b, p_img, q_img, bb, torch.float32))


@pytest.mark.parametrize("native", [True, False])
def test_training_step_from_raw_images(native):
    """PointDSC(num_layers=3).train(), B = 2, N = 256, images 2 x 3 x 64 x 80, classification + spectral loss: the gradients of
    encoder.image_encoder.* against the stock backbone in float64 feeding the oracle's training losses.  native_train = False
    (the path being replaced) passes the same check."""
    sd, b, p_img, q_img = _step_inputs()
    g64, g32 = _step_reference()
    m = gmf_amd.PointDSC(in_dim=6, num_layers=LAYERS, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
                         sigma_d=0.10, k=40, nms_radius=0.10)
    m.load_state_dict(sd, strict=False)
    m.encoder.image_encoder.load_state_dict(_encoder().state_dict())
    m = m.to(DEV).train()
    m.encoder.image_encoder.native_train = native
    data = {k: b[k].to(DEV) for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    data["p_image"], data["q_image"] = p_img.to(DEV), q_img.to(DEV)
    gt = b["gt_labels"].to(DEV)

    def run():
        res = m(data)
        cl = gmf_amd.ClassificationLoss(balanced=False)(res["final_labels"], gt)["loss"]
        sm = gmf_amd.SpectralMatchingLoss(balanced=False)(res["M"], gt)
        (cl + sm).backward()
    _, keys = _all_kernels(run)
    ours = {R.parse_kernel(k)[0] for k in keys if R.parse_kernel(k)}
    assert ("k_conv2d_wgrad" in ours) == native, sorted(ours)
    params = dict(m.named_parameters())
    assert len(g64) == 48
    _report(check_close({k: params[k].grad for k in g64}, g64, g32, what=f"native={native} grad "))


# ---- 8. shape errors ----------------------------------------------------------------------------------------------------------------
def test_too_small_image_raises_and_names_the_shape():
    enc = _encoder().to(DEV).train()
    with pytest.raises(ValueError, match=r"\(1, 3, 8, 8\)"):
        enc(torch.zeros(1, 3, 8, 8, device=DEV))
    h = _lib.handle_for(0)
    x = torch.zeros(4 * 4 * 32, device=DEV)
    with pytest.raises(RuntimeError, match=r"\(32, 64, 3, 1\)"):
        h.call("gmf_conv2d_forward_f32", x.data_ptr(), 512, 1, 128, 32, x.data_ptr(), x.data_ptr(), 1, 4, 4, 32, 64, 3, 1, _stream())
    with pytest.raises(RuntimeError, match="stem"):
        h.call("gmf_conv2d_dgrad", x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 1, 4, 4, 3, 64, 7, 2, _stream())
    with pytest.raises(RuntimeError, match="dense NHWC"):
        h.call("gmf_conv2d_forward_f32", x.data_ptr(), 1024, 16, 4, 1, x.data_ptr(), x.data_ptr(), 1, 4, 4, 64, 64, 3, 1, _stream())
