"""Helpers of the image encoder's training tests (gmf_amd/csrc/image_train_kernels.hip): seeded cases with their float64 /
float32 autograd references, and float64 restatements of the index formulas the kernels use - the dgrad as a gather, the wgrad
sum, the max-pool's first-maximum rule - which test_image_train_host.py holds against torch on the CPU.  Nothing here needs a GPU.

Tolerance: tests/test_train_gradients.py `check_close`, |hip - ref64| <= max(4 floor, 2e-5 max|ref64|) + 3e-6 gmax for every
entry, floor = the same computation in float32 on the CPU."""
import torch
import torch.nn.functional as F

CONV_SHAPES = [(3, 64, 7, 2), (64, 64, 3, 1), (128, 128, 3, 1), (64, 128, 3, 2), (64, 128, 1, 2)]     # cin, cout, ks, stride


def out_size(H, W, ks, stride):
    pad = ks // 2
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def conv_autograd(x, Wt, dy, stride, dtype, dx_add=None):
    """{y, dx, dW} of F.conv2d(x, W, pad = ks // 2) for the upstream gradient dy, in `dtype` on the CPU (dx + dx_add if given)."""
    x = x.detach().clone().to(dtype).requires_grad_(True)
    Wt = Wt.detach().clone().to(dtype).requires_grad_(True)
    y = F.conv2d(x, Wt, None, stride, Wt.shape[2] // 2)
    y.backward(dy.to(dtype))
    dx = x.grad if dx_add is None else x.grad + dx_add.to(dtype)
    return {"y": y.detach(), "dx": dx, "dW": Wt.grad}


def conv_train_case(cin, cout, ks, stride, B, H, W, seed):
    """Seeded x [B, cin, H, W], W [cout, cin, ks, ks], dy, dx_add and the float64 / float32 autograd results (with and
    without dx_add)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=gen)
    Wt = torch.randn(cout, cin, ks, ks, generator=gen) / (cin * ks * ks) ** 0.5
    Ho, Wo = out_size(H, W, ks, stride)
    dy = torch.randn(B, cout, Ho, Wo, generator=gen)
    dx_add = torch.randn(B, cin, H, W, generator=gen)
    c = {"x": x, "W": Wt, "dy": dy, "dx_add": dx_add, "stride": stride, "Ho": Ho, "Wo": Wo}
    for name, dt in (("ref", torch.float64), ("f32", torch.float32)):
        c[name] = conv_autograd(x, Wt, dy, stride, dt)
        c[name]["dx_added"] = c[name]["dx"] + dx_add.to(dt)
    return c


# ---- the launchers' arithmetic (launch_conv2d_forward / _dgrad / _wgrad), recomputed ------------------------------------------------
def conv_workgroups(P, n):
    """Workgroups of k_conv2d_f32 over P pixels (of y for the forward, of dx for the dgrad) and n output channels."""
    return ((P + 255) // 256) * (n // 64)


def wgrad_slabs(cin, cout, ks, P):
    """Pixel chunks of the wgrad over P output pixels: chunks of at least 256 pixels, about 2048 waves, at most 256 chunks; the
    chunk length is rounded up to an even number (an MFMA step contracts a pixel pair)."""
    groups = 1 if cin == 3 else ks * ks * (cout // 64) * (cin // 64)
    n = max(1, min(min(256, max(1, 2048 // groups)), (P + 255) // 256))
    chunk = ((P + n - 1) // n + 1) // 2 * 2
    return (P + chunk - 1) // chunk


# ---- the kernels' index formulas in float64 -------------------------------------------------------------------------------------
def dgrad_gather(dy, Wt, H, W, stride):
    """dx[b, ci, y, x] = sum over taps (ky, kx) and co of dy[b, co, (y + pad - ky) / s, (x + pad - kx) / s] W[co, ci, ky, kx] where
    both divisions are exact and the output pixel exists (k_conv2d_f32<.., DG = true>): every dx entry is computed, none
    scattered to."""
    dy, Wt = dy.double(), Wt.double()
    B, cout, Ho, Wo = dy.shape
    cin, ks = Wt.shape[1], Wt.shape[2]
    pad = ks // 2
    dx = torch.zeros(B, cin, H, W, dtype=torch.float64)
    ys, xs = torch.arange(H), torch.arange(W)
    for ky in range(ks):
        ty = ys + pad - ky
        vy = (ty >= 0) & (ty % stride == 0) & (ty // stride < Ho)
        for kx in range(ks):
            tx = xs + pad - kx
            vx = (tx >= 0) & (tx % stride == 0) & (tx // stride < Wo)
            if not (vy.any() and vx.any()):
                continue
            src = dy[:, :, (ty[vy] // stride)][:, :, :, (tx[vx] // stride)]              # [B, cout, ny, nx]
            term = torch.einsum("bohw,oi->bihw", src, Wt[:, :, ky, kx])
            dx[:, :, torch.nonzero(vy)[:, 0][:, None], torch.nonzero(vx)[:, 0][None, :]] += term
    return dx


def wgrad_sum(x, dy, ks, stride):
    """dW[co, ci, ky, kx] = sum over output pixels p of dy[p, co] x[p s + k - pad, ci], 0 outside the image (k_conv2d_wgrad,
    k_stem_wgrad)."""
    x, dy = x.double(), dy.double()
    B, cout, Ho, Wo = dy.shape
    pad = ks // 2
    xp = F.pad(x, (pad, pad, pad, pad))
    dW = torch.zeros(cout, x.shape[1], ks, ks, dtype=torch.float64)
    for ky in range(ks):
        for kx in range(ks):
            win = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            dW[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", dy, win)
    return dW


def maxpool_first_max(x):
    """(y, arg) of max-pool 3x3 stride 2 pad 1 on [B, C, H, W]: arg = y2 * W + x2 of the window's FIRST maximum in row-major
    window order (a later element wins only when strictly greater) - k_maxpool_bwd's rule."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (1, 1, 1, 1), value=float("-inf"))
    best = torch.full((B, C, Ho, Wo), float("-inf"), dtype=x.dtype)
    arg = torch.full((B, C, Ho, Wo), -1, dtype=torch.long)
    oy, ox = torch.arange(Ho)[:, None], torch.arange(Wo)[None, :]
    for ky in range(3):
        for kx in range(3):
            v = xp[:, :, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2]
            y2, x2 = oy * 2 - 1 + ky, ox * 2 - 1 + kx
            inside = ((y2 >= 0) & (y2 < H) & (x2 >= 0) & (x2 < W)).expand(B, C, Ho, Wo)
            take = inside & ((arg < 0) | (v > best))
            best = torch.where(take, v, best)
            arg = torch.where(take, (y2 * W + x2).expand(B, C, Ho, Wo), arg)
    return best, arg


def maxpool_backward_gather(x, dy):
    """dx of the max-pool by the first-maximum rule, float64."""
    B, C, H, W = x.shape
    _, arg = maxpool_first_max(x)
    dx = torch.zeros(B, C, H * W, dtype=torch.float64)
    dx.scatter_add_(2, arg.reshape(B, C, -1), dy.double().reshape(B, C, -1))
    return dx.reshape(B, C, H, W)


def maxpool_autograd(x, dy, dtype):
    x = x.detach().clone().to(dtype).requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    y.backward(dy.to(dtype))
    return {"y": y.detach(), "dx": x.grad}


def maxpool_case(B, H, W, C, seed, ties=False):
    """Seeded [B, C, H, W] input and upstream gradient.  ties: the values are ReLU outputs quantised to quarters, so windows hold
    equal positive maxima; the window of output (1, 1) holds the same maximum twice (at its second and sixth element), and the
    window of output (2, 3) is all zero, in every channel."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=gen)
    if ties:
        x = torch.relu((x * 4).round() / 4)
        x[:, :, 1:4, 1:4] = torch.minimum(x[:, :, 1:4, 1:4], torch.tensor(1.0))
        x[:, :, 1, 2] = 5.0
        x[:, :, 2, 3] = 5.0
        x[:, :, 3:6, 5:8] = 0.0
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(B, C, Ho, Wo, generator=gen)
    return x, dy


# ---- residual BatchNorm + ReLU ----------------------------------------------------------------------------------------------------
def bn_residual_case(rows, C, seed):
    gen = torch.Generator().manual_seed(seed)
    c = {"x": torch.randn(rows, C, generator=gen) * 1.5 + 0.3, "res": torch.randn(rows, C, generator=gen),
         "gamma": torch.rand(C, generator=gen) + 0.5, "beta": torch.randn(C, generator=gen) * 0.2,
         "rm": torch.randn(C, generator=gen) * 0.1, "rv": torch.rand(C, generator=gen) + 0.5,
         "dy": torch.randn(rows, C, generator=gen)}
    return c


def bn_residual_autograd(c, dtype, relu=True, eps=1e-5, momentum=0.1):
    """relu?(batch_norm(x) + res) in training mode: outputs, the four gradients and the updated running statistics."""
    x, res, gamma, beta = (c[k].detach().clone().to(dtype).requires_grad_(True) for k in ("x", "res", "gamma", "beta"))
    rm, rv = c["rm"].to(dtype).clone(), c["rv"].to(dtype).clone()
    y = F.batch_norm(x, rm, rv, gamma, beta, True, momentum, eps) + res
    if relu:
        y = torch.relu(y)
    y.backward(c["dy"].to(dtype))
    return {"y": y.detach(), "dx": x.grad, "dres": res.grad, "dgamma": gamma.grad, "dbeta": beta.grad, "running_mean": rm,
            "running_var": rv}


# ---- the whole encoder ------------------------------------------------------------------------------------------------------------
def stock_encoder_step(backbone, images, projections, dtype):
    """The stock `_ResNet34ToLayer2` (a deep copy in `dtype`, train mode, on the CPU) called once per image; loss = sum over the
    calls of <output, projection>.  -> ({name: output}, {name: gradient}, {name: running statistic / num_batches_tracked})."""
    import copy
    bb = copy.deepcopy(backbone).to("cpu", dtype).train()
    outs, loss = {}, 0
    for n, (img, proj) in enumerate(zip(images, projections)):
        y = bb(img.to("cpu", dtype))
        outs[f"out{n}"] = y.detach()
        loss = loss + (y * proj.to("cpu", dtype)).sum()
    loss.backward()
    grads = {k: p.grad for k, p in bb.named_parameters()}
    stats = {k: v.detach().clone() for k, v in bb.state_dict().items() if "running" in k or "num_batches" in k}
    return outs, grads, stats
