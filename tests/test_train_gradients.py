"""The training path entry by entry against float64 autograd.

The reference of every comparison is torch autograd in float64 (the oracle's `training_losses` for the whole step, the plain
formula for a single autograd function), run on the device.  The same formula in float32 gives each tensor's noise floor:
`floor_t = max |ref32_t - ref64_t|`.  Every entry of every compared tensor must satisfy

    |hip - ref64| <= max(FLOOR_MULT * floor_t, REL * max|ref64_t|) + ABS_G * gmax

with gmax the largest entry of the group the tensor belongs to (all gradients of a model, all outputs of a function).  Wherever
the fp32 floor is below 5e-5 of the tensor's largest entry - every tensor of the training step up to N = 1000 at B = 2; at
16 x 1000 a few of them reach 4e-3 on their own - this is tighter than F19's `2e-4 * max_t + 3e-6 * gmax`.
`test_check_close_rejects_planted_errors` shows on the CPU what this catches and F19's heads-plus-norm check does not.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gmf_amd
from gmf_amd import synthetic
from oracle import gmf_oracle as O

DEV = "cuda:0"
gpu = pytest.mark.gpu

FLOOR_MULT, REL, ABS_G = 4.0, 2e-5, 3e-6
LAYERS = 3                        # twelve layers are chaotic in train mode (see oracle/gen_fixtures.py gen_f19)
SM_ROW_REL, SM_PAIR_REL = 1e-5, 1e-6


def check_close(got, ref, ref32, what="", gmax=None):
    """Assert the bound of the module docstring for every tensor of the dicts `got` (the HIP result), `ref` (float64) and
    `ref32` (the same reference in float32).  Names the tensor and the index of its worst entry on failure; returns
    {name: (max error, tolerance)}."""
    if gmax is None:
        gmax = max(float(r.detach().abs().max()) for r in ref.values())
    report = {}
    for name, r in ref.items():
        r = r.detach().double()
        g = got[name]
        assert g is not None, f"{what}{name}: no gradient"
        g = g.detach().to(r.device, torch.float64).reshape(r.shape)
        amax = float(r.abs().max())
        floor = float((ref32[name].detach().to(r.device, torch.float64).reshape(r.shape) - r).abs().max())
        tol = max(FLOOR_MULT * floor, REL * amax) + ABS_G * gmax
        err = (g - r).abs()
        worst = float(err.max())
        if not worst <= tol:
            idx = np.unravel_index(int(err.reshape(-1).argmax()), tuple(r.shape))
            raise AssertionError(f"{what}{name}: |hip - f64| = {worst:.3e} at index {tuple(int(i) for i in idx)} > tol {tol:.3e} "
                                 f"(fp32 floor {floor:.3e}, max|f64| {amax:.3e}, gmax {gmax:.3e})")
        report[name] = (worst, tol)
    return report


def f19_heads_and_norm_pass(got, ref, gmax):
    """F19's check of a gradient: the first 16 entries and the L2 norm, at 2e-4 of the tensor's largest entry + 3e-6 gmax."""
    for name, r in ref.items():
        r = r.detach().double().reshape(-1)
        g = got[name].detach().double().reshape(-1)
        k = min(16, r.numel())
        amax, nrm = float(r.abs().max()), float(r.norm())
        if float((g[:k] - r[:k]).abs().max()) >= 2e-4 * amax + 3e-6 * gmax:
            return False
        if abs(float(g.norm()) - nrm) >= 2e-4 * nrm + 3e-6 * gmax * math.sqrt(r.numel()):
            return False
    return True


# ---- the whole training step -----------------------------------------------------------------------------------------
def _trained_names(sd):
    return [k for k, v in sd.items() if v.is_floating_point() and k != "sigma_spat" and "running" not in k]


def oracle_step(sd, b, balanced, dtype, dev):
    """torch autograd over oracle.training_losses in `dtype` on `dev`: ({name: gradient}, {logits, M, losses})."""
    names = _trained_names(sd)
    sdx = {k: (v.to(dev, dtype).requires_grad_(k in names) if v.is_floating_point() else v.to(dev)) for k, v in sd.items()}
    data = {k: b[k].to(dev, dtype) for k in ("corr_pos", "src_keypts", "tgt_keypts", "p_tokens", "q_tokens", "gt_labels")}
    logits, M, cl, sm = O.training_losses(sdx, data, LAYERS, balanced)
    (cl + sm).backward()
    return ({n: sdx[n].grad for n in names},
            {"logits": logits.detach(), "M": M.detach(), "losses": torch.stack([cl.detach(), sm.detach()])})


def hip_step(sd, b, balanced, sigma_on_device=False):
    m = gmf_amd.PointDSC(in_dim=6, num_layers=LAYERS, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
                         sigma_d=0.10, k=40, nms_radius=0.10)
    m.load_state_dict(sd, strict=False)
    m = m.to(DEV).train()
    m.sigma_on_device = sigma_on_device
    data = {k: b[k].to(DEV) for k in ("corr_pos", "src_keypts", "tgt_keypts", "p_tokens", "q_tokens")}
    gt = b["gt_labels"].to(DEV)
    res = m(data)
    cl = gmf_amd.ClassificationLoss(balanced=balanced)(res["final_labels"], gt)["loss"]
    sm = gmf_amd.SpectralMatchingLoss(balanced=balanced)(res["M"], gt)
    (cl + sm).backward()
    params = dict(m.named_parameters())
    return ({n: params[n].grad for n in _trained_names(sd)},
            {"logits": res["final_labels"].detach(), "M": res["M"].detach(), "losses": torch.stack([cl.detach(), sm.detach()])})


def _step_batch(B, N, T, seed0=300):
    b = synthetic.synthetic_batch([seed0 + i for i in range(B)], N=N, T=T)
    return b


def test_check_close_rejects_planted_errors():
    """CPU: the bound passes the oracle's own fp32 gradients against fp64 and rejects four planted mistakes; F19's
    heads-plus-norm check lets two of them through."""
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, LAYERS, 128), seed=7)
    b = _step_batch(2, 200, 40)
    g64, _ = oracle_step(sd, b, False, torch.float64, "cpu")
    g32, _ = oracle_step(sd, b, False, torch.float32, "cpu")
    gmax = max(float(v.abs().max()) for v in g64.values())
    assert len(g64) == 137
    check_close(g32, g64, g32, gmax=gmax)

    wname = "encoder.blocks.PointCN_layer_1.0.weight"                  # [128, 128, 1]
    bname = max((n for n in g64 if n.endswith(".bias")), key=lambda n: float(g64[n].abs().max()))

    def planted(fn, name):
        bad = dict(g32)
        bad[name] = fn(g32[name].clone())
        return bad

    def flip(t):
        v = t.reshape(128, 128)
        v[64:, 64:] *= -1
        return t

    def swap(t):
        v = t.reshape(128, 128)
        v[[5, 77]] = v[[77, 5]]
        return t

    def transpose(t):
        return t.reshape(128, 128).t().contiguous().reshape(t.shape)

    def scale_max(t):
        v = t.reshape(-1)
        i = int(v.abs().argmax())
        v[i] *= 1.01
        return t

    cases = {"sign flip": planted(flip, wname), "row swap": planted(swap, wname), "transpose": planted(transpose, wname),
             "bias x 1.01": planted(scale_max, bname)}
    for what, bad in cases.items():
        with pytest.raises(AssertionError, match="at index"):
            check_close(bad, g64, g32, what=what + ": ", gmax=gmax)
    assert f19_heads_and_norm_pass(g32, g64, gmax)
    assert f19_heads_and_norm_pass(cases["sign flip"], g64, gmax)        # what the old check misses
    assert f19_heads_and_norm_pass(cases["row swap"], g64, gmax)


STEP_CASES = [  # (B, N, T, balanced, label overrides)
    (2, 200, 40, False, None),           # F19's shape
    (3, 150, 40, True, None),
    (1, 37, 1, True, None),              # one image token; N is a multiple of no tile
    (4, 257, 196, False, None),          # ragged 128-row tiles
    pytest.param((2, 1000, 40, True, "few"), marks=pytest.mark.xfail(strict=True, reason=(
        "open finding: with a pair without inliers and a pair with one (balanced losses), several weight gradients differ "
        "from float64 by up to 6e-4 of their largest entry while the fp32 oracle stays within 5e-5; cause not yet located"))),
    (16, 1000, 40, False, None),         # the training-timing shape: weight gradients on the 16-way split-K GEMM
]


@gpu
@pytest.mark.parametrize("case", STEP_CASES, ids=["B2N200T40mse", "B3N150T40bal", "B1N37T1bal", "B4N257T196mse", "B2N1000T40balfew",
                                                  "B16N1000T40mse"])
def test_training_step_every_entry(case):
    """One training step (train() mode, 3 layers, ClassificationLoss + SpectralMatchingLoss(M, gt)): every entry of the 137
    parameter gradients (sigma's included), the logits, both losses and all of M against float64 autograd of the oracle."""
    B, N, T, balanced, labels = case
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, LAYERS, 128), seed=7)
    b = _step_batch(B, N, T)
    if labels == "few":                  # labels enter only the losses: both sides see the same gt
        b["gt_labels"][0] = 0
        b["gt_labels"][1] = 0
        b["gt_labels"][1, 17] = 1
    _check_step(sd, b, balanced, sigma_on_device=False)


@gpu
def test_training_step_every_entry_sigma_on_device():
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, LAYERS, 128), seed=7)
    _check_step(sd, _step_batch(3, 150, 40), True, sigma_on_device=True)


def _check_step(sd, b, balanced, sigma_on_device):
    g64, o64 = oracle_step(sd, b, balanced, torch.float64, DEV)
    g32, o32 = oracle_step(sd, b, balanced, torch.float32, DEV)
    gh, oh = hip_step(sd, b, balanced, sigma_on_device)
    assert len(g64) == 137
    check_close(gh, g64, g32, what="grad ")
    for k in ("logits", "M", "losses"):
        check_close({k: oh[k]}, {k: o64[k]}, {k: o32[k]})


# ---- every autograd function of gmf_amd/train.py -------------------------------------------------------------------------
def _compare_fn(hip_fn, ref_fn, args, what="", seed=0):
    """hip_fn(*fp32 args) against ref_fn(*args) in float64 (ref_fn in float32: the floor); floating tensors of `args` that
    require grad are differentiated with one random upstream gradient per output.  Compares outputs and input gradients."""
    def run(fn, dtype, hip):
        a = [(x.detach().to(DEV, dtype).requires_grad_(x.requires_grad) if torch.is_tensor(x) and x.is_floating_point() else x)
             for x in args]
        if hip:
            a = [(x.detach().float().requires_grad_(x.requires_grad) if torch.is_tensor(x) and x.is_floating_point() else x)
                 for x in a]
        out = fn(*a)
        out = out if isinstance(out, tuple) else (out,)
        gen = torch.Generator(device="cpu").manual_seed(seed)
        ups = [torch.randn(o.shape, generator=gen, dtype=torch.float64).to(DEV, o.dtype) for o in out]
        torch.autograd.backward([o for o in out if o.requires_grad], [u for o, u in zip(out, ups) if o.requires_grad])
        outs = {f"out{i}": o.detach() for i, o in enumerate(out)}
        grads = {f"d{i}": x.grad for i, x in enumerate(a) if torch.is_tensor(x) and x.is_floating_point() and x.requires_grad}
        return outs, grads
    o64, g64 = run(ref_fn, torch.float64, False)
    o32, g32 = run(ref_fn, torch.float32, False)
    oh, gh = run(hip_fn, torch.float32, True)
    check_close(oh, o64, o32, what=what)
    if g64:
        check_close(gh, g64, g32, what=what)


def _grid(gen, shape, step, spread):
    """Values on a grid of `step` (products and sums of a few hundred stay exact in fp32: a ReLU mask is the same in any
    summation order, so the comparison of its gradient is not at the mercy of rounding at the kink)."""
    return (torch.randn(shape, generator=gen) * spread / step).round() * step


@gpu
@pytest.mark.parametrize("rows", [1, 37, 257, 16000])
@pytest.mark.parametrize("io", [(6, 128), (128, 384), (128, 32), (32, 1)])
def test_linear(rows, io):
    from gmf_amd import train as T_
    cin, cout = io
    gen = torch.Generator().manual_seed(rows * 1000 + cin + cout)
    x = _grid(gen, (rows, cin), 1 / 8, 2.0)
    W = _grid(gen, (cout, cin, 1), 1 / 64, 4.0 / math.sqrt(cin))
    bias = _grid(gen, (cout,), 1 / 64, 0.5)
    res = _grid(gen, (rows, cout), 1 / 8, 1.0)
    for has_b, has_r, relu in ((True, False, False), (False, False, False), (True, True, True), (True, False, True), (False, True, False)):
        args = [x.clone().requires_grad_(True), W.clone().requires_grad_(True), bias.clone().requires_grad_(True) if has_b else None,
                res.clone().requires_grad_(True) if has_r else None]

        def ref(x, W, b, r):
            y = x @ W[:, :, 0].t()
            y = y + b if b is not None else y
            y = y + r if r is not None else y
            return torch.relu(y) if relu else y
        _compare_fn(lambda x, W, b, r: T_.linear(x, W, b, residual=r, relu=relu), ref, args,
                    what=f"linear rows={rows} {cin}->{cout} b={has_b} r={has_r} relu={relu}: ")


@gpu
@pytest.mark.parametrize("rows", [2, 3, 257, 16000])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("momentum", [0.1, 0.37])
def test_batchnorm_train(rows, relu, momentum):
    """Train-mode BatchNorm1d (+ ReLU) over the rows, with a channel offset by +1e3 and a nearly constant one: output, the
    gradients to x, gamma and beta, and the running statistics against nn.BatchNorm1d in float64."""
    from gmf_amd import train as T_
    C = 128
    gen = torch.Generator().manual_seed(rows + int(relu))
    x = torch.randn(rows, C, generator=gen) * 2.0 + torch.randn(C, generator=gen)
    x[:, 3] += 1e3
    x[:, 9] = 0.25 + 1e-3 * torch.randn(rows, generator=gen)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
    run_m, run_v = 0.1 * torch.randn(C, generator=gen), 1 + 0.2 * torch.rand(C, generator=gen)

    bn = torch.nn.BatchNorm1d(C, momentum=momentum).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(run_m)
        bn.running_var.copy_(run_v)
    bn.train()
    xh = x.to(DEV).requires_grad_(True)
    yh = T_.batchnorm_train(xh, bn, relu=relu)
    mask = (yh.detach() > 0).double() if relu else None

    def ref_of(dtype):
        m = torch.nn.BatchNorm1d(C, momentum=momentum).to(DEV, dtype).train()
        with torch.no_grad():
            m.weight.copy_(gamma)
            m.bias.copy_(beta)
            m.running_mean.copy_(run_m)
            m.running_var.copy_(run_v)
        xr = x.to(DEV, dtype).requires_grad_(True)
        pre = m(xr)
        if relu:
            # the backward of the reference's ReLU uses the HIP kernel's mask: the two may differ where rounding decides the
            # sign (the channel at 1e3 keeps ~3e-5 of its spread after the mean is taken in fp32), nowhere else
            off = (mask != (pre.detach() > 0).double()) & (pre.detach().abs() > 1e-4 * float(pre.detach().abs().max()))
            assert not bool(off.any()), "ReLU masks differ away from the kink"
            return m, xr, pre * mask.to(dtype), torch.relu(pre.detach())
        return m, xr, pre, pre.detach()
    gen_u = torch.Generator().manual_seed(5)
    up = torch.randn(rows, C, generator=gen_u, dtype=torch.float64).to(DEV)
    (yh * up.float()).sum().backward()
    got_o = {"y": yh.detach(), "run_mean": bn.running_mean, "run_var": bn.running_var}
    got_g = {"dx": xh.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad}
    refs = {}
    for dtype in (torch.float64, torch.float32):
        m, xr, y, y_out = ref_of(dtype)
        (y * up.to(dtype)).sum().backward()
        refs[dtype] = ({"y": y_out, "run_mean": m.running_mean, "run_var": m.running_var},
                       {"dx": xr.grad, "dgamma": m.weight.grad, "dbeta": m.bias.grad})
    for name in got_o:
        check_close({name: got_o[name]}, {name: refs[torch.float64][0][name]}, {name: refs[torch.float32][0][name]},
                    what=f"bn rows={rows} relu={relu}: ")
    check_close(got_g, refs[torch.float64][1], refs[torch.float32][1], what=f"bn rows={rows} relu={relu}: ")


@gpu
@pytest.mark.parametrize("BN", [(1, 37), (2, 64), (2, 65), (3, 257), (2, 1000)])
def test_sc_attention(BN):
    """softmax_j(compat_ij <q_i, k_j> / sqrt(C)) V with whole zero rows and columns in compat: the message and dqkv (the three
    strided products into one buffer)."""
    from gmf_amd import train as T_
    B, N = BN
    C = 128
    gen = torch.Generator().manual_seed(B * 7919 + N)
    qkv = torch.randn(B, N, 3 * C, generator=gen)
    compat = torch.rand(B, N, N, generator=gen) * 2.0
    compat[:, N // 3, :] = 0
    compat[:, :, (2 * N) // 3] = 0
    compat[:, :, 0] = 0

    def ref(qkv, compat):
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        return torch.softmax(compat * (q @ k.transpose(1, 2)) / math.sqrt(C), dim=-1) @ v
    _compare_fn(T_.sc_attention, ref, [qkv.requires_grad_(True), compat], what=f"sc_attention B={B} N={N}: ")


@gpu
@pytest.mark.parametrize("NT", [(1, 1), (2, 2), (37, 300), (1, 300), (37, 1), (2, 37)])
@pytest.mark.parametrize("pe", [True, False])
def test_fusion_layer_train(NT, pe):
    _fusion_case(gmf_amd.FusionLayer, 128, 64, NT, pe)


@gpu
def test_perceiver_io_train():
    _fusion_case(gmf_amd.PerceiverIO, 256, 128, (37, 40), True)


def _fusion_case(cls, lat, dh, NT, pe):
    N, T = NT
    B = 2
    m = cls(depth=0, dim=128, latent_dim=lat, cross_heads=1, latent_heads=8, cross_dim_head=dh, latent_dim_head=dh, pe=pe)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = synthetic.seeded_state_dict(shapes, seed=31 + N + T)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    gen = torch.Generator().manual_seed(N * 1000 + T)
    x = torch.randn(B, N, lat, generator=gen)
    ctx = torch.randn(B, T, 128, generator=gen)
    up = torch.randn(B, N, lat, generator=gen, dtype=torch.float64)
    xh, ch = x.to(DEV).requires_grad_(True), ctx.to(DEV).requires_grad_(True)
    y = m(ch, queries_encoder=xh)
    y.backward(up.to(DEV).float())
    got = {"dx": xh.grad, "dctx": ch.grad}
    got.update({n: p.grad for n, p in m.named_parameters()})
    refs = []
    for dtype in (torch.float64, torch.float32):
        sdx = {k: v.to(DEV, dtype).requires_grad_(True) for k, v in sd.items()}
        xr, cr = x.to(DEV, dtype).requires_grad_(True), ctx.to(DEV, dtype).requires_grad_(True)
        yr = O.fusion_layer(sdx, "", cr, xr, pe=pe)
        yr.backward(up.to(DEV, dtype))
        g = {"dx": xr.grad, "dctx": cr.grad}
        g.update({n: sdx[n].grad for n, _ in m.named_parameters()})
        refs.append((yr.detach(), g))
    what = f"{cls.__name__} N={N} T={T} pe={pe}: "
    check_close({"out": y.detach()}, {"out": refs[0][0]}, {"out": refs[1][0]}, what=what)
    check_close(got, refs[0][1], refs[1][1], what=what)


@gpu
@pytest.mark.parametrize("on_device", [False, True])
def test_normalize_and_similarity_matrix(on_device):
    """F.normalize -> M = clamp(1 - (1 - Fn Fn^T) / sigma^2, 0, 1), zero diagonal, for a random upstream dM: M, d features and
    d sigma (gmf_normalize_rows, gmf_similarity_matrix, the dense gmf_similarity_backward)."""
    from gmf_amd import train as T_
    B, N = 2, 300
    gen = torch.Generator().manual_seed(77)
    f = torch.randn(B, N, 128, generator=gen) + 0.9 * torch.randn(1, 1, 128, generator=gen)     # s spread over both clamp sides
    sigma = torch.tensor([0.9])

    def hip(f, s):
        fn = T_.normalize_rows(f.reshape(B * N, 128)).reshape(B, N, 128)
        return T_.similarity_matrix_train(fn, s, T_.SIGMA_ON_DEVICE if on_device else None)

    def ref(f, s):
        fn = F.normalize(f, p=2, dim=-1)
        M = torch.clamp(1 - (1 - fn @ fn.transpose(1, 2)) / s ** 2, min=0, max=1)
        return M * (1 - torch.eye(N, device=M.device, dtype=M.dtype))
    _compare_fn(hip, ref, [f.requires_grad_(True), sigma.requires_grad_(True)], what=f"similarity on_device={on_device}: ")


@gpu
@pytest.mark.parametrize("kind", ["random", "zeros", "ones", "single", "weight", "large"])
def test_classification_loss(kind):
    from gmf_amd import train as T_
    B, N = (40, 2000) if kind == "large" else (3, 333)
    gen = torch.Generator().manual_seed(len(kind))
    pred = torch.randn(B, N, generator=gen) * 6
    pred[:, :5] = torch.tensor([80.0, -80.0, 80.0, -80.0, 0.0])
    gt = (torch.rand(B, N, generator=gen) < 0.3).float()
    gt[:, 2:4] = torch.tensor([0.0, 1.0])
    if kind == "zeros":
        gt.zero_()
    if kind == "ones":
        gt.fill_(1)
    if kind == "single":                 # one inlier in the batch: pos_weight ~ B N, on a confident logit
        gt.zero_()
        gt[1, 17] = 1
        pred[1, 17] = 9.0
    w = torch.rand(B, N, generator=gen) if kind == "weight" else None
    for balanced in (True, False):
        def ref(pred, gt, w):
            if w is not None:
                return (F.binary_cross_entropy_with_logits(pred, gt, reduction="none") * w).mean()
            if not balanced:
                return F.binary_cross_entropy_with_logits(pred, gt)
            pw = (torch.relu((1 - gt).sum() - 1) + 1) / (torch.relu(gt.sum() - 1) + 1)
            return F.binary_cross_entropy_with_logits(pred, gt, pos_weight=pw)
        _compare_fn(lambda p, g, w: T_.classification_loss_train(p, g, w, balanced)[0], ref,
                    [pred.requires_grad_(True), gt, w], what=f"classification {kind} balanced={balanced}: ")


def _sm_dense_ref(M, gt, balanced):
    gt = gt.to(M.dtype)
    N = M.shape[1]
    eye = torch.eye(N, device=M.device, dtype=M.dtype)
    gtM = gt[:, None, :] * gt[:, :, None] * (1 - eye)
    if balanced:
        lp = ((M - 1) ** 2 * gtM).sum((-1, -2)) / (torch.relu(gtM.sum((-1, -2)) - 1.0) + 1.0)
        ln = (M ** 2 * (1 - gtM)).sum((-1, -2)) / (torch.relu((1 - gtM).sum((-1, -2)) - 1.0) + 1.0)
        return torch.mean(lp * 0.5 + ln * 0.5)
    return ((M - gtM) ** 2).mean()


@gpu
@pytest.mark.parametrize("balanced", [True, False])
def test_spectral_matching_loss_dense(balanced):
    """SpectralMatchingLoss(M, gt) on a row-padded M (ldm > N) with a pair without inliers: the loss and dL/dM (zero in the
    padding and on the diagonal)."""
    B, N, ldm = 3, 301, 320
    gen = torch.Generator().manual_seed(9)
    base = torch.rand(B, N, ldm, generator=gen)
    base[:, torch.arange(N), torch.arange(N)] = 0                 # M's diagonal is zero by construction (PointDSC.py:233)
    gt = (torch.rand(B, N, generator=gen) < 0.2).float()
    gt[1] = 0
    sm = gmf_amd.SpectralMatchingLoss(balanced=balanced)
    _compare_fn(lambda m, g: sm(m[:, :, :N], g), lambda m, g: _sm_dense_ref(m[:, :, :N], g, balanced),
                [base.requires_grad_(True), gt], what=f"sm dense balanced={balanced}: ")


@gpu
@pytest.mark.parametrize("N", [1000, 1001])
def test_gemm_split_k_epilogue_into_strided_buffer(N):
    """gmf_gemm_f32 as the attention backward uses it, with everything at once: batched dV = P^T dmsg written into the middle
    column block of a [B, N, 3C] buffer (ldc != n, c_off), a long contraction on the split-K path (N = 1001: the direct
    kernel, K % 4 != 0), bias + residual + ReLU + alpha != 1 applied by the reduction.  The other two blocks stay untouched."""
    from gmf_amd import train as T_
    B, C, alpha = 2, 128, 0.7
    gen = torch.Generator().manual_seed(N)
    P = torch.rand(B, N, N, generator=gen).to(DEV)
    dm = torch.randn(B, N, C, generator=gen).to(DEV)
    bias = torch.randn(C, generator=gen).to(DEV)
    res = torch.randn(B, N, 3 * C, generator=gen).to(DEV) * 10
    out = torch.full((B, N, 3 * C), 7.0, device=DEV)
    T_.gemm(P, dm, ta=True, out=out, m=N, n=C, k=N, lda=N, ldb=C, ldc=3 * C, c_off=C, batch=B, sa=N * N, sb=N * C, sc=N * 3 * C,
            bias=bias, residual=res, alpha=alpha, relu=True)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        refs[dtype] = torch.relu(alpha * (P.to(dtype).transpose(1, 2) @ dm.to(dtype)) + bias.to(dtype) + res[..., C:2 * C].to(dtype))
    check_close({"out": out[..., C:2 * C]}, {"out": refs[torch.float64]}, {"out": refs[torch.float32]}, what=f"gemm N={N}: ")
    assert bool((out[..., :C] == 7.0).all()) and bool((out[..., 2 * C:] == 7.0).all())


# ---- SpectralMatchingLoss.from_features: per row and per pair ---------------------------------------------------------------
def sm_features(B, N, inliers, seed):
    """Unit features [B, N, 128] whose similarities cover both sides of the clamp, labels with inliers[b] inliers in pair b."""
    gen = torch.Generator().manual_seed(seed)
    f = torch.randn(B, N, 128, generator=gen) + 1.1 * torch.randn(B, 1, 128, generator=gen)
    gt = torch.zeros(B, N)
    for b, n in enumerate(inliers):
        idx = torch.randperm(N, generator=gen)[:n]
        gt[b, idx] = 1
        f[b, idx] += 1.5 * torch.randn(1, 128, generator=gen)
    return F.normalize(f, p=2, dim=-1), gt


def sm_from_features_errors(B, N, inliers, sigma, balanced, seed=0):
    """(loss err rel, dsigma err rel, per-row errors of dF scaled as in the test bound, gt, the reference rows' max, pair max)."""
    fn, gt = sm_features(B, N, inliers, seed)
    sm = gmf_amd.SpectralMatchingLoss(balanced=balanced)
    fh = fn.to(DEV).requires_grad_(True)
    sh = torch.tensor([sigma], device=DEV, requires_grad=True)
    loss = sm.from_features(fh, sh, gt.to(DEV))
    loss.backward()
    outs = {}
    for dtype in (torch.float64, torch.float32):
        fr = fn.to(DEV, dtype).requires_grad_(True)
        sr = torch.tensor([sigma], device=DEV, dtype=dtype, requires_grad=True)
        M = torch.clamp(1 - (1 - fr @ fr.transpose(1, 2)) / sr ** 2, min=0, max=1)
        M = M * (1 - torch.eye(N, device=DEV, dtype=dtype))          # zero diagonal (PointDSC.py:233)
        lr = _sm_dense_ref(M, gt.to(DEV), balanced)
        lr.backward()
        outs[dtype] = (float(lr.detach()), fr.grad.double(), float(sr.grad))
    l64, d64, s64 = outs[torch.float64]
    err = (fh.grad.double() - d64).abs().amax(-1)                       # [B, N]
    floor = (outs[torch.float32][1] - d64).abs().amax(-1)
    row_max = d64.abs().amax(-1)
    pair_max = row_max.amax(-1, keepdim=True)
    return {"loss": abs(float(loss) - l64) / abs(l64), "dsigma": abs(float(sh.grad) - s64) / abs(s64),
            "dsigma32": abs(outs[torch.float32][2] - s64) / abs(s64), "err": err, "floor": floor, "row_max": row_max,
            "pair_max": pair_max, "gt": gt.to(DEV)}


SM_CASES = [  # (B, N, inliers per pair)
    (1, 33, [5]),
    (2, 2000, [0, 1]),
    (2, 2000, [2, 6]),
    (2, 2000, [0, 600]),                 # a pair without inliers next to a pair with many
    (2, 5000, [1, 1200]),
]


@gpu
@pytest.mark.parametrize("case", SM_CASES, ids=lambda c: f"B{c[0]}N{c[1]}in{'-'.join(map(str, c[2]))}")
@pytest.mark.parametrize("sigma", [1.0, 0.8])
@pytest.mark.parametrize("balanced", [True, False])
def test_sm_from_features_per_row(case, sigma, balanced):
    """The fused backward of SpectralMatchingLoss.from_features (k_sm_backward) against float64 autograd, each ROW of dL/dFn
    against its own scale: a pair with few inliers makes its rows tiny next to the batch maximum, and only a per-row bound
    sees them."""
    B, N, inl = case
    r = sm_from_features_errors(B, N, inl, sigma, balanced, seed=N + sum(inl))
    assert r["loss"] < 1e-5, r["loss"]
    assert r["dsigma"] < max(4 * r["dsigma32"], 1e-5), (r["dsigma"], r["dsigma32"])
    tol = SM_ROW_REL * r["row_max"] + SM_PAIR_REL * r["pair_max"]
    bad = r["err"] > tol
    if bool(bad.any()):
        b, i = (int(v) for v in torch.nonzero(bad)[0])
        ratio = float((r["err"] / r["row_max"].clamp_min(1e-300)).max())
        raise AssertionError(f"row ({b}, {i}) gt={float(r['gt'][b, i]):.0f}: err {float(r['err'][b, i]):.3e} > {float(tol[b, i]):.3e} "
                             f"(row max {float(r['row_max'][b, i]):.3e}, fp32 floor {float(r['floor'][b, i]):.3e}); "
                             f"{int(bad.sum())} rows fail, worst err / row max {ratio:.2e}")
