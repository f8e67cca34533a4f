"""float64 restatement of FCGF's ResUNetBN2C (GMF_DeepGlobalRegistration_fcgf/model/resunet.py:598-650) for the tests of
gmf_amd/fcgf.py, built on tests/sparse_reference.py's levels, maps, convolution and BatchNorm.  The inlier network's U-Net
without its fusion layers, with FCGF's head: conv1_tr (1x1) on [out_s1_tr | out_s1], ReLU, final (1x1 + bias) and, with
normalize_feature, y / (||y||_2 + 1e-8)."""
from __future__ import annotations

import torch

import sparse_reference as R


def fcgf_forward(sd, coords, feats, conv1_kernel_size: int, normalize: bool, dtype=torch.float64, calibrate: bool = False,
                 levels_maps=None):
    """-> (features [M, out], calib): calib the batch statistics of every BatchNorm input when `calibrate`, else None."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    if levels_maps is None:
        levels_maps = R.levels_and_maps(coords, conv1_kernel_size)
    lv, maps = levels_maps
    n = [len(r) for r in lv]
    calib = {} if calibrate else None

    def cbn(name, norm, x, m, lvl, residual=None, act=False):
        y = R.conv(x, maps[m] if m is not None else None, sd[name + ".kernel"], n[lvl], dtype)
        if norm is not None:
            y = R._bn(y, sd, norm, calib)
        if residual is not None:
            y = y + residual
        return torch.relu(y) if act else y

    def block(p, x, m, lvl):
        h = cbn(p + ".conv1", p + ".norm1", x, m, lvl, act=True)
        return cbn(p + ".conv2", p + ".norm2", h, m, lvl, residual=x, act=True)

    x = torch.as_tensor(feats).to(dtype)
    s1 = block("block1", cbn("conv1", "norm1", x, "c1", 0), "s0", 0)
    s2 = block("block2", cbn("conv2", "norm2", s1, "d01", 1), "s1", 1)
    s4 = block("block3", cbn("conv3", "norm3", s2, "d12", 2), "s2", 2)
    s8 = block("block4", cbn("conv4", "norm4", s4, "d23", 3), "s3", 3)
    t4 = block("block4_tr", cbn("conv4_tr", "norm4_tr", s8, "t32", 2), "s2", 2)
    t2 = block("block3_tr", cbn("conv3_tr", "norm3_tr", torch.cat([t4, s4], 1), "t21", 1), "s1", 1)
    t1 = block("block2_tr", cbn("conv2_tr", "norm2_tr", torch.cat([t2, s2], 1), "t10", 0), "s0", 0)
    o = cbn("conv1_tr", None, torch.cat([t1, s1], 1), None, 0, act=True)
    y = R.conv(o, None, sd["final.kernel"], n[0], dtype) + sd["final.bias"].to(dtype)
    if normalize:
        y = y / (torch.norm(y, p=2, dim=1, keepdim=True) + 1e-8)
    return y, calib


def head(xa, xb, W1, W2, bias, normalize, dtype=torch.float64):
    """The head alone: relu([xa | xb] W1) W2 + bias, then the optional normalisation, in `dtype`."""
    x = torch.cat([xa, xb], 1) if xb is not None else xa
    y = torch.relu(x.to(dtype) @ W1.to(dtype)) @ W2.to(dtype)
    if bias is not None:
        y = y + bias.to(dtype).reshape(-1)
    if normalize:
        y = y / (torch.norm(y, p=2, dim=1, keepdim=True) + 1e-8)
    return y


def conditioned_state_dict(model, coords, feats, seed: int = 0):
    """A state_dict of an FCGF `model` whose activations are O(1) on this input (as sparse_reference.conditioned_state_dict):
    kernels N(0, 1 / (k^D Cin)), BatchNorm affine near (1, 0), running stats = the batch statistics of an fp64 pass."""
    g = torch.Generator().manual_seed(seed)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for name, norm in R.LAYERS:
        W = sd[name + ".kernel"]
        K = W.shape[0] if W.dim() == 3 else 1
        sd[name + ".kernel"] = torch.randn(W.shape, generator=g) * (1.0 / (K * W.shape[-2])) ** 0.5
        if norm is not None:
            C = W.shape[-1]
            sd[norm + ".bn.weight"] = 1 + 0.1 * torch.randn(C, generator=g)
            sd[norm + ".bn.bias"] = 0.1 * torch.randn(C, generator=g)
    sd["final.bias"] = 0.1 * torch.randn(sd["final.bias"].shape, generator=g)
    _, calib = fcgf_forward(sd, coords, feats, model.conv1_kernel_size, False, calibrate=True)
    sd.update(calib)
    return sd
