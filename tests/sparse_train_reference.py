"""Train-mode restatement of DGR's inlier network ResUNetBN2C (resunet_new.py:627-706 with batch-statistics BatchNorm) and of the
inlier-model loss of GMF_DeepGlobalRegistration_fcgf/core/trainer.py:229-270, with torch autograd through it, for the tests of
the training path (gmf_amd.train.resunet_train, gmf_amd.dgr.inlier_training_loss).

Levels, maps and conditioned weights are tests/sparse_reference.py's; the fusion layers are oracle.gmf_oracle.fusion_layer.  The
convolution is sparse_reference.conv's per-offset gather / index_add, run on the device of its input (float64 on the device keeps
the whole-network comparisons within their time limit).  BatchNorm normalises with the biased batch variance and updates the
running variance with the unbiased one, as torch does.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import gmf_oracle as O
import sparse_reference as SR

EPS_BN = SR.EPS_BN


def transpose_map(cmap, n_in):
    """The pairs of a map (row_ptr, pairs) read backwards, as (row_ptr, pairs) over the n_in input rows: (d, o) for each pair (d, i)
    of output row o, ascending d within a row."""
    row_ptr, pairs = cmap
    o = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    d, i = pairs[:, 0], pairs[:, 1]
    srt = np.lexsort((d, i))
    rp = np.zeros(n_in + 1, dtype=np.int64)
    np.add.at(rp, i + 1, 1)
    return np.cumsum(rp), np.stack([d[srt], o[srt]], axis=1)


class DeviceMap:
    """A host map's (o, d, i) on a device, grouped by offset for the gather / index_add restatement."""

    def __init__(self, cmap, n_out, device):
        row_ptr, pairs = cmap
        o = np.repeat(np.arange(n_out), np.diff(row_ptr))
        self.n_out = n_out
        self.groups = []
        for dd in np.unique(pairs[:, 0]):
            s = pairs[:, 0] == dd
            self.groups.append((int(dd), torch.as_tensor(o[s], device=device), torch.as_tensor(pairs[s, 1], device=device)))


def conv(x, dmap, W, n_out):
    """sparse_reference.conv on x's device and dtype: y [n_out, Cout] = sum over the pairs (d, i) of row o of x[i] W[d];
    dmap None: the identity map."""
    W = W if W.dim() == 3 else W.unsqueeze(0)
    if dmap is None:
        return x[:n_out] @ W[0]
    y = x.new_zeros((n_out, W.shape[2]))
    for d, o, i in dmap.groups:
        y = y.index_add(0, o, x[i] @ W[d])
    return y


def bn_train(x, p, running):
    """BatchNorm1d in train mode on the rows of x: batch statistics; `running` {name: tensor} gets the updated running stats."""
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    n = x.shape[0]
    m = 0.1
    running[p + ".bn.running_mean"] = (1 - m) * p_get(running, p, "running_mean", x) + m * mean.detach()
    running[p + ".bn.running_var"] = (1 - m) * p_get(running, p, "running_var", x) + m * var.detach() * n / (n - 1)
    return (x - mean) / torch.sqrt(var + EPS_BN) * running["__params__"][p + ".bn.weight"] + running["__params__"][p + ".bn.bias"]


def p_get(running, p, name, x):
    return running["__init__"][f"{p}.bn.{name}"].to(x)


def resunet_train_forward(params, buffers, lm, feats, p_tok, q_tok, pe, c1_key="c1", relu_masks=None):
    """The train-mode forward over `params` {state_dict name: tensor (leaf, requires_grad)} and `buffers` (the running stats
    before the step), levels and device maps `lm` = (counts, {map name: DeviceMap or None}).  Returns (logits [n0, out],
    {running stat name: updated value}).

    relu_masks: None, or the 14 boolean masks [>= n_l, C] of the ReLUs that follow a BatchNorm, in forward order, to take in
    place of `> 0` (the derivative on a given side of every kink: a pre-activation within the forward's rounding of 0 makes
    the ReLU's derivative, and so every gradient upstream of it, depend on that rounding)."""
    n, maps = lm
    running = {"__params__": params, "__init__": buffers}
    masks = None if relu_masks is None else list(relu_masks)

    def relu(y):
        if masks is None:
            return torch.relu(y)
        return y * masks.pop(0)[:y.shape[0]].to(y)

    def cbn(name, norm, x, m, lvl, residual=None, act=False):
        y = conv(x, maps[m] if m is not None else None, params[name + ".kernel"], n[lvl])
        if norm is not None:
            y = bn_train(y, norm, running)
        if residual is not None:
            y = y + residual
        if act and norm is None:
            return torch.relu(y)
        return relu(y) if act else y

    def block(p, x, m, lvl):
        h = cbn(p + ".conv1", p + ".norm1", x, m, lvl, act=True)
        return cbn(p + ".conv2", p + ".norm2", h, m, lvl, residual=x, act=True)

    s1 = block("block1", cbn("conv1", "norm1", feats, c1_key, 0), "s0", 0)
    s2 = block("block2", cbn("conv2", "norm2", s1, "d01", 1), "s1", 1)
    s4 = block("block3", cbn("conv3", "norm3", s2, "d12", 2), "s2", 2)
    s8 = block("block4", cbn("conv4", "norm4", s4, "d23", 3), "s3", 3)
    image_feat = O.fusion_layer(params, "image_fusion.", p_tok, q_tok, False)
    f8 = O.fusion_layer(params, "perceiver_io.", image_feat, s8.unsqueeze(0), pe)[0]
    t4 = block("block4_tr", cbn("conv4_tr", "norm4_tr", f8, "t32", 2), "s2", 2)
    t2 = block("block3_tr", cbn("conv3_tr", "norm3_tr", torch.cat([t4, s4], 1), "t21", 1), "s1", 1)
    t1 = block("block2_tr", cbn("conv2_tr", "norm2_tr", torch.cat([t2, s2], 1), "t10", 0), "s0", 0)
    o = cbn("conv1_tr", None, torch.cat([t1, s1], 1), None, 0, act=True)
    out = conv(o, None, params["final.kernel"], n[0]) + params["final.bias"]
    upd = {k: v for k, v in running.items() if not k.startswith("__")}
    return out, upd


def device_levels_and_maps(coords, device, conv1_kernel_size=3):
    """(counts, {name: DeviceMap}, host levels) of sparse_reference.levels_and_maps, the maps moved to `device`; the level-0 rows
    stay in input order."""
    lv, maps = SR.levels_and_maps(coords, conv1_kernel_size)
    n = [len(r) for r in lv]
    out_level = {"s0": 0, "s1": 1, "s2": 2, "s3": 3, "d01": 1, "d12": 2, "d23": 3, "t10": 0, "t21": 1, "t32": 2, "c1": 0}
    dm = {k: (None if v is None else DeviceMap(v, n[out_level[k]], device)) for k, v in maps.items()}
    return n, dm


def inlier_training_loss(logits, xyz0s, xyz1s, pred_pairs, is_correct, T_gt, clip_weight_thresh=0.05, trans_weight=1.0,
                         procrustes_loss_weight=1.0, inlier_direct_loss_weight=1.0, use_balanced_loss=False):
    """trainer.py:229-270 in the dtype of `logits`: per batch the weighted Procrustes of registration.py:91-113 (fp64 SVD with the
    determinant fix), the errors of core/metrics.py, the mean over batches with ws > 10, plus the BCE of core/loss.py."""
    logits = logits.reshape(-1)
    w = torch.sigmoid(logits)
    w = torch.where(w > clip_weight_thresh, w, torch.zeros_like(w))
    Rs, ts, ws, o = [], [], [], 0
    for x0, x1, p in zip(xyz0s, xyz1s, pred_pairs):
        k = p.shape[0]
        wb = w[o:o + k]
        o += k
        X = x0[p[:, 0].long()].to(logits)
        Y = x1[p[:, 1].long()].to(logits)
        R, t = weighted_procrustes(X, Y, wb, float(np.finfo(np.float32).eps))
        Rs.append(R)
        ts.append(t)
        ws.append(float(wb.detach().sum()))
    R = torch.stack(Rs)
    t = torch.stack(ts)
    ws = torch.tensor(ws)
    T_gt = T_gt.to(logits)
    rot = torch.acos(torch.clamp(((R.reshape(-1, 9) * T_gt[:, :3, :3].reshape(-1, 9)).sum(1) - 1) / 2, min=-0.999, max=0.999))
    tr = torch.norm(t - T_gt[:, :3, 3], p=2, dim=1)
    valid = (ws > 10).to(logits.device)
    loss = procrustes_loss_weight * (rot + trans_weight * tr)[valid].mean()
    target = is_correct.to(logits).reshape(-1)
    if use_balanced_loss:
        crit = logits.new_zeros(())
        for lab in (0, 1):
            m = target == lab
            if bool(m.any()):
                crit = crit + F.binary_cross_entropy_with_logits(logits[m], target[m]) / 2
    else:
        crit = F.binary_cross_entropy_with_logits(logits, target)
    return loss + inlier_direct_loss_weight * crit, {"rot_error": rot, "trans_error": tr}


def weighted_procrustes(X, Y, w, eps):
    """GlobalRegistration.weighted_procrustes (registration.py:91-113), differentiable in w (torch's SVD)."""
    W1 = torch.abs(w).sum()
    w_norm = w / (W1 + eps)
    mux = (w_norm[:, None] * X).sum(0, keepdim=True)
    muy = (w_norm[:, None] * Y).sum(0, keepdim=True)
    Sxy = (Y - muy).t() @ (w_norm[:, None] * (X - mux))
    U, D, Vh = torch.linalg.svd(Sxy.double())
    S = torch.eye(3, dtype=torch.float64, device=X.device)
    if torch.det(U) * torch.det(Vh) < 0:
        S[2, 2] = -1
    R = (U @ S @ Vh).to(X)
    t = muy.reshape(-1) - R @ mux.reshape(-1)
    return R, t
