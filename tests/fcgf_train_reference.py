"""Train-mode restatement of FCGF's ResUNetBN2C (GMF_DeepGlobalRegistration_fcgf/model/resunet.py:598-650 with batch-statistics
BatchNorm) and of the hardest-contrastive loss as gmf_amd.fcgf.hardest_contrastive_loss defines it, in plain torch (float64 or
float32) with autograd through it, for the tests of gmf_amd.train.fcgf_train and of the loss.

The convolution, the train-mode BatchNorm and the levels / maps are tests/sparse_train_reference.py's (`conv`, `bn_train`,
`device_levels_and_maps(..., conv1_kernel_size)`).  The network is the inlier network's U-Net without its fusion layers and with
FCGF's head: conv1_tr (1x1) on [out_s1_tr | out_s1], ReLU, final (1x1 + bias) and, with normalize, y / (||y||_2 + 1e-8) - a zero
row giving a zero row and a zero gradient.
"""
from __future__ import annotations

import torch

import sparse_train_reference as STR


def normalize_eps(y):
    """y / (||y||_2 + 1e-8) per row; a zero row gives a zero row and a zero gradient (gmf_amd.train.normalize_rows_eps)."""
    n = torch.linalg.vector_norm(y, dim=1, keepdim=True)
    live = n > 0
    safe = torch.where(live, y, torch.ones_like(y))            # the dead rows never reach the norm's backward
    out = safe / (torch.linalg.vector_norm(safe, dim=1, keepdim=True) + 1e-8)
    return torch.where(live, out, torch.zeros_like(out))


def fcgf_train_forward(params, buffers, lm, feats, normalize, relu_masks=None):
    """The train-mode forward over `params` {state_dict name: tensor (leaf, requires_grad)} and `buffers` (the running statistics
    before the step), levels and device maps `lm` = (counts, {map name: DeviceMap or None}) with conv1's map under "c1".
    Returns (features [n0, out], {running stat name: updated value}).

    relu_masks: None, or the 15 boolean masks [>= n_l, C] of the network's ReLUs in forward order - the 14 that follow a BatchNorm,
    then the head's - to take in place of `> 0` (sparse_train_reference.resunet_train_forward says why)."""
    n, maps = lm
    running = {"__params__": params, "__init__": buffers}
    masks = None if relu_masks is None else list(relu_masks)

    def relu(y):
        if masks is None:
            return torch.relu(y)
        return y * masks.pop(0)[:y.shape[0]].to(y)

    def cbn(name, norm, x, m, lvl, residual=None, act=False):
        y = STR.conv(x, maps[m] if m is not None else None, params[name + ".kernel"], n[lvl])
        if norm is not None:
            y = STR.bn_train(y, norm, running)
        if residual is not None:
            y = y + residual
        return relu(y) if act else y

    def block(p, x, m, lvl):
        h = cbn(p + ".conv1", p + ".norm1", x, m, lvl, act=True)
        return cbn(p + ".conv2", p + ".norm2", h, m, lvl, residual=x, act=True)

    s1 = block("block1", cbn("conv1", "norm1", feats, "c1", 0), "s0", 0)
    s2 = block("block2", cbn("conv2", "norm2", s1, "d01", 1), "s1", 1)
    s4 = block("block3", cbn("conv3", "norm3", s2, "d12", 2), "s2", 2)
    s8 = block("block4", cbn("conv4", "norm4", s4, "d23", 3), "s3", 3)
    t4 = block("block4_tr", cbn("conv4_tr", "norm4_tr", s8, "t32", 2), "s2", 2)
    t2 = block("block3_tr", cbn("conv3_tr", "norm3_tr", torch.cat([t4, s4], 1), "t21", 1), "s1", 1)
    t1 = block("block2_tr", cbn("conv2_tr", "norm2_tr", torch.cat([t2, s2], 1), "t10", 0), "s0", 0)
    o = cbn("conv1_tr", None, torch.cat([t1, s1], 1), None, 0, act=True)
    out = STR.conv(o, None, params["final.kernel"], n[0]) + params["final.bias"]
    if normalize:
        out = normalize_eps(out)
    assert not masks, "relu_masks holds more masks than the network has ReLUs"
    upd = {k: v for k, v in running.items() if not k.startswith("__")}
    return out, upd


def hardest_contrastive_loss(F0, F1, positive_pairs, sel0, sel1, pos_sel=None, pos_thresh=0.1, neg_thresh=1.4, h01=None, h10=None,
                             masks=None):
    """The loss of gmf_amd.fcgf.hardest_contrastive_loss in the dtype of F0 / F1, differentiable by autograd.
    -> (pos_loss, neg_loss, aux); aux holds h01, h10, keep0, keep1, D01, D10, the second-best distances `D01_second` /
    `D10_second` (inf with a single candidate) and the three hinge arguments `pos_arg`, `neg0_arg`, `neg1_arg`.

    h01 / h10: the mined rows to take in place of the argmin.  masks: (pos, neg0, neg1) boolean hinge masks to take in place
    of `> 0`."""
    pairs = positive_pairs if pos_sel is None else positive_pairs[pos_sel]
    i, j = pairs[:, 0], pairs[:, 1]
    a0, a1 = F0[i], F1[j]

    def dist(a, b):                                        # [P, H]
        return torch.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(2) + 1e-7)

    def mine(anchor, cand, sel, given):
        d = dist(anchor, cand[sel])
        pos = d.argmin(1) if given is None else None       # torch's argmin: the first of equal values
        h = sel[pos] if given is None else given
        D = torch.sqrt(((anchor - cand[h]) ** 2).sum(1) + 1e-7)
        second = torch.topk(d.detach(), 2, dim=1, largest=False).values[:, 1] if d.shape[1] > 1 else torch.full_like(D, float("inf"))
        return h, D, second

    h01_, D01, second01 = mine(a0, F1, sel1, h01)
    h10_, D10, second10 = mine(a1, F0, sel0, h10)
    nmax = max(F0.shape[0], F1.shape[0])
    keys = torch.sort(positive_pairs[:, 0] + positive_pairs[:, 1] * nmax).values

    def member(key):
        at = torch.searchsorted(keys, key).clamp(max=keys.shape[0] - 1)
        return keys[at] == key
    keep0 = ~member(i + h01_ * nmax)
    keep1 = ~member(h10_ + j * nmax)

    pos_arg = ((a0 - a1) ** 2).sum(1) - pos_thresh
    neg0_arg, neg1_arg = neg_thresh - D01, neg_thresh - D10

    def hinge(x, m):
        return torch.relu(x) if m is None else x * m.to(x)
    m = (None, None, None) if masks is None else masks
    pos_loss = hinge(pos_arg, m[0]).mean()

    def masked_mean(v, keep):
        return (v * keep.to(v)).sum() / keep.sum() if bool(keep.any()) else v.sum() * 0.0
    neg_loss = 0.5 * (masked_mean(hinge(neg0_arg, m[1]) ** 2, keep0) + masked_mean(hinge(neg1_arg, m[2]) ** 2, keep1))
    aux = {"h01": h01_, "h10": h10_, "keep0": keep0, "keep1": keep1, "D01": D01.detach(), "D10": D10.detach(),
           "D01_second": second01, "D10_second": second10, "pos_arg": pos_arg.detach(), "neg0_arg": neg0_arg.detach(),
           "neg1_arg": neg1_arg.detach()}
    return pos_loss, neg_loss, aux


def margin_case(seed=2, N0=300, N1=257, C=32, K=180, P=64, H=50, noise=0.45, dtype=torch.float32):
    """The loss case of the tests: correlated unit features (F1[j] = normalise(F0[i] + noise) on the positives), some true
    partners among the candidates, thresholds near the medians of their hinge arguments.  tests/test_fcgf_train_host.py asserts
    its margins in float64: every hinge argument and every gap between a mined row and its runner-up is at least 1e-4, so a
    float32 implementation must reproduce the selection and the masks exactly.  -> dict of host tensors and the two thresholds."""
    g = torch.Generator().manual_seed(seed)
    F0 = torch.nn.functional.normalize(torch.randn(N0, C, generator=g, dtype=torch.float64), dim=1)
    F1 = torch.nn.functional.normalize(torch.randn(N1, C, generator=g, dtype=torch.float64), dim=1)
    i = torch.randperm(N0, generator=g)[:K]
    j = torch.randperm(N1, generator=g)[:K]
    F1[j] = torch.nn.functional.normalize(F0[i] + noise * torch.randn(K, C, generator=g, dtype=torch.float64), dim=1)
    extra = torch.stack([i[:K // 3], j[torch.randperm(K // 3, generator=g)]], 1)     # a few rows with several partners
    pairs = torch.unique(torch.cat([torch.stack([i, j], 1), extra]), dim=0)
    if P is None:                                           # every pair sampled
        pos_sel = None
    else:
        pos_sel = torch.randperm(pairs.shape[0], generator=g)[:P]
    if H is None:                                           # every row a candidate
        sel0, sel1 = torch.arange(N0), torch.arange(N1)
    else:
        # candidates: some true partners of the sampled rows, the rest random rows
        sampled = pairs if pos_sel is None else pairs[pos_sel]
        q = len(sampled) // 4
        sel1 = torch.unique(torch.cat([sampled[:q, 1], torch.randperm(N1, generator=g)[:H]]))[:H]
        sel0 = torch.unique(torch.cat([sampled[q:2 * q, 0], torch.randperm(N0, generator=g)[:H]]))[:H]
        sel1 = sel1[torch.randperm(sel1.shape[0], generator=g)]
        sel0 = sel0[torch.randperm(sel0.shape[0], generator=g)]
    F0, F1 = F0.to(dtype), F1.to(dtype)
    _, _, aux = hardest_contrastive_loss(F0.double(), F1.double(), pairs, sel0, sel1, pos_sel, 0.0, 0.0)

    def between_the_middle(v):                              # no value of v sits on the threshold
        v = torch.sort(v).values
        return float(v[len(v) // 2 - 1] + v[len(v) // 2]) / 2
    pos_thresh = between_the_middle(aux["pos_arg"])
    kept = torch.cat([aux["D01"][aux["keep0"]], aux["D10"][aux["keep1"]]])
    neg_thresh = between_the_middle(kept if len(kept) >= 2 else torch.cat([aux["D01"], aux["D10"]]))
    return {"F0": F0, "F1": F1, "pairs": pairs, "sel0": sel0, "sel1": sel1, "pos_sel": pos_sel, "pos_thresh": pos_thresh,
            "neg_thresh": neg_thresh}
