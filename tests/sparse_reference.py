"""float64 restatement of the sparse coordinate engine, the sparse convolution and DGR's inlier network ResUNetBN2C
(GMF_DeepGlobalRegistration/*/model/resunet_new.py:424-721) for the tests of gmf_amd/sparse.py.

Levels and kernel maps are built on the host from integer keys: every row (batch, c_1 .. c_D) is encoded into one int64 and
looked up by binary search in the sorted keys of the input level.  The convolution gathers per offset and accumulates in the
dtype it is given (float64 for the reference, float32 for the "fp32 restatement" that bounds the device error).  The fusion
layers are oracle.gmf_oracle.fusion_layer.  The conventions are gmf_amd/sparse.py's ("Sparse inlier network").
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import gmf_oracle as O

EPS_BN = 1e-5

# forward order of the 23 convolutions: (kernel key, BatchNorm prefix or None)
LAYERS = [("conv1", "norm1"), ("block1.conv1", "block1.norm1"), ("block1.conv2", "block1.norm2"),
          ("conv2", "norm2"), ("block2.conv1", "block2.norm1"), ("block2.conv2", "block2.norm2"),
          ("conv3", "norm3"), ("block3.conv1", "block3.norm1"), ("block3.conv2", "block3.norm2"),
          ("conv4", "norm4"), ("block4.conv1", "block4.norm1"), ("block4.conv2", "block4.norm2"),
          ("conv4_tr", "norm4_tr"), ("block4_tr.conv1", "block4_tr.norm1"), ("block4_tr.conv2", "block4_tr.norm2"),
          ("conv3_tr", "norm3_tr"), ("block3_tr.conv1", "block3_tr.norm1"), ("block3_tr.conv2", "block3_tr.norm2"),
          ("conv2_tr", "norm2_tr"), ("block2_tr.conv1", "block2_tr.norm1"), ("block2_tr.conv2", "block2_tr.norm2"),
          ("conv1_tr", None), ("final", None)]


def kernel_offsets(k: int, D: int) -> np.ndarray:
    """[k^D, D]: offset index d has the first spatial axis varying fastest."""
    d = np.arange(k ** D)
    return np.stack([(d // k ** a) % k - k // 2 for a in range(D)], axis=1).astype(np.int64)


def coarsen(rows: np.ndarray, s: int) -> np.ndarray:
    out = rows.astype(np.int64).copy()
    out[:, 1:] = np.floor_divide(out[:, 1:], s) * s
    return out


def build_levels(coords, levels: int):
    """[level 0 = the input rows in input order, then the sorted unique coarse rows of each stride]."""
    lv = [np.asarray(coords, dtype=np.int64)]
    for l in range(1, levels):
        lv.append(np.unique(coarsen(lv[-1], 2 ** l), axis=0))
    return lv


class _Codec:
    """Rows (batch, c_1 .. c_D) -> one int64 each, order-preserving within the box the rows (and their neighbours) span."""

    def __init__(self, *row_sets, reach: int):
        allr = np.concatenate(row_sets, axis=0)
        self.lo = allr.min(axis=0) - reach
        span = allr.max(axis=0) + reach - self.lo + 1
        self.base = int(span.max())
        assert float(self.base) ** allr.shape[1] < 2.0 ** 62, "coordinates span too wide for the int64 codec"

    def __call__(self, rows):
        r = rows - self.lo
        code = np.zeros(rows.shape[0], dtype=np.int64)
        for c in range(rows.shape[1]):
            code = code * self.base + r[:, c]
        return code


def build_map(out_rows, in_rows, k: int, t: int, sign: int):
    """CSR (row_ptr [n_out + 1], pairs [nnz, 2] = (offset index, input row)): output o reads input o + sign d t."""
    offs = kernel_offsets(k, out_rows.shape[1] - 1)
    codec = _Codec(out_rows, in_rows, reach=(k // 2) * t)
    in_code = codec(in_rows)
    order = np.argsort(in_code, kind="stable")
    sorted_code = in_code[order]
    outs, ds, ins = [], [], []
    for d, off in enumerate(offs):
        q = out_rows.copy()
        q[:, 1:] += sign * off * t
        qc = codec(q)
        pos = np.searchsorted(sorted_code, qc)
        pos_c = np.minimum(pos, len(sorted_code) - 1)
        hit = sorted_code[pos_c] == qc
        o = np.nonzero(hit)[0]
        outs.append(o)
        ds.append(np.full(len(o), d))
        ins.append(order[pos_c[hit]])
    o = np.concatenate(outs)
    d = np.concatenate(ds)
    r = np.concatenate(ins)
    srt = np.lexsort((d, o))
    o, d, r = o[srt], d[srt], r[srt]
    row_ptr = np.zeros(out_rows.shape[0] + 1, dtype=np.int64)
    np.add.at(row_ptr, o + 1, 1)
    return np.cumsum(row_ptr), np.stack([d, r], axis=1)


def map_between(levels, k: int, out: int, inp: int):
    """The map of gmf_amd.SparsePlan's (k, out level, in level)."""
    t = 2 ** min(out, inp)
    return build_map(levels[out], levels[inp], k, t, -1 if out < inp else 1)


def conv(x, cmap, W, n_out: int, dtype=torch.float64):
    """y [n_out, Cout] = sum over the map's pairs (d, i) of row o of x[i] W[d], accumulated in `dtype`; cmap None: identity."""
    W = torch.as_tensor(W).to(dtype)
    if W.dim() == 2:
        W = W.unsqueeze(0)
    x = torch.as_tensor(x).to(dtype)
    if cmap is None:
        return x[:n_out] @ W[0]
    row_ptr, pairs = cmap
    o = torch.as_tensor(np.repeat(np.arange(n_out), np.diff(row_ptr)))
    d = torch.as_tensor(pairs[:, 0])
    r = torch.as_tensor(pairs[:, 1])
    y = torch.zeros((n_out, W.shape[2]), dtype=dtype)
    for dd in torch.unique(d).tolist():
        s = d == dd
        y.index_add_(0, o[s], x[r[s]] @ W[dd])
    return y


def _bn(x, sd, p, calib):
    if calib is not None:                       # conditioned weights: running stats = this pass's batch statistics
        calib[p + ".bn.running_mean"] = x.mean(0).float()
        calib[p + ".bn.running_var"] = x.var(0, unbiased=False).float()
        sd = dict(sd, **{k: v.to(x.dtype) for k, v in calib.items() if k.startswith(p + ".")})
    g = lambda n: sd[f"{p}.bn.{n}"].to(x.dtype)    # noqa: E731
    return (x - g("running_mean")) / torch.sqrt(g("running_var") + EPS_BN) * g("weight") + g("bias")


def resunet_forward(sd, coords, feats, p_tok, q_tok, pe: bool, conv1_kernel_size: int = 3, dtype=torch.float64,
                    calibrate: bool = False, levels_maps=None):
    """ResUNetBN2C.forward (resunet_new.py:627-706) in `dtype`.  sd: the module's state_dict (host tensors); coords [M, 1 + D];
    p_tok / q_tok [1, T, 128] (the image encoder's tokens).  Returns (logits [M, out], calib): calib the batch statistics of
    every BatchNorm input when `calibrate` (running stats to load for a conditioned test), else None."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    if levels_maps is None:
        levels_maps = levels_and_maps(coords, conv1_kernel_size)
    lv, maps = levels_maps
    n = [len(r) for r in lv]
    calib = {} if calibrate else None
    relu = torch.relu

    def cbn(name, norm, x, m, lvl, residual=None, act=False):
        y = conv(x, maps[m] if m is not None else None, sd[name + ".kernel"], n[lvl], dtype)
        if norm is not None:
            y = _bn(y, sd, norm, calib)
        if residual is not None:
            y = y + residual
        return relu(y) if act else y

    def block(p, x, m, lvl):
        h = cbn(p + ".conv1", p + ".norm1", x, m, lvl, act=True)
        return cbn(p + ".conv2", p + ".norm2", h, m, lvl, residual=x, act=True)

    x = torch.as_tensor(feats).to(dtype)
    s1 = block("block1", cbn("conv1", "norm1", x, "c1", 0), "s0", 0)
    s2 = block("block2", cbn("conv2", "norm2", s1, "d01", 1), "s1", 1)
    s4 = block("block3", cbn("conv3", "norm3", s2, "d12", 2), "s2", 2)
    s8 = block("block4", cbn("conv4", "norm4", s4, "d23", 3), "s3", 3)
    f = {k: v.to(dtype) for k, v in sd.items() if k.startswith(("image_fusion.", "perceiver_io."))}
    image_feat = O.fusion_layer(f, "image_fusion.", p_tok.to(dtype), q_tok.to(dtype), False)
    f8 = O.fusion_layer(f, "perceiver_io.", image_feat, s8.unsqueeze(0), pe)[0]
    t4 = block("block4_tr", cbn("conv4_tr", "norm4_tr", f8, "t32", 2), "s2", 2)
    t2 = block("block3_tr", cbn("conv3_tr", "norm3_tr", torch.cat([t4, s4], 1), "t21", 1), "s1", 1)
    t1 = block("block2_tr", cbn("conv2_tr", "norm2_tr", torch.cat([t2, s2], 1), "t10", 0), "s0", 0)
    o = cbn("conv1_tr", None, torch.cat([t1, s1], 1), None, 0, act=True)
    out = conv(o, None, sd["final.kernel"], n[0], dtype) + sd["final.bias"].to(dtype)
    return out, calib


def levels_and_maps(coords, conv1_kernel_size: int = 3):
    coords = np.asarray(coords, dtype=np.int64)
    lv = build_levels(coords, 4)
    maps = {"s0": map_between(lv, 3, 0, 0), "s1": map_between(lv, 3, 1, 1), "s2": map_between(lv, 3, 2, 2),
            "s3": map_between(lv, 3, 3, 3), "d01": map_between(lv, 3, 1, 0), "d12": map_between(lv, 3, 2, 1),
            "d23": map_between(lv, 3, 3, 2), "t10": map_between(lv, 3, 0, 1), "t21": map_between(lv, 3, 1, 2),
            "t32": map_between(lv, 3, 2, 3)}
    k1 = conv1_kernel_size
    maps["c1"] = maps["s0"] if k1 == 3 else (None if k1 == 1 else map_between(lv, k1, 0, 0))
    return lv, maps


def conditioned_state_dict(model, coords, feats, p_tok, q_tok, seed: int = 0):
    """A state_dict of `model` whose activations are O(1) on this input: kernels N(0, 1 / (k^D Cin)) scaled by fan-in, BatchNorm
    affine near (1, 0), running stats = the batch statistics of an fp64 restatement pass on the input; the bias and the fusion
    layers as initialised."""
    g = torch.Generator().manual_seed(seed)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for name, norm in LAYERS:
        W = sd[name + ".kernel"]
        K = W.shape[0] if W.dim() == 3 else 1
        cin = W.shape[-2]
        sd[name + ".kernel"] = torch.randn(W.shape, generator=g) * (1.0 / (K * cin)) ** 0.5
        if norm is not None:
            C = W.shape[-1]
            sd[norm + ".bn.weight"] = 1 + 0.1 * torch.randn(C, generator=g)
            sd[norm + ".bn.bias"] = 0.1 * torch.randn(C, generator=g)
    sd["final.bias"] = 0.1 * torch.randn(sd["final.bias"].shape, generator=g)
    _, calib = resunet_forward(sd, coords, feats, p_tok, q_tok, pe=model.pe, conv1_kernel_size=model.conv1_kernel_size,
                               calibrate=True)
    sd.update(calib)
    return sd
