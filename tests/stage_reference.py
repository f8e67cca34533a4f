"""Restatements of the encoder's stage entry points (gmf_hip.h, "encoder stages") from the oracle's pieces, evaluated in any
dtype, and the floor-relative accuracy rule the stage tests apply.

Each function takes the state dict converted to the evaluation dtype (`sd_as`) and returns row-major tensors.  The scales the
packers fold into the weights are applied here as the kernels see them: Q' = (Wq f + bq) log2(e) / sqrt(C) (pack_front), and
the spatial-consistency softmax is taken in base 2 on Q' K^T (c_ij x Q'K^T, exp2) - the same function as the reference's
softmax(c_ij q k^T / sqrt(C)) up to those folded constants."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import gmf_oracle as O

EPS32 = float(np.finfo(np.float32).eps)
LOG2E = 1.4426950408889634
C = 128


def sd_as(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}


def floor_bound(ref64, ref32):
    """(err_fp32, bound): the fp32 restatement's error against float64 and the largest error a kernel may have,
    2 err_fp32 + 2 eps32 max|ref|."""
    r64 = ref64.double()
    e32 = (ref32.double() - r64).abs().max().item() if r64.numel() else 0.0
    scale = r64.abs().max().item() if r64.numel() else 0.0
    return e32, 2 * e32 + 2 * EPS32 * scale


def floor_violation(got, ref64, ref32):
    """None when `got` is finite and within 2 err_fp32 + 2 eps32 max|ref| of `ref64`, else a message."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape == ref32.shape, (got.shape, ref64.shape, ref32.shape)
    if not torch.isfinite(got).all():
        return f"{int((~torch.isfinite(got)).sum())} non-finite elements"
    e32, bound = floor_bound(ref64, ref32)
    err = (got - ref64.double()).abs().max().item() if got.numel() else 0.0
    if err > bound:
        return f"max error {err:.3e} > bound {bound:.3e} (err_fp32 {e32:.3e})"
    return None


def assert_floor(got, ref64, ref32, what):
    msg = floor_violation(got, ref64, ref32)
    assert msg is None, f"{what}: {msg}"


# ---- the stages -------------------------------------------------------------------------------------------------------------
def front(sd, layer, x, first):
    """gmf_front_forward: [layer0 if first] + PointCN_layer + projection_{q,k,v}; x = corr_pos [B,N,6] or features [B,N,C]."""
    if first:
        x = O._lin(x, sd["encoder.layer0.weight"], sd["encoder.layer0.bias"])
    f = O.point_cn(sd, f"encoder.blocks.PointCN_layer_{layer}.", x)
    n = f"encoder.blocks.NonLocal_layer_{layer}."
    q = O._lin(f, sd[n + "projection_q.weight"], sd[n + "projection_q.bias"]) * (LOG2E / math.sqrt(C))
    k = O._lin(f, sd[n + "projection_k.weight"], sd[n + "projection_k.bias"])
    v = O._lin(f, sd[n + "projection_v.weight"], sd[n + "projection_v.bias"])
    return f, q, k, v


def scattn(sd, layer, q, k, v, compat, fus):
    """gmf_scattn_forward(_dense): softmax_j(c_ij Q'_i.K_j in base 2) V, fc_message, + fusion2_out."""
    s = (q @ k.transpose(1, 2)) * math.log(2.0)
    msg = torch.softmax(compat * s, dim=-1) @ v
    return O.fc_message(msg, sd, f"encoder.blocks.NonLocal_layer_{layer}.fc_message.") + fus


def ctx_prepare(sd, prefix, ctx, pe):
    """gmf_fusion_ctx_prepare: [LCPE(content)] + LayerNorm_context + to_kv -> (Kc, Vc) [B,T,64]."""
    if pe:
        ctx = O.conv_pos_enc_1(ctx, sd[prefix + "cpe.proj_content.weight"], sd[prefix + "cpe.proj_content.bias"])
    a = prefix + "cross_attend_blocks.0."
    cn = O.layer_norm(ctx, sd[a + "norm_context.weight"], sd[a + "norm_context.bias"])
    kv = cn @ sd[a + "fn.to_kv.weight"].t()
    d = kv.shape[-1] // 2
    return kv[..., :d], kv[..., d:]


def fusion_attn(sd, prefix, x, Kc, Vc, pe):
    """gmf_fusion_attn_forward: [LCPE(q)] + LayerNorm + to_q + softmax(q Kc^T d^-1/2) Vc + to_out + the LCPE'd x."""
    if pe:
        x = O.conv_pos_enc_1(x, sd[prefix + "cpe.proj_q.weight"], sd[prefix + "cpe.proj_q.bias"])
    a = prefix + "cross_attend_blocks.0."
    xn = O.layer_norm(x, sd[a + "norm.weight"], sd[a + "norm.bias"])
    q = xn @ sd[a + "fn.to_q.weight"].t()
    p = torch.softmax((q @ Kc.transpose(-1, -2)) * (q.shape[-1] ** -0.5), dim=-1)
    return (p @ Vc) @ sd[a + "fn.to_out.weight"].t() + sd[a + "fn.to_out.bias"] + x


def fusion_ff(sd, prefix, x1):
    """gmf_fusion_ff_forward: geglu_ff(LayerNorm(x1)) + x1."""
    f = prefix + "cross_attend_blocks.1."
    xn = O.layer_norm(x1, sd[f + "norm.weight"], sd[f + "norm.bias"])
    return O.geglu_ff(xn, sd[f + "fn.net.0.weight"], sd[f + "fn.net.0.bias"], sd[f + "fn.net.2.weight"], sd[f + "fn.net.2.bias"]) + x1


def classifier(sd, feat):
    """gmf_classifier_forward: (logits, feat_n)."""
    return O.classifier(sd, feat), F.normalize(feat, p=2, dim=-1)
