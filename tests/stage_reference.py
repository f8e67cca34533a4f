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


# ---- the 256-wide fusion layer (DGR's bottleneck PerceiverIO: latent 256, context 128, one head of 128) -------------------------
WIDE_KINDS = ("plain", "rows", "offset", "peaked", "wide_ff")


def wide_case(B, M, T, pe, kind="plain", seed=0):
    """(state dict, queries [B,M,256], context [B,T,128]) in float32 on the host, seeded by the shape.
      plain    N(0, 1) queries and context.
      rows     as plain, with all-zero query rows (the sparse network pads its bottleneck with them: rows 0, 5-8 and the last
               three) and constant rows (12-15; 1.25 + the batch index, exact sums in fp32).
      offset   queries 300 + N(0, 1) (the LayerNorm's cancellation), to_out and the second feed-forward linear x 60 so that
               both branches still stand out of the 300-sized residual.
      peaked   to_q scaled so that a row's scores span ~40 (natural units); one row's best token is moved to the last
               position (the last context tile's only token when T = 32 k + 1).  Needs pe = False.
      wide_ff  the feed-forward's LayerNorm gain x 5: GEGLU gate pre-activations beyond +-6."""
    from gmf_amd import synthetic
    assert kind in WIDE_KINDS and not (kind == "peaked" and pe)
    sd = synthetic.seeded_state_dict(synthetic.fusion_layer_shapes("", 128, 256, 128, pe=pe, out_to_query=True), seed=131 + seed)
    r = np.random.default_rng([137, B, M, T, int(pe), WIDE_KINDS.index(kind), seed])
    x = torch.from_numpy(r.normal(0, 1, (B, M, 256)).astype(np.float32))
    ctx = torch.from_numpy(r.normal(0, 1, (B, T, 128)).astype(np.float32))
    a, f = "cross_attend_blocks.0.", "cross_attend_blocks.1."
    if kind == "rows":
        for i in [0, 5, 6, 7, 8, M - 3, M - 2, M - 1]:
            if 0 <= i < M:
                x[:, i] = 0
        for b in range(B):
            x[b, 12:16] = 1.25 + b
    elif kind == "offset":
        x += 300
        for k in (a + "fn.to_out.weight", a + "fn.to_out.bias", f + "fn.net.2.weight", f + "fn.net.2.bias"):
            sd[k] = sd[k] * 60
    elif kind == "wide_ff":
        sd[f + "norm.weight"] = sd[f + "norm.weight"] * 5
    elif kind == "peaked":
        s = wide_scores(sd_as(sd, torch.float64), x.double(), ctx.double(), False)
        rng = (s.amax(-1) - s.amin(-1)).median().item()
        sd[a + "fn.to_q.weight"] = (sd[a + "fn.to_q.weight"].double() * (40.0 / rng)).float()
        j = int(s[0, 0].argmax())
        if j != T - 1:
            ctx[0, T - 1] = ctx[0, j]
            ctx[0, j] = torch.from_numpy(r.normal(0, 1, 128).astype(np.float32))
    return sd, x, ctx


def wide_scores(sd, x, ctx, pe):
    """softmax argument q Kc^T d^-1/2 [B,M,T] of the cross-attention (natural units)."""
    Kc, _ = ctx_prepare(sd, "", ctx, pe)
    if pe:
        x = O.conv_pos_enc_1(x, sd["cpe.proj_q.weight"], sd["cpe.proj_q.bias"])
    a = "cross_attend_blocks.0."
    q = O.layer_norm(x, sd[a + "norm.weight"], sd[a + "norm.bias"]) @ sd[a + "fn.to_q.weight"].t()
    return (q @ Kc.transpose(-1, -2)) * (q.shape[-1] ** -0.5)


def _row_chunks(M, rows):
    """(lo, hi, a, b): rows [a, b) of the output are rows [a - lo, b - lo) of an evaluation over the queries [lo, hi) - a halo of
    one row on each side, so the LCPE of every kept row sees both of its neighbours (and zero padding only at the ends)."""
    for a in range(0, M, rows):
        b = min(M, a + rows)
        yield max(0, a - 1), min(M, b + 1), a, b


def wide_reference(sd, x, ctx, pe, rows=4096):
    """oracle fusion_layer (depth 0, prefix "") in the dtype of sd / x / ctx, over row chunks of the queries."""
    out = torch.empty_like(x)
    for lo, hi, a, b in _row_chunks(x.shape[1], rows):
        out[:, a:b] = O.fusion_layer(sd, "", ctx, x[:, lo:hi], pe)[:, a - lo:b - lo]
    return out


def wide_branches(sd, x, ctx, pe, rows=4096):
    """From the stage pieces (same function as wide_reference): max |attention branch| (x1 - LCPE(x)), max |feed-forward
    branch| (out - x1), max |GEGLU gate pre-activation|, the per-row argmax token [B,M] and the smallest row score span."""
    Kc, Vc = ctx_prepare(sd, "", ctx, pe)
    f = "cross_attend_blocks.1."
    st = {"attn": 0.0, "ff": 0.0, "gate": 0.0, "span": math.inf}
    arg = torch.empty(x.shape[:2], dtype=torch.long)
    for lo, hi, a, b in _row_chunks(x.shape[1], rows):
        xs = x[:, lo:hi]
        xl = O.conv_pos_enc_1(xs, sd["cpe.proj_q.weight"], sd["cpe.proj_q.bias"]) if pe else xs
        x1 = fusion_attn(sd, "", xs, Kc, Vc, pe)
        y = fusion_ff(sd, "", x1)
        xn = O.layer_norm(x1, sd[f + "norm.weight"], sd[f + "norm.bias"])
        g = (xn @ sd[f + "fn.net.0.weight"].t() + sd[f + "fn.net.0.bias"])[..., 1024:]
        s = wide_scores(sd, xs, ctx, pe)
        k = slice(a - lo, b - lo)
        st["attn"] = max(st["attn"], (x1 - xl)[:, k].abs().max().item())
        st["ff"] = max(st["ff"], (y - x1)[:, k].abs().max().item())
        st["gate"] = max(st["gate"], g[:, k].abs().max().item())
        st["span"] = min(st["span"], (s.amax(-1) - s.amin(-1))[:, k].min().item())
        arg[:, a:b] = s[:, k].argmax(-1)
    st["argmax"] = arg
    return st
