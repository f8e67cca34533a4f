"""CPU: the float64 reference of the 256-wide fusion layer (DGR's bottleneck PerceiverIO) that tests/test_gpu_fusion_wide.py checks
the kernels against, and proof that its accuracy rule (stage_reference.floor_violation) catches plausible kernel bugs at the
shapes that GPU file relies on for each effect."""
import torch
import torch.nn.functional as F

from oracle import gmf_oracle as O

import stage_reference as R

A, FF = "cross_attend_blocks.0.", "cross_attend_blocks.1."


def _lcpe(x, sd, name, drop_tile_last_down=False, replicate=False):
    """conv_pos_enc_1 with two planted mistakes: the last row of every 32-row tile without its lower neighbour (a lost halo row),
    or the sequence padded by replicating its end rows instead of zeros."""
    w, b = sd[name + ".weight"], sd[name + ".bias"]
    if replicate:
        xp = torch.cat([x[:, :1], x, x[:, -1:]], dim=1)
    else:
        xp = F.pad(x, (0, 0, 1, 1))
    dn = xp[:, 2:].clone()
    if drop_tile_last_down:
        dn[:, 31::32] = 0
    return x + b + w[:, 0, 0] * xp[:, :-2] + w[:, 0, 1] * x + w[:, 0, 2] * dn


def _layer(sd, x, ctx, pe, drop_last_token=False, q_tile_halo=False, ctx_replicate=False, tanh_gelu=False):
    """The layer from the stage pieces, with the LCPE, the context and the GELU open to planted mistakes."""
    if pe:
        x = _lcpe(x, sd, "cpe.proj_q", drop_tile_last_down=q_tile_halo)
        ctx = _lcpe(ctx, sd, "cpe.proj_content", replicate=ctx_replicate)
    Kc, Vc = R.ctx_prepare(sd, "", ctx, False)
    if drop_last_token:
        Kc, Vc = Kc[:, :-1], Vc[:, :-1]
    x1 = R.fusion_attn(sd, "", x, Kc, Vc, False)
    xn = O.layer_norm(x1, sd[FF + "norm.weight"], sd[FF + "norm.bias"])
    h = xn @ sd[FF + "fn.net.0.weight"].t() + sd[FF + "fn.net.0.bias"]
    g = h[..., :1024] * F.gelu(h[..., 1024:], approximate="tanh" if tanh_gelu else "none")
    return g @ sd[FF + "fn.net.2.weight"].t() + sd[FF + "fn.net.2.bias"] + x1


def test_wide_reference_chunks_and_pieces_agree():
    """The chunked oracle evaluation (one-row halo per chunk) equals the unchunked one, and the stage pieces compose to the same
    function - at B = 2 with the LCPE, chunk edges inside and at the ends of the sequence."""
    sd, x, ctx = R.wide_case(2, 77, 33, True)
    s64, x64, c64 = R.sd_as(sd, torch.float64), x.double(), ctx.double()
    full = O.fusion_layer(s64, "", c64, x64, True)
    for rows in (1, 2, 32, 76, 4096):
        assert (R.wide_reference(s64, x64, c64, True, rows=rows) - full).abs().max().item() < 1e-12, rows
    assert (_layer(s64, x64, c64, True) - full).abs().max().item() < 1e-12
    st = R.wide_branches(s64, x64, c64, True, rows=10)
    st_full = R.wide_branches(s64, x64, c64, True)
    assert torch.equal(st["argmax"], st_full["argmax"]) and abs(st["attn"] - st_full["attn"]) < 1e-12


def test_floor_rule_rejects_planted_wide_layer_bugs():
    """Each planted mistake, built from the float64 reference itself and rounded to fp32 like a kernel output, breaks the rule
    err <= 2 err_fp32 + 2 eps32 max|ref| at the GPU file's case (B, M, T) = (1, 129, 385) with the LCPE: 13 context tiles, the
    last holding one token; four query tiles, the last holding one row.  The fp32 evaluation itself passes."""
    sd, x, ctx = R.wide_case(1, 129, 385, True)
    s64, x64, c64 = R.sd_as(sd, torch.float64), x.double(), ctx.double()
    ref64 = R.wide_reference(s64, x64, c64, True)
    ref32 = R.wide_reference(R.sd_as(sd, torch.float32), x, ctx, True)
    assert R.floor_violation(ref32, ref64, ref32) is None

    def shifted(key):
        bad = dict(s64)
        bad[key] = torch.roll(s64[key], 32)
        return _layer(bad, x64, c64, True)

    planted = {
        "last context token dropped": _layer(s64, x64, c64, True, drop_last_token=True),
        "query LCPE: a tile's last row without its lower neighbour": _layer(s64, x64, c64, True, q_tile_halo=True),
        "context LCPE: end rows replicated instead of zero padding": _layer(s64, x64, c64, True, ctx_replicate=True),
        "tanh GELU": _layer(s64, x64, c64, True, tanh_gelu=True),
        "to_out bias shifted by a 32-feature block": shifted(A + "fn.to_out.bias"),
        "feed-forward output bias shifted by a 32-feature block": shifted(FF + "fn.net.2.bias"),
    }
    e32, bound = R.floor_bound(ref64, ref32)
    for what, bad in planted.items():
        msg = R.floor_violation(bad.float(), ref64, ref32)
        err = (bad.float().double() - ref64).abs().max().item()
        print(f"{what}: max error {err:.2e} = {err / bound:.0f} x the bound {bound:.2e}")
        assert msg is not None, what
