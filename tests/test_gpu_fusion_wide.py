"""The 256-wide fusion layer (DGR's bottleneck PerceiverIO: latent 256, context 128, one head of 128; gmf_amd/csrc/fusion_wide.hip)
against a float64 evaluation of the oracle's fusion_layer, in every launch form the planner can choose.

Accuracy: err_hip <= 2 err_fp32 + 2 eps32 max|ref| on every valid output element (stage_reference.floor_violation), err_fp32 being
the same oracle evaluated in float32.  The float64 reference is computed once per case; every form of the case is checked
against it:
  h2         split-fp16 context preparation, cross-attention and feed-forward (the module's default), hidden splits automatic;
  fp32_attn  fp32-MFMA context preparation and cross-attention, split-fp16 feed-forward;
  fp32       fp32 MFMA throughout (what ResUNetBN2C runs);
  hs1..hs8   the default form with the feed-forward's hidden splits forced to 1, 2, 4, 8;
  attn4      the default form with the cross-attention forced to one workgroup per four tiles (wide_attn_tile = 0).
The torch profiler's kernel names show that each run took the launch path the host planner (gmf_fusion_layer_forward,
launch_fusion_attn_w_h2, plan_ff_split_w) is meant to choose for its shape, and the automatic hidden split is pinned by bit
identity with the forced run of the planned count.  The cases reach every branch of that planner: see
test_cases_reach_every_planner_branch."""
import contextlib
import re
from collections import Counter

import pytest
import torch

import gmf_amd
from gmf_amd import _lib

import stage_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FORMS = {"h2": (True, True), "fp32_attn": (False, True), "fp32": (False, False)}      # (split_fp16_attn, split_fp16_ff)
WORST = {}                                                                              # form -> (err / bound, case)

# (B, M, T, pe, kind, planned cross-attention kernel of the default form, planned hidden splits)
CASES = [
    # context tiles 1, 2, 3, 4, 10, 13, 33: idle waves of the tile kernel, a one-token last tile (33, 97, 385, 1025), the
    # `wave + 8` tile (300) and the `wave + 12` loop (385, 1025); one to five query tiles, B = 1 and 3
    (1, 1, 1, True, "plain", "tile", 8),
    (1, 1, 1, False, "rows", "tile", 8),
    (3, 31, 33, True, "rows", "tile", 8),
    (1, 32, 33, False, "plain", "tile", 8),
    (1, 33, 65, True, "plain", "tile", 8),
    (3, 33, 65, False, "rows", "tile", 8),
    (3, 129, 97, True, "plain", "tile", 8),
    (1, 32, 97, False, "rows", "tile", 8),
    (1, 129, 300, True, "plain", "tile", 8),
    (3, 33, 300, False, "offset", "tile", 8),
    (1, 129, 33, True, "offset", "tile", 8),
    (1, 129, 385, True, "plain", "tile", 8),
    (3, 31, 385, False, "plain", "tile", 8),
    (1, 129, 1025, True, "rows", "tile", 8),
    (3, 33, 1025, False, "plain", "tile", 8),
    (1, 129, 97, True, "wide_ff", "tile", 8),
    (1, 4000, 385, False, "peaked", "tile", 8),
    # B > 1 at moderate sizes: 273 tiles (4-tile attention, hs 2); 128 tiles (tile attention, hs 8); 132 tiles (hs 4)
    (3, 2900, 97, True, "plain", "h2", 2),
    (4, 1000, 300, False, "rows", "tile", 8),
    (2, 2100, 65, True, "plain", "tile", 4),
    # planner boundaries at B = 1
    (1, 8192, 385, True, "plain", "tile", 4),
    (1, 8193, 300, False, "plain", "h2", 2),
    (1, 16384, 97, True, "plain", "h2", 2),
    (1, 16385, 33, False, "plain", "h2", 1),
    (1, 40000, 65, True, "plain", "h2", 2),
    (1, 50000, 97, False, "plain", "h2", 1),
]


def _tiles(n):
    return (n + 31) // 32


def _plan_hs(base):
    """plan_ff_split_w (fusion_wide.hip) for base = ceil(tiles / 4) * B workgroups."""
    hs = 1
    while hs < 8 and base * hs * 2 <= 256:
        hs *= 2
    return 2 if 256 < base <= 384 else hs


def _expected(B, M, form, hs_knob=0, tile_knob=1):
    """(the gmf kernels one forward launches, with their counts; the hidden splits) as gmf_fusion_layer_forward plans them."""
    h2_attn, h2_ff = FORMS[form]
    tiles = _tiles(M)
    k = Counter({"k_pack_p32": 1 if h2_attn else 2})               # the queries; the context too unless the h2 kernel reads it row-major
    if h2_attn:
        k["k_ctx_prep_w_h2"] += 1
        k["k_fusion_attn_w_tile" if tile_knob and tiles * B <= 256 else "k_fusion_attn_w_h2"] += 1
    else:
        k["k_ctx_prep_w"] += 1
        k["k_fusion_attn_w"] += 1
    hs = 1
    if h2_ff:
        hs = hs_knob if hs_knob else _plan_hs(((tiles + 3) // 4) * B)
        k["k_fusion_ff_w_h2"] += 1
        k["k_ff_reduce_w" if hs > 1 else "k_unpack_p32"] += 1     # the reduction writes the caller's tensor itself
    else:
        k["k_fusion_ff_w"] += 1
        k["k_unpack_p32"] += 1
    return k, hs


_KERNEL = re.compile(r"gmf::(?:\(anonymous namespace\)::)?(k_\w+)")


def _launched(fn):
    """(fn(), Counter of the gmf kernels it launched, by exact name)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = Counter()
    for e in prof.key_averages():
        m = _KERNEL.search(e.key)
        if m and e.device_time_total > 0:
            names[m.group(1)] += e.count
    return out, names


@contextlib.contextmanager
def _tuning(ff_hidden_splits=0, wide_attn_tile=1):
    h = _lib.handle_for(0)
    try:
        h.call("gmf_set_tuning", b"ff_hidden_splits", ff_hidden_splits)
        h.call("gmf_set_tuning", b"wide_attn_tile", wide_attn_tile)
        yield
    finally:
        h.call("gmf_set_tuning", b"ff_hidden_splits", 0)
        h.call("gmf_set_tuning", b"wide_attn_tile", 1)


def _module(sd, pe):
    m = gmf_amd.PerceiverIO(depth=0, dim=128, latent_dim=256, cross_heads=1, cross_dim_head=128, pe=pe)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m._blobs(torch.device(DEV))                       # packed (and placed) before any profiled forward
    return m


def _form(m, form):
    m.split_fp16_attn, m.split_fp16_ff = FORMS[form]
    return m


def _check(got, ref64, ref32, form, what):
    bound = R.floor_bound(ref64, ref32)[1]
    msg = R.floor_violation(got, ref64, ref32)
    assert msg is None, f"{what} [{form}]: {msg}"
    ratio = (got.detach().cpu().double() - ref64).abs().max().item() / bound
    if ratio >= WORST.get(form, (-1.0, ""))[0]:
        WORST[form] = (ratio, what)


def _case_id(c):
    B, M, T, pe, kind = c[:5]
    return f"B{B}-M{M}-T{T}-{'pe' if pe else 'nope'}-{kind}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_wide_layer_against_float64(case):
    B, M, T, pe, kind, attn_plan, hs_plan = case
    what = _case_id(case)
    sd, x, ctx = R.wide_case(B, M, T, pe, kind)
    s64, x64, c64 = R.sd_as(sd, torch.float64), x.double(), ctx.double()
    ref64 = R.wide_reference(s64, x64, c64, pe)
    ref32 = R.wide_reference(R.sd_as(sd, torch.float32), x, ctx, pe)
    st = R.wide_branches(s64, x64, c64, pe)
    # the inputs make both branches and the case's own effect visible
    top = ref64.abs().max().item()
    assert st["attn"] >= 0.05 * top and st["ff"] >= 0.05 * top, (st["attn"], st["ff"], top)
    if kind == "wide_ff":
        assert st["gate"] > 8, st["gate"]
    if kind == "peaked":
        assert st["span"] > 20, st["span"]
        waves = {int(t) % 4 for t in (st["argmax"] // 32).flatten()}
        assert waves == {0, 1, 2, 3} and (st["argmax"] == T - 1).any(), (waves, T)

    m = _module(sd, pe)
    xd, cd = x.to(DEV), ctx.to(DEV)
    e, hs = _expected(B, M, "h2")
    assert (e["k_fusion_attn_w_tile"] == 1) == (attn_plan == "tile") and hs == hs_plan, (e, hs)
    outs = {}
    for form in FORMS:
        with _tuning():
            out, got = _launched(lambda: _form(m, form)(cd, queries_encoder=xd))
        assert got == _expected(B, M, form)[0], (form, got)
        _check(out, ref64, ref32, form, what)
        outs[form] = out
    _form(m, "h2")
    forced = {}
    for k in (1, 2, 4, 8):
        with _tuning(ff_hidden_splits=k):
            forced[k], got = _launched(lambda: m(cd, queries_encoder=xd))
        assert got == _expected(B, M, "h2", hs_knob=k)[0], (k, got)
        _check(forced[k], ref64, ref32, f"hs{k}", what)
    # the automatic choice is the planned count: bit-identical to that forced run and to no other
    assert [k for k in forced if torch.equal(forced[k], outs["h2"])] == [hs_plan]
    with _tuning(wide_attn_tile=0):
        out, got = _launched(lambda: m(cd, queries_encoder=xd))
    assert got == _expected(B, M, "h2", tile_knob=0)[0], got
    _check(out, ref64, ref32, "attn4", what)
    gmf_amd.check_status()


def test_cases_reach_every_planner_branch():
    """The case table reaches every decision of the planner (and the profiler checks above hold each case to it)."""
    attn, hs_auto, tile_waves = set(), set(), set()
    for B, M, T, pe, kind, attn_plan, hs_plan in CASES:
        hs = _expected(B, M, "h2")[1]
        attn.add((attn_plan, B > 1))
        base = ((_tiles(M) + 3) // 4) * B
        hs_auto.add((hs, "second round" if 256 < base <= 384 else ("base >= 385" if base >= 385 else "")))
        if attn_plan == "tile":
            tt = _tiles(T)
            tile_waves |= {"idle waves"} if tt < 4 else set()
            tile_waves |= {"wave + 8"} if tt > 8 else set()
            tile_waves |= {"wave + 12 loop"} if tt > 12 else set()
            tile_waves |= {"one-token last tile"} if T % 32 == 1 else set()
    assert attn >= {("tile", False), ("tile", True), ("h2", False), ("h2", True)}, attn
    assert hs_auto >= {(8, ""), (4, ""), (2, ""), (1, ""), (2, "second round"), (1, "base >= 385")}, hs_auto
    assert tile_waves == {"idle waves", "wave + 8", "wave + 12 loop", "one-token last tile"}, tile_waves
    for pe in (True, False):
        assert {_tiles(c[2]) for c in CASES if c[3] == pe} >= {1, 2, 3, 4, 10, 13, 33}, pe


def _abi_forward(m, ctx, x, out, pe):
    """gmf_fusion_layer_forward straight through the C ABI with the module's blobs, into `out` at its own strides."""
    b = m._blobs(torch.device(DEV))
    B, N, _ = x.shape
    h2_attn = m.split_fp16_attn and b.attn_wst_h2
    _lib.handle_for(0).call("gmf_fusion_layer_forward", 1 if pe else 0, b.latent_dim, b.d_head, b.ctx_wst, b.ctx_vec, b.attn_wst,
                            b.attn_vec, b.ff_wst, b.ff_vec, ctx.data_ptr(), x.data_ptr(), *x.stride(), out.data_ptr(), *out.stride(),
                            B, N, ctx.shape[1], torch.cuda.current_stream().cuda_stream,
                            b.ff_wst_h2 if m.split_fp16_ff else None, *((b.ctx_wst_h2, b.attn_wst_h2) if h2_attn else (None, None)))


@pytest.mark.parametrize("B,M,T", [(3, 100, 65), (3, 2900, 33)])
def test_strided_output_and_queries(B, M, T):
    """The caller's output through non-contiguous strides (a transposed view with gaps in a NaN-filled buffer) on both kernels
    that write it - k_ff_reduce_w (hidden-split feed-forward) and k_unpack_p32 - and strided queries: bit-identical to the
    contiguous call, nothing outside the view written."""
    sd, x, ctx = R.wide_case(B, M, T, True)
    m = _module(sd, True)
    xd, cd = x.to(DEV), ctx.to(DEV)
    for form, hs, writer in (("h2", 0, "k_ff_reduce_w"), ("h2", 1, "k_unpack_p32"), ("fp32", 0, "k_unpack_p32")):
        _form(m, form)
        with _tuning(ff_hidden_splits=hs):
            ref = m(cd, queries_encoder=xd)
            buf = torch.full((B, 300, M + 9), NAN, device=DEV)
            view = buf[:, 20:276, 5:5 + M].transpose(1, 2)
            assert view.shape == (B, M, 256) and view.stride() == (300 * (M + 9), 1, M + 9)
            _, got = _launched(lambda: _abi_forward(m, cd, xd, view, True))
            assert got[writer] == 1, (form, hs, got)
            assert torch.equal(view, ref), (form, hs)
            outside = torch.ones_like(buf, dtype=torch.bool)
            outside[:, 20:276, 5:5 + M] = False
            assert torch.isnan(buf[outside]).all(), (form, hs)
            # strided queries: a permuted copy and a gapped slice
            xt = xd.permute(0, 2, 1).contiguous().permute(0, 2, 1)
            xg = torch.full((B, M + 5, 300), NAN, device=DEV)
            xg[:, 3:3 + M, 10:266] = xd
            for q in (xt, xg[:, 3:3 + M, 10:266]):
                assert torch.equal(m(cd, queries_encoder=q), ref), (form, hs, q.stride())
    gmf_amd.check_status()


@pytest.mark.parametrize("form,hs,last", [("fp32", 0, "k_unpack_p32"), ("h2", 1, "k_unpack_p32"), ("h2", 0, "k_ff_reduce_w")])
def test_status_word_on_every_feed_forward_form(form, hs, last):
    """A NaN in one query row (of the second pair) reaches the output; the kernel that writes it flags the handle's status word,
    check_status() raises, and the next clean forward leaves the word clear."""
    sd, x, ctx = R.wide_case(2, 200, 50, True)
    m = _form(_module(sd, True), form)
    xd, cd = x.to(DEV), ctx.to(DEV)
    with _tuning(ff_hidden_splits=hs):
        _, got = _launched(lambda: m(cd, queries_encoder=xd))
        assert got[last] == 1, got
        gmf_amd.check_status()
        bad = xd.clone()
        bad[1, 137, 3] = NAN
        y = m(cd, queries_encoder=bad)
        with pytest.raises(RuntimeError, match="non-finite"):
            gmf_amd.check_status()
        assert torch.isnan(y[1, 137]).any() and torch.isfinite(y[0]).all()
        y = m(cd, queries_encoder=xd)
        gmf_amd.check_status()
        assert torch.isfinite(y).all()


def test_fp16_range_fallback():
    """A dense weight beyond the split-fp16 range (|256 w| > 65504) makes the packer drop the split images with a warning; the
    layer then runs its fp32-MFMA kernels and meets the same rule."""
    B, M, T = 2, 129, 97
    sd, x, ctx = R.wide_case(B, M, T, True)
    key = "cross_attend_blocks.1.fn.net.2.weight"
    sd[key] = sd[key].clone()
    sd[key][3, 5] = 300.0
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        m = _module(sd, True)                                         # (packs the blobs)
    blobs = m._blobs(torch.device(DEV))
    assert not blobs.split_fp16 and not blobs.ff_wst_h2 and not blobs.attn_wst_h2
    assert m.split_fp16_attn and m.split_fp16_ff                      # the module asks for split-fp16; the blobs decide
    out, got = _launched(lambda: m(ctx.to(DEV), queries_encoder=x.to(DEV)))
    assert got == _expected(B, M, "fp32")[0], got
    ref64 = R.wide_reference(R.sd_as(sd, torch.float64), x.double(), ctx.double(), True)
    ref32 = R.wide_reference(R.sd_as(sd, torch.float32), x, ctx, True)
    _check(out, ref64, ref32, "fp32 (fallback)", "fp16-range fallback")
    gmf_amd.check_status()


def test_report_worst_ratios():
    """Prints the worst err_hip / bound of every form over the cases run in this session."""
    for form, (ratio, what) in sorted(WORST.items()):
        print(f"{form:>16}: worst err / bound {ratio:.3f} ({what})")
    assert all(r <= 1.0 for r, _ in WORST.values())
