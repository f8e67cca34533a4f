"""The staged encoder entry points of the C ABI (gmf_hip.h, "layout conversion" and "encoder stages"), each against a float64
restatement built from the oracle's pieces (tests/stage_reference.py).

Accuracy: err_hip <= 2 err_fp32 + 2 eps32 max|ref|, err_fp32 being the same restatement evaluated in float32.  Every output
buffer is filled with NaN before a call: the valid rows must be finite and within the rule, and the padding rows (>= N) that a
later stage reads must be finite.  A second call whose input images carry NaN in their padding rows shows that no valid row
reads them (the LCPE at the last valid row included).  Finally the stages, composed into NonLocalNet + classifier, equal the
whole forward bit for bit on the handle's fp32 plan ("scattn_variant" 0)."""
import ctypes

import numpy as np
import pytest
import torch

import gmf_amd
from gmf_amd import _lib, packing, synthetic
from oracle import gmf_oracle as O

import stage_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_W = 3                     # layers of the per-stage weights (ctx_prepare reads three weight sets at their strides)
NAN = float("nan")
F2 = "encoder.blocks.NonLocal_layer_{}.fusion_layer_2."
F1 = "encoder.fusion_layer_1."


def _tiles(n):
    return (n + 31) // 32


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _h():
    return _lib.handle_for(0), torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr()


@pytest.fixture(scope="module")
def W():
    """(fp32 state dict, its float64 / float32 copies, the fp32 blobs of the pure-Python packers on the device)."""
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, L_W, 128), seed=11)
    blobs, _ = packing.python_packed_encoder(sd, L_W)
    dev = {k: v.to(DEV).contiguous() for k, v in blobs.items()}
    return sd, R.sd_as(sd, torch.float64), R.sd_as(sd, torch.float32), dev


def _scene(B, N, T, seed0=300):
    return synthetic.synthetic_batch([seed0 + i for i in range(B)], N=N, T=T)


def _feat0(sd64, corr):
    """layer0(corr_pos) in float64, rounded: realistic input features of a PointCN (signed, O(1))."""
    return O._lin(corr.double(), sd64["encoder.layer0.weight"], sd64["encoder.layer0.bias"]).float()


def _img_p32(X, pad_nan=False):
    """Row-major [B, N, K] (host) -> P32 image on the device; padding rows zero (as gmf_pack_rows_p32 writes them) or NaN."""
    img = packing.rows_p32(X).reshape(X.shape[0], -1, X.shape[-1])
    if pad_nan:
        img = img.clone()
        pad = packing.rows_p32(torch.ones_like(X)).reshape(img.shape) == 0
        img[pad] = NAN
    return img.reshape(-1).to(DEV)


def _rows(img, B, N, K, timg=False):
    """Image on the device -> (valid rows [B, N, K], padding rows [B, Npad - N, K]) on the host, decoded in Python."""
    x = img.detach().cpu().reshape(B, -1)
    full = packing.untimg(x, _tiles(N) * 32, K) if timg else packing.unrows_p32(x, _tiles(N) * 32, K)
    return full[:, :N], full[:, N:]


def _assert_pad_finite(pad, what):
    assert torch.isfinite(pad).all(), f"{what}: a padding row read by a later stage is not finite"


# ---- gmf_pack_pts8 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 31, 32, 33, 1000])
def test_pack_pts8(N):
    h, st = _h()
    B = 3
    b = _scene(B, N, 1)
    src, tgt = b["src_keypts"].to(DEV), b["tgt_keypts"].to(DEV)
    Np = _tiles(N) * 32
    out = _nan(B, Np, 8)
    h.call("gmf_pack_pts8", _p(src), _p(tgt), B, N, _p(out), st)
    ref = torch.zeros(B, Np, 8)
    ref[:, :N, 0:3] = b["src_keypts"]
    ref[:, :N, 4:7] = b["tgt_keypts"]
    assert torch.equal(out.cpu().view(torch.int32), ref.view(torch.int32))


# ---- gmf_front_forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [1, 0])
@pytest.mark.parametrize("B,N", [(1, 1), (2, 31), (3, 33), (2, 257), (1, 1000)])
def test_front_forward(W, first, B, N):
    """first = 1: layer0 + PointCN_0 + Q'/K/V from row-major corr_pos; first = 0: PointCN_1 + Q'/K/V from a P32 feature image.
    f, Q', K read back through gmf_unpack_rows_p32, V through the T image's definition (packing.untimg)."""
    sd, sd64, sd32, t = W
    h, st = _h()
    layer = 0 if first else 1
    b = _scene(B, N, 1)
    x32 = b["corr_pos"] if first else _feat0(sd64, b["corr_pos"])
    ref64 = R.front(sd64, layer, x32.double(), first)
    ref32 = R.front(sd32, layer, x32, first)
    act = B * _tiles(N) * 32 * 128

    def run(pad_nan):
        inp = x32.to(DEV).contiguous() if first else _img_p32(x32, pad_nan)
        outs = [_nan(act) for _ in range(4)]
        h.call("gmf_front_forward", first, _p(inp), _p(t["front_wst"][layer]), _p(t["front_vec"][layer]), *map(_p, outs), B, N, st)
        return outs

    outs = run(False)
    for name, img, r64, r32 in zip("fqk", outs[:3], ref64[:3], ref32[:3]):
        got = _nan(B, N, 128)
        h.call("gmf_unpack_rows_p32", _p(img), B, N, 128, _p(got), N * 128, 128, 1, st)
        R.assert_floor(got, r64, r32, f"front {name}")
        _assert_pad_finite(_rows(img, B, N, 128)[1], f"front {name}")
    v, vpad = _rows(outs[3], B, N, 128, timg=True)
    R.assert_floor(v, ref64[3], ref32[3], "front v")
    _assert_pad_finite(vpad, "front v")
    if not first:
        # NaN in the input image's padding rows reaches no valid row
        again = run(True)
        for name, a, b_, ti in zip("fqkv", outs, again, (False, False, False, True)):
            assert torch.equal(_rows(a, B, N, 128, ti)[0], _rows(b_, B, N, 128, ti)[0]), name


# ---- gmf_scattn_forward / gmf_scattn_forward_dense -------------------------------------------------------------------------
def _pts8(src, tgt):
    B, N, _ = src.shape
    out = torch.zeros(B, _tiles(N) * 32, 8)
    out[:, :N, 0:3], out[:, :N, 4:7] = src, tgt
    return out


def _scattn_inputs(sd64, b, layer, seed):
    """fp64-derived, fp32-rounded Q', K, V (front of the scene's layer0 features) and a Fusion-2 output."""
    f0 = _feat0(sd64, b["corr_pos"])
    _, q, k, v = (y.float() for y in R.front(sd64, layer, f0.double(), False))
    g = torch.Generator().manual_seed(seed)
    fus = torch.randn(q.shape, generator=g)
    return q, k, v, fus


def _scattn_refs(sd64, sd32, layer, q, k, v, fus, compat64, compat32):
    ref64 = R.scattn(sd64, layer, q.double(), k.double(), v.double(), compat64, fus.double())
    ref32 = R.scattn(sd32, layer, q, k, v, compat32, fus)
    return ref64, ref32


def _run_scattn(t, layer, q, k, v, fus, B, N, pts8=None, dense=None, sigma_d=None, pad_nan=False):
    h, st = _h()
    imgs = [_img_p32(q, pad_nan), _img_p32(k, pad_nan), packing.timg(v).reshape(-1).to(DEV), _img_p32(fus, pad_nan)]
    out = _nan(B * _tiles(N) * 32 * 128)
    if dense is None:
        p8 = pts8.clone()
        if pad_nan:
            p8[:, N:] = NAN
        p8 = p8.to(DEV)
        h.call("gmf_scattn_forward", *map(_p, imgs[:3]), _p(p8), _p(imgs[3]), _p(t["tail_wst"][layer]), _p(t["tail_vec"][layer]),
               _p(out), B, N, sigma_d, st)
    else:
        d = dense.to(DEV).contiguous()
        h.call("gmf_scattn_forward_dense", *map(_p, imgs[:3]), _p(d), _p(imgs[3]), _p(t["tail_wst"][layer]),
               _p(t["tail_vec"][layer]), _p(out), B, N, st)
    return out


@pytest.mark.parametrize("kind,B,N,sigma_d", [(kind, B, N, s) for kind, B, N in [
    ("scene", 2, 1), ("scene", 2, 33), ("scene", 2, 257), ("scene", 2, 1000), ("diagonal", 2, 70), ("identical", 2, 70)]
    for s in (0.10, 1.2)] + [("scene", 1, 5000, 0.10)])
def test_scattn_forward(W, kind, B, N, sigma_d):
    """Compat matrix recomputed in-kernel from pts8.  "diagonal": points spread so that every c_ij = 0 but the diagonal
    (ds - dt = -10 |i - j|); "identical": every point the same, c = 1 everywhere (plain softmax)."""
    sd, sd64, sd32, t = W
    layer = 1
    sigma_d = float(np.float32(sigma_d))            # the value the kernel receives
    b = _scene(B, N, 1)
    src, tgt = b["src_keypts"].clone(), b["tgt_keypts"].clone()
    if kind == "diagonal":
        i = torch.arange(N, dtype=torch.float32)
        src = torch.zeros(B, N, 3)
        tgt = torch.zeros(B, N, 3)
        src[..., 0], tgt[..., 0] = 10 * i, 20 * i
    elif kind == "identical":
        src = torch.full((B, N, 3), 0.75)
        tgt = torch.full((B, N, 3), -1.25)
    q, k, v, fus = _scattn_inputs(sd64, b, layer, seed=N)
    c64 = O.compat_matrix(src.double(), tgt.double(), sigma_d)[0]
    c32 = O.compat_matrix(src, tgt, np.float32(sigma_d))[0]
    if kind == "diagonal":
        assert torch.equal(c64, torch.eye(N, dtype=torch.float64).expand(B, N, N))
    if kind == "identical":
        assert bool((c64 == 1).all())
    ref64, ref32 = _scattn_refs(sd64, sd32, layer, q, k, v, fus, c64, c32)
    pts8 = _pts8(src, tgt)
    out = _run_scattn(t, layer, q, k, v, fus, B, N, pts8=pts8, sigma_d=sigma_d)
    got, pad = _rows(out, B, N, 128)
    R.assert_floor(got, ref64, ref32, f"scattn {kind} sigma_d={sigma_d}")
    _assert_pad_finite(pad, "scattn out")
    # NaN in the padding rows of Q', K, pts8 and fusion2_out reaches no valid row (V's padding rows meet P = 0: they must be
    # finite, which gmf_front_forward guarantees)
    again = _run_scattn(t, layer, q, k, v, fus, B, N, pts8=pts8, sigma_d=sigma_d, pad_nan=True)
    assert torch.equal(_rows(again, B, N, 128)[0], got)


@pytest.mark.parametrize("B,N", [(2, 33), (1, 257), (2, 1000)])
def test_scattn_forward_dense(W, B, N):
    """(a) the oracle's compat matrix given densely agrees with the in-kernel recomputation of gmf_scattn_forward;
    (b) a caller's matrix - not symmetric, values in [-1, 2], some all-zero rows - is used as given."""
    sd, sd64, sd32, t = W
    layer = 2
    sigma_d = float(sd["sigma_spat"])
    b = _scene(B, N, 1)
    q, k, v, fus = _scattn_inputs(sd64, b, layer, seed=N + 1)
    src, tgt = b["src_keypts"], b["tgt_keypts"]
    c64 = O.compat_matrix(src.double(), tgt.double(), sigma_d)[0]
    c32 = O.compat_matrix(src, tgt, np.float32(sigma_d))[0]
    ref64, ref32 = _scattn_refs(sd64, sd32, layer, q, k, v, fus, c64, c32)
    dense, _ = _rows(_run_scattn(t, layer, q, k, v, fus, B, N, dense=c64.float()), B, N, 128)
    recomp, _ = _rows(_run_scattn(t, layer, q, k, v, fus, B, N, pts8=_pts8(src, tgt), sigma_d=sigma_d), B, N, 128)
    R.assert_floor(dense, ref64, ref32, "scattn dense (oracle compat)")
    _, bound = R.floor_bound(ref64, ref32)
    assert (dense.double() - recomp.double()).abs().max().item() <= bound
    # (b)
    g = torch.Generator().manual_seed(N)
    A = torch.rand(B, N, N, generator=g) * 3 - 1
    A[:, ::7] = 0                                             # all-zero rows: uniform attention over the pair's keys
    assert not torch.equal(A, A.transpose(1, 2)) or N == 1
    ref64, ref32 = _scattn_refs(sd64, sd32, layer, q, k, v, fus, A.double(), A)
    out = _run_scattn(t, layer, q, k, v, fus, B, N, dense=A)
    got, pad = _rows(out, B, N, 128)
    R.assert_floor(got, ref64, ref32, "scattn dense (caller matrix)")
    _assert_pad_finite(pad, "scattn dense out")


# ---- gmf_fusion_ctx_prepare ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sets", [1, 3])
@pytest.mark.parametrize("T", [1, 33, 196, 300])
@pytest.mark.parametrize("pe", [0, 1])
def test_fusion_ctx_prepare(W, pe, T, sets):
    """out [sets, B, Tt, 4096] = per 32-token tile Kc as P32 (K = 64) | Vc as T image (D = 64).  sets = 1: Fusion-1's weights
    (pe = 0) or layer 0's Fusion-2 (pe = 1); sets = 3: the Fusion-2 weights of three layers at their strides."""
    sd, sd64, sd32, t = W
    h, st = _h()
    B = 2
    ctx = _scene(B, 8, T)["p_tokens"]
    tt = _tiles(T)
    if sets == 1 and pe == 0:
        prefixes, wst, vec, ws, vs = [F1], t["f1_ctx_wst"], t["f1_ctx_vec"], 0, 0
    else:
        prefixes = [F2.format(s) for s in range(sets)]
        wst, vec, ws, vs = t["ctx_wst"], t["ctx_vec"], packing.CTX_WST, packing.CTX_VEC

    def run(pad_nan):
        inp = _img_p32(ctx, pad_nan)
        out = _nan(sets, B, tt, 4096)
        h.call("gmf_fusion_ctx_prepare", pe, _p(inp), _p(wst), _p(vec), _p(out), B, T, sets, ws, vs, st)
        return out.cpu()

    out = run(False)
    Kc, Vc = packing.split_ctx_image(out, tt * 32)
    for s, pre in enumerate(prefixes):
        k64, v64 = R.ctx_prepare(sd64, pre, ctx.double(), pe)
        k32, v32 = R.ctx_prepare(sd32, pre, ctx, pe)
        R.assert_floor(Kc[s, :, :T], k64, k32, f"ctx_prepare Kc set {s}")
        R.assert_floor(Vc[s, :, :T], v64, v32, f"ctx_prepare Vc set {s}")
    _assert_pad_finite(Kc[:, :, T:], "ctx_prepare Kc")
    _assert_pad_finite(Vc[:, :, T:], "ctx_prepare Vc")
    K2, V2 = packing.split_ctx_image(run(True), T)
    assert torch.equal(K2, Kc[:, :, :T]) and torch.equal(V2, Vc[:, :, :T])


# ---- gmf_fusion_attn_forward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 33, 196, 300])
@pytest.mark.parametrize("N", [1, 31, 33, 257, 1000])
@pytest.mark.parametrize("pe", [0, 1])
def test_fusion_attn_forward(W, pe, N, T):
    """[LCPE] + LayerNorm + to_q + softmax + to_out + the residual on the LCPE'd x, against a context image built from the
    fp64 context side (pe = 0: Fusion-1 on the query tokens; pe = 1: layer 1's Fusion-2 on PointCN features)."""
    sd, sd64, sd32, t = W
    h, st = _h()
    B = 2
    b = _scene(B, N, T)
    if pe:
        pre, wst, vec = F2.format(1), t["attn_wst"][1], t["attn_vec"][1]
        x = torch.relu(_feat0(sd64, b["corr_pos"]))
    else:
        pre, wst, vec = F1, t["f1_attn_wst"], t["f1_attn_vec"]
        x = synthetic.synthetic_tokens(900 + N, N)[1]
        x = torch.from_numpy(np.stack([x, synthetic.synthetic_tokens(901 + N, N)[1]]))
    Kc, Vc = (y.float() for y in R.ctx_prepare(sd64, pre, b["p_tokens"].double(), pe))
    ctx = packing.ctx_image(Kc, Vc).reshape(-1).to(DEV)
    ref64 = R.fusion_attn(sd64, pre, x.double(), Kc.double(), Vc.double(), pe)
    ref32 = R.fusion_attn(sd32, pre, x, Kc, Vc, pe)

    def run(pad_nan):
        out = _nan(B * _tiles(N) * 32 * 128)
        h.call("gmf_fusion_attn_forward", pe, _p(_img_p32(x, pad_nan)), _p(ctx), _p(wst), _p(vec), _p(out), B, N, T, st)
        return out

    got, pad = _rows(run(False), B, N, 128)
    R.assert_floor(got, ref64, ref32, f"fusion_attn pe={pe} N={N} T={T}")
    _assert_pad_finite(pad, "fusion_attn x1")
    assert torch.equal(_rows(run(True), B, N, 128)[0], got)      # the LCPE's last valid row reads no padding row


# ---- gmf_fusion_ff_forward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(4, 1), (2, 33), (3, 1000)])
def test_fusion_ff_forward(W, B, N):
    """N = 1 at B = 4: the fp32 restatement's error over a single row's 128 outputs is too small a sample for the floor."""
    sd, sd64, sd32, t = W
    h, st = _h()
    pre = F2.format(2)
    x1 = _feat0(sd64, _scene(B, N, 1)["corr_pos"])
    ref64 = R.fusion_ff(sd64, pre, x1.double())
    ref32 = R.fusion_ff(sd32, pre, x1)

    def run(pad_nan):
        out = _nan(B * _tiles(N) * 32 * 128)
        h.call("gmf_fusion_ff_forward", _p(_img_p32(x1, pad_nan)), _p(t["ff_wst"][2]), _p(t["ff_vec"][2]), _p(out), B, N, st)
        return out

    got, pad = _rows(run(False), B, N, 128)
    R.assert_floor(got, ref64, ref32, "fusion_ff")
    _assert_pad_finite(pad, "fusion_ff x2")
    assert torch.equal(_rows(run(True), B, N, 128)[0], got)


# ---- gmf_classifier_forward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 1), (2, 33), (3, 1000)])
def test_classifier_forward(W, B, N):
    """logits, feat_n (unit rows) and feat (the rows as given) row-major; feat may be NULL; NaN in a valid row sets
    GMF_STATUS_NONFINITE, NaN in padding rows only sets nothing and leaves every logit finite."""
    sd, sd64, sd32, t = W
    h, st = _h()
    feat = _feat0(sd64, _scene(B, N, 1)["corr_pos"])
    lg64, fn64 = R.classifier(sd64, feat.double())
    lg32, fn32 = R.classifier(sd32, feat)

    def run(img, with_feat=True):
        lg, fn, fr = _nan(B, N), _nan(B, N, 128), _nan(B, N, 128)
        h.call("gmf_classifier_forward", _p(img), _p(t["head_wst"]), _p(t["head_vec"]), _p(lg), _p(fn),
               _p(fr) if with_feat else None, B, N, st)
        return lg.cpu(), fn.cpu(), fr.cpu()

    torch.cuda.synchronize()
    h.status(clear=True)
    try:
        lg, fn, fr = run(_img_p32(feat))
        R.assert_floor(lg, lg64, lg32, "classifier logits")
        R.assert_floor(fn, fn64, fn32, "classifier feat_n")
        assert torch.equal(fr, feat)
        lg2, fn2, fr2 = run(_img_p32(feat), with_feat=False)
        assert torch.equal(lg2, lg) and torch.equal(fn2, fn) and bool(torch.isnan(fr2).all())
        torch.cuda.synchronize()
        assert h.status() & _lib.GMF_STATUS_NONFINITE == 0
        if N % 32:
            lg3, fn3, _ = run(_img_p32(feat, pad_nan=True))
            torch.cuda.synchronize()
            assert h.status() & _lib.GMF_STATUS_NONFINITE == 0
            assert bool(torch.isfinite(lg3).all()) and torch.equal(lg3, lg) and torch.equal(fn3, fn)
        # NaN in the last valid row: the word is set, that row's feat_n is zero (the pose head derives indices from it), feat
        # carries the NaN, and no other row changes
        bad = feat.clone()
        bad[B - 1, N - 1, 77] = NAN
        lg4, fn4, fr4 = run(_img_p32(bad))
        torch.cuda.synchronize()
        assert h.status(clear=True) & _lib.GMF_STATUS_NONFINITE
        assert h.status() & _lib.GMF_STATUS_NONFINITE == 0
        assert torch.equal(fn4[B - 1, N - 1], torch.zeros(128)) and torch.isnan(fr4[B - 1, N - 1, 77])
        assert torch.equal(lg4.reshape(-1)[:-1], lg.reshape(-1)[:-1])
        assert torch.equal(fn4.reshape(B * N, 128)[:-1], fn.reshape(B * N, 128)[:-1])
    finally:
        torch.cuda.synchronize()
        h.status(clear=True)


# ---- argument checks -------------------------------------------------------------------------------------------------------
def _arg_table(p, st):
    """name -> (valid arguments after the handle, positions of pointer arguments, positions of B / N / T / sets)."""
    return {
        "gmf_pack_pts8": ([p, p, 1, 1, p, st], [0, 1, 4], [2, 3]),
        "gmf_front_forward": ([1, p, p, p, p, p, p, p, 1, 1, st], [1, 2, 3, 4, 5, 6, 7], [8, 9]),
        "gmf_scattn_forward": ([p] * 8 + [1, 1, 0.1, st], list(range(8)), [8, 9]),
        "gmf_scattn_forward_dense": ([p] * 8 + [1, 1, st], list(range(8)), [8, 9]),
        "gmf_fusion_ctx_prepare": ([1, p, p, p, p, 1, 1, 1, 0, 0, st], [1, 2, 3, 4], [5, 6, 7]),
        "gmf_fusion_attn_forward": ([1, p, p, p, p, p, 1, 1, 1, st], [1, 2, 3, 4, 5], [6, 7, 8]),
        "gmf_fusion_ff_forward": ([p, p, p, p, 1, 1, st], [0, 1, 2, 3], [4, 5]),
        "gmf_classifier_forward": ([p, p, p, p, p, None, 1, 1, st], [0, 1, 2, 3, 4], [6, 7]),
    }


def test_stage_argument_checks():
    """A null pointer is GMF_ERR_BAD_ARG, an empty shape GMF_ERR_UNSUPPORTED_SHAPE, sigma_d <= 0 (or NaN) GMF_ERR_BAD_ARG; the
    message names the entry point.  Nothing is launched (the buffer behind the pointers is never touched)."""
    h, st = _h()
    lib = h.lib
    buf = torch.zeros(64, device=DEV)
    torch.cuda.synchronize()
    for name, (args, ptrs, shapes) in _arg_table(_p(buf), st).items():
        fn = getattr(lib, name)
        short = name[len("gmf_"):]
        for i in ptrs:
            a = list(args)
            a[i] = None
            assert fn(h.h, *a) == -1, (name, i)
            assert short + ":" in lib.gmf_last_error_string(h.h).decode(), name
        for i in shapes:
            a = list(args)
            a[i] = 0
            assert fn(h.h, *a) == -2, (name, i)
            assert short + ":" in lib.gmf_last_error_string(h.h).decode(), name
        assert fn(None, *args) == -1, name
    args = _arg_table(_p(buf), st)["gmf_scattn_forward"][0]
    for bad in (0.0, -0.1, NAN):
        a = list(args)
        a[10] = bad
        assert lib.gmf_scattn_forward(h.h, *a) == -1, bad
        assert "scattn_forward" in lib.gmf_last_error_string(h.h).decode() and "sigma_d" in lib.gmf_last_error_string(h.h).decode()
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), torch.zeros(64))


# ---- composed forward ------------------------------------------------------------------------------------------------------
def _composed(t, b, L, sigma_d):
    """NonLocalNet + classifier from the stage entry points alone, every buffer NaN-filled: the kFp32 plan of gmf_api.cpp."""
    h, st = _h()
    d = {k: v.to(DEV).contiguous() for k, v in b.items()}
    B, N, _ = d["corr_pos"].shape
    T = d["p_tokens"].shape[1]
    tt, act = _tiles(T), B * _tiles(N) * 32 * 128
    tok = B * tt * 4096
    pimg, qimg, f1ctx, x1t, imgfeat = (_nan(tok) for _ in range(5))
    for src, dst in ((d["p_tokens"], pimg), (d["q_tokens"], qimg)):
        h.call("gmf_pack_rows_p32", _p(src), T * 128, 128, 1, B, T, 128, _p(dst), st)
    h.call("gmf_fusion_ctx_prepare", 0, _p(pimg), _p(t["f1_ctx_wst"]), _p(t["f1_ctx_vec"]), _p(f1ctx), B, T, 1, 0, 0, st)
    h.call("gmf_fusion_attn_forward", 0, _p(qimg), _p(f1ctx), _p(t["f1_attn_wst"]), _p(t["f1_attn_vec"]), _p(x1t), B, T, T, st)
    h.call("gmf_fusion_ff_forward", _p(x1t), _p(t["f1_ff_wst"]), _p(t["f1_ff_vec"]), _p(imgfeat), B, T, st)
    ctxall = _nan(L, tok)
    h.call("gmf_fusion_ctx_prepare", 1, _p(imgfeat), _p(t["ctx_wst"]), _p(t["ctx_vec"]), _p(ctxall), B, T, L, packing.CTX_WST,
           packing.CTX_VEC, st)
    pts8 = _nan(B * _tiles(N) * 32 * 8)
    h.call("gmf_pack_pts8", _p(d["src_keypts"]), _p(d["tgt_keypts"]), B, N, _p(pts8), st)
    cur = d["corr_pos"]
    for l in range(L):
        f, q, k, v, x1, x2, out = (_nan(act) for _ in range(7))
        h.call("gmf_front_forward", 1 if l == 0 else 0, _p(cur), _p(t["front_wst"][l]), _p(t["front_vec"][l]), _p(f), _p(q), _p(k),
               _p(v), B, N, st)
        h.call("gmf_fusion_attn_forward", 1, _p(f), _p(ctxall[l]), _p(t["attn_wst"][l]), _p(t["attn_vec"][l]), _p(x1), B, N, T, st)
        h.call("gmf_fusion_ff_forward", _p(x1), _p(t["ff_wst"][l]), _p(t["ff_vec"][l]), _p(x2), B, N, st)
        h.call("gmf_scattn_forward", _p(q), _p(k), _p(v), _p(pts8), _p(x2), _p(t["tail_wst"][l]), _p(t["tail_vec"][l]), _p(out), B, N,
               sigma_d, st)
        cur = out
    logits, feat_n, feat = _nan(B, N), _nan(B, N, 128), _nan(B, N, 128)
    h.call("gmf_classifier_forward", _p(cur), _p(t["head_wst"]), _p(t["head_vec"]), _p(logits), _p(feat_n), _p(feat), B, N, st)
    return logits.cpu(), feat_n.cpu(), feat.cpu()


@pytest.mark.parametrize("B,N,T,L", [(1, 33, 1, 2), (2, 257, 196, 12), (3, 1000, 300, 12)])
def test_composed_stages_equal_whole_forward(B, N, T, L):
    """Fusion-1 (pack, ctx_prepare pe 0, attn pe 0 with N = T, ff), one ctx_prepare for the L Fusion-2 contexts, per layer
    front + attn (pe 1) + ff + scattn, then the classifier: bit for bit what gmf_encoder_forward computes under
    "scattn_variant" = 0 (the kFp32 plan runs exactly these kernels), and within 1e-4 of the fp64 oracle."""
    sd = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, L, 128), seed=23)
    blobs, _ = packing.python_packed_encoder(sd, L)
    t = {k: v.to(DEV).contiguous() for k, v in blobs.items()}
    sigma_d = float(sd["sigma_spat"])
    b = _scene(B, N, T, seed0=4100 + N)
    m = gmf_amd.PointDSC(num_layers=L)
    _, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    m = m.to(DEV).eval()
    h, _ = _h()
    prev = ctypes.c_int(0)
    h.call("gmf_get_tuning", b"scattn_variant", ctypes.byref(prev))
    try:
        h.call("gmf_set_tuning", b"scattn_variant", 0)
        whole_lg, whole_fn, _ = m.encode(*[b[k].to(DEV) for k in ("corr_pos", "src_keypts", "tgt_keypts", "p_tokens", "q_tokens")])
        whole_lg, whole_fn = whole_lg.cpu(), whole_fn.cpu()
    finally:
        h.call("gmf_set_tuning", b"scattn_variant", prev.value)
    lg, fn, feat = _composed(t, b, L, sigma_d)
    assert torch.equal(lg, whole_lg) and torch.equal(fn, whole_fn)
    sd64 = R.sd_as(sd, torch.float64)
    compat = O.compat_matrix(b["src_keypts"].double(), b["tgt_keypts"].double(), sigma_d)[0]
    f64 = O.encoder(sd64, b["corr_pos"].double(), compat, b["p_tokens"].double(), b["q_tokens"].double(), L)
    lg64, fn64 = R.classifier(sd64, f64)
    assert (lg.double() - lg64).abs().max().item() < 1e-4
    assert (fn.double() - fn64).abs().max().item() < 1e-4
    assert (feat.double() - f64).abs().max().item() < 1e-3 * max(1.0, f64.abs().max().item())
