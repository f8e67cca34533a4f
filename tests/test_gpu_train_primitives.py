"""The row primitives of csrc/train_kernels.hip at the edges of their layouts: one wave per row and four rows per workgroup
(LayerNorm, softmax, normalize_rows), one thread per element in 256-thread workgroups (LCPE, GEGLU, ReLU backward), 64-column
blocks x row chunks (gmf_colsum).

Every primitive is held twice: against the same formula in float64 through check_close (test_train_gradients.py: the fp32 formula
gives the noise floor), and - wherever the arithmetic allows - exactly on integer data.  Tensors whose magnitudes differ by orders
(the rstd of a constant row, the gradient of a zero row) go through check_close on their own, so that their size does not widen
another tensor's tolerance."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from gmf_amd import train as T_
from test_train_gradients import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = [1, 3, 4, 5]             # four rows per workgroup: a partly filled, a full, a full and a partly filled one


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(gen, *shape):
    return torch.randn(*shape, generator=gen).to(DEV)


def _ri(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float().to(DEV)


def _each(got, fn, args, alone=(), what=""):
    """check_close of `got` against fn(*args) in float64 and float32 (dicts with the same keys): the outputs of the function as one
    group, the tensors named in `alone` each on its own (their size does not enter another tensor's tolerance, nor the reverse)."""
    ref = fn(*[a.double() if torch.is_tensor(a) and a.is_floating_point() else a for a in args])
    ref32 = fn(*args)
    groups = [[k for k in ref if k not in alone]] + [[k] for k in alone]
    rep = {}
    for names in groups:
        if names:
            rep.update(check_close({k: got[k] for k in names}, {k: ref[k] for k in names}, {k: ref32[k] for k in names}, what=what))
    return rep


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def _ln_ref(x, gamma, beta, dy, dx_add):
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = (var + 1e-5) ** -0.5
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return {"y": xh * gamma + beta, "mean": mean, "rstd": rstd, "dx": dx, "dx_add": dx + dx_add}


def _ln_hip(x, gamma, beta, dy, dx_add):
    y, mean, rstd = T_.layernorm_fwd(x, gamma, beta)
    return {"y": y, "mean": mean, "rstd": rstd, "dx": T_.layernorm_bwd(dy, x, gamma, mean, rstd),
            "dx_add": T_.layernorm_bwd(dy, x, gamma, mean, rstd, dx_add=dx_add)}


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 128, 1024, 1025])
@pytest.mark.parametrize("rows", ROWS)
def test_layernorm_forward_backward(rows, C):
    """Forward with the saved mean and rstd, backward with and without dx_add.  C = 1: every row is constant (y = beta, dx = 0).
    C = 1025 is past the `C <= 1024` an earlier comment claimed: the kernels loop over the row, any C is right."""
    gen = _gen(100 * C + rows)
    args = [_rn(gen, rows, C) * 2 + 0.5, _rn(gen, C), _rn(gen, C), _rn(gen, rows, C), _rn(gen, rows, C)]
    _each(_ln_hip(*args), _ln_ref, args, alone=("rstd",), what=f"layernorm rows={rows} C={C}: ")     # C = 1: rstd = 316


@pytest.mark.parametrize("C", [2, 63, 64, 65, 1025])
def test_layernorm_constant_row(C):
    """A row of one value (0.5 C is exact in fp32, so the mean is too): variance 0, rstd = rsqrt(1e-5), y = beta, and
    dx = rstd (g - mean(g)) - 316 times the size of the other tensors, so it is held on its own."""
    gen = _gen(C)
    x = torch.full((3, C), 0.5, device=DEV)
    args = [x, _rn(gen, C), _rn(gen, C), _rn(gen, 3, C), _rn(gen, 3, C)]
    got = _ln_hip(*args)
    _each(got, _ln_ref, args, alone=("rstd", "dx", "dx_add"), what=f"layernorm constant rows C={C}: ")
    assert torch.equal(got["mean"], torch.full((3,), 0.5, device=DEV))
    assert float((got["rstd"] - 1e-5 ** -0.5).abs().max()) <= 2e-5 * 1e-5 ** -0.5
    assert torch.equal(got["y"], args[2].expand(3, C))


def test_layernorm_exact_on_integers():
    """Rows of +-1 with zero sum at C = 64: mean 0, variance 1 exactly; with gamma = 2^k and integer beta y is exact up to rstd's
    own rounding: 1 + 1e-5 rounds to fp32 (half an ulp, halved by the root) and rsqrtf is good to an ulp or two - 2^-21 relative."""
    gen = _gen(7)
    x = torch.ones(5, 64)
    x[:, torch.randperm(64, generator=gen)[:32]] = -1
    y, mean, rstd = T_.layernorm_fwd(x.to(DEV), torch.ones(64, device=DEV), torch.zeros(64, device=DEV))
    assert torch.equal(mean, torch.zeros(5, device=DEV))
    want = torch.tensor(1.00001, dtype=torch.float64).rsqrt().float().item()
    assert float((rstd - want).abs().max()) <= want * 2.0 ** -21
    assert torch.equal(y, x.to(DEV) * rstd[:, None])


# ---- softmax -----------------------------------------------------------------------------------------------------------------------
def _softmax_ref(S, mul, dP, scale):
    z = S * scale if mul is None else mul * (S * scale)
    P = torch.softmax(z, -1)
    dS = scale * (1.0 if mul is None else mul) * P * (dP - (P * dP).sum(-1, keepdim=True))
    return {"P": P, "dS": dS}


def _softmax_hip(S, mul, dP, scale):
    P = T_.softmax_rows(S, scale, mul=mul)
    return {"P": P, "dS": T_.softmax_rows_bwd(P, dP, scale, mul=mul)}


@pytest.mark.parametrize("T", [1, 63, 64, 65, 196, 4096, 4097])
@pytest.mark.parametrize("rows", ROWS)
def test_softmax_forward_backward(rows, T):
    """With and without `mul`, scale 1 and 0.3.  Row 0 spans the logits +-80, the last row has one dominant logit.  T = 4097 is past
    the `T <= 4096` an earlier comment claimed: the kernels loop over the row, any T is right."""
    gen = _gen(100 * T + rows)
    S = _rn(gen, rows, T) * 3
    S[0] = torch.linspace(-80, 80, T) if T > 1 else 80.0
    S[-1, T // 2] += 40.0
    dP = _rn(gen, rows, T)
    for scale, mul in itertools.product((1.0, 0.3), (None, torch.rand(rows, T, generator=gen).to(DEV) + 0.5)):
        args = [S, mul, dP, scale]
        got = _softmax_hip(*args)
        _each(got, _softmax_ref, args)
        assert float((got["P"].double().sum(-1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("T", [2, 65, 4097])
def test_softmax_logits_that_overflow_without_the_max(T):
    """Logits of +-100 (and +-150 through mul = 1.5): exp of the largest alone is past fp32.  The row is the float64 softmax."""
    S = torch.zeros(3, T, device=DEV)
    S[:, 0], S[:, -1] = -100.0, 100.0
    S[1, T // 2] = 100.0
    for mul in (None, torch.full((3, T), 1.5, device=DEV)):
        got = T_.softmax_rows(S, 1.0, mul=mul)
        assert bool(torch.isfinite(got).all())
        _each({"P": got}, lambda s, m: {"P": torch.softmax(s if m is None else m * s, -1)}, [S, mul])


# ---- GEGLU -------------------------------------------------------------------------------------------------------------------------
def _geglu_ref(hdn, dg):
    H = hdn.shape[1] // 2
    x, gt = hdn[:, :H], hdn[:, H:]
    Phi = 0.5 * (1 + torch.erf(gt / math.sqrt(2.0)))
    phi = torch.exp(-0.5 * gt * gt) / math.sqrt(2 * math.pi)
    return {"g": x * gt * Phi, "dx": dg * gt * Phi, "dgates": dg * x * (Phi + gt * phi)}


@pytest.mark.parametrize("H", [1, 63, 64, 65, 128])
@pytest.mark.parametrize("rows", [1, 7])
def test_geglu_forward_backward(rows, H):
    """Gates over [-6, 6] with 0 and both tails in every shape; rows x H crosses a 256-thread workgroup at 7 x 63."""
    gen = _gen(10 * H + rows)
    hdn = _rn(gen, rows, 2 * H)
    gates = torch.linspace(-6, 6, rows * H).reshape(rows, H)
    gates.view(-1)[(rows * H) // 2] = 0.0
    hdn[:, H:] = gates.to(DEV)
    hdn[0, H] = -6.0 if rows * H > 1 else 0.0
    dg = _rn(gen, rows, H)
    dh = T_.geglu_bwd(hdn, dg)
    _each({"g": T_.geglu_fwd(hdn), "dx": dh[:, :H], "dgates": dh[:, H:]}, _geglu_ref, [hdn, dg])


def test_geglu_zero_gate_is_exact():
    hdn = torch.tensor([[3.0, -2.0, 0.0, -0.0]], device=DEV)
    dg = torch.tensor([[5.0, 7.0]], device=DEV)
    assert torch.equal(T_.geglu_fwd(hdn), torch.zeros(1, 2, device=DEV))
    assert torch.equal(T_.geglu_bwd(hdn, dg), torch.tensor([[0.0, 0.0, 7.5, -7.0]], device=DEV))     # dgates = dg x Phi(0) = dg x / 2


# ---- LCPE --------------------------------------------------------------------------------------------------------------------------
def _shifted(v, L, shift):
    """v [S * L, C] -> row r holds v[r + shift] when that row lies in r's sequence of L rows, else 0"""
    s = v.reshape(-1, L, v.shape[-1])
    out = torch.zeros_like(s)
    if shift == 0:
        out = s.clone()
    elif shift > 0 and L > shift:
        out[:, :-shift] = s[:, shift:]
    elif shift < 0 and L > -shift:
        out[:, -shift:] = s[:, :shift]
    return out.reshape(v.shape)


def _lcpe_ref(x, w, b, dy, L):
    w = w.reshape(-1, 3)
    return {"y": x + b + w[:, 0] * _shifted(x, L, -1) + w[:, 1] * x + w[:, 2] * _shifted(x, L, 1),
            "dx": dy * (1 + w[:, 1]) + w[:, 0] * _shifted(dy, L, 1) + w[:, 2] * _shifted(dy, L, -1)}


@pytest.mark.parametrize("C", [1, 64, 65])
@pytest.mark.parametrize("L", [1, 2, 3, 37])
def test_lcpe_forward_backward(L, C):
    """Five sequences of L rows: no tap crosses a sequence boundary (the neighbouring sequence holds other values, so a crossing
    tap changes the result).  Against float64, and exactly with integer x, taps and bias."""
    gen = _gen(100 * L + C)
    for integer in (False, True):
        draw = (lambda *s: _ri(gen, -8, 8, *s)) if integer else (lambda *s: _rn(gen, *s))
        x, w, b, dy = draw(5 * L, C), draw(C, 1, 3), draw(C), draw(5 * L, C)
        got = {"y": T_.lcpe_fwd(x, w, b, L), "dx": T_.lcpe_bwd(dy, w, L)}
        if integer:
            ref = _lcpe_ref(x.double(), w.double(), b.double(), dy.double(), L)
            assert torch.equal(got["y"].double(), ref["y"]) and torch.equal(got["dx"].double(), ref["dx"])
        else:
            _each(got, lambda *a: _lcpe_ref(*a, L), [x, w, b, dy])


# ---- gmf_colsum --------------------------------------------------------------------------------------------------------------------
def _colsum_ref(x, y, mean, rstd, cmean, crstd, relu_y, center_x, shift, L, dual):
    xp = x if relu_y is None else torch.where(relu_y > 0, x, torch.zeros_like(x))
    if center_x:
        xp = xp - cmean
    plain = xp.sum(0)
    if y is None:
        return {"out": plain}
    yp = y
    if mean is not None:
        yp = (yp - mean[:, None]) * rstd[:, None]
    if cmean is not None:
        yp = (yp - cmean) * (1.0 if crstd is None else crstd)
    hit = _shifted(torch.ones_like(x), L, shift)                  # rows whose partner lies outside the sequence contribute 0
    out = (xp * _shifted(yp, L, shift) * hit).sum(0)
    return {"out": out, "plain": plain} if dual else {"out": out}


def _colsum_hip(x, y, mean, rstd, cmean, crstd, relu_y, center_x, shift, L, dual):
    rows, C = x.shape
    out = torch.full((2 * C if dual else C,), float("nan"), device=DEV)
    T_._call("gmf_colsum", x, x, y, mean, rstd, cmean, crstd, int(center_x), int(shift), int(L), rows, C, relu_y, int(dual), out)
    return {"out": out[:C], "plain": out[C:]} if dual else {"out": out}


# option sets (which tensors are given): every option alone, the pairs of the issue, and dual with each
_OPTS = {
    "plain": dict(),
    "y": dict(y=1),
    "mean_rstd": dict(y=1, mean=1),
    "cmean_crstd": dict(y=1, cmean=1, crstd=1),
    "cmean_only": dict(y=1, cmean=1),
    "cmean_crstd_center": dict(y=1, cmean=1, crstd=1, center_x=1),
    "center_no_y": dict(cmean=1, center_x=1),
    "relu_y": dict(relu_y=1),
    "relu_y_y": dict(y=1, relu_y=1),
    "everything": dict(y=1, mean=1, cmean=1, crstd=1, center_x=1, relu_y=1),
}


def _colsum_args(gen, rows, C, opt, shift, L, dual, integer):
    if integer:       # all values multiples of 1/4 and every partial sum below 2^24 quarters: exact in any order
        x, y, ry = _ri(gen, -4, 4, rows, C), _ri(gen, -4, 4, rows, C), _ri(gen, -2, 2, rows, C)
        mean, rstd = _ri(gen, -1, 1, rows), 0.5 * _ri(gen, 1, 2, rows)
        cmean, crstd = _ri(gen, -1, 1, C), 0.5 * _ri(gen, 1, 2, C)
    else:
        x, y, ry = _rn(gen, rows, C), _rn(gen, rows, C) + 0.3, _rn(gen, rows, C)
        mean, rstd = _rn(gen, rows) * 0.2, torch.rand(rows, generator=gen).to(DEV) + 0.5
        cmean, crstd = _rn(gen, C) * 0.2, torch.rand(C, generator=gen).to(DEV) + 0.5
    pick = lambda k, v: v if opt.get(k) else None
    return [x, pick("y", y), pick("mean", mean), pick("mean", rstd), pick("cmean", cmean), pick("crstd", crstd), pick("relu_y", ry),
            bool(opt.get("center_x")), shift, L, bool(dual and opt.get("y"))]


def _colsum_check(rows, C, name, shift, L, dual, seed):
    what = f"colsum rows={rows} C={C} {name} shift={shift} L={L} dual={dual}: "
    gen = _gen(seed)
    args = _colsum_args(gen, rows, C, _OPTS[name], shift, L, dual, integer=True)
    got, ref = _colsum_hip(*args), _colsum_ref(*[a.double() if torch.is_tensor(a) else a for a in args])
    for k in ref:
        bad = (got[k].double() != ref[k]).nonzero()
        assert bad.numel() == 0, f"{what}{k} on integers: column {int(bad[0])}: got {float(got[k][bad[0]])}, want {float(ref[k][bad[0]])}"
    args = _colsum_args(gen, rows, C, _OPTS[name], shift, L, dual, integer=False)
    got = _colsum_hip(*args)
    _each(got, _colsum_ref, args)
    again = _colsum_hip(*args)                # the result does not depend on scheduling
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), what + k + ": two runs differ"


@pytest.mark.parametrize("C", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_colsum_every_option(rows, C):
    """Every option set of _OPTS, plain and dual, at every (rows, C) up to 1000 rows: a part of a chunk, one chunk, one row into the
    second, 16 chunks with a short last one; a part of a column block, one, one column into the second, five."""
    for n, (name, dual) in enumerate(itertools.product(_OPTS, (False, True))):
        if dual and not _OPTS[name].get("y"):
            continue
        _colsum_check(rows, C, name, 0, rows, dual, seed=1000 * rows + 10 * C + n)


@pytest.mark.parametrize("L", [1, 2, 37])
@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_colsum_shifted_partner_stays_in_its_sequence(shift, L):
    """shift x L, plain and dual, with y alone and with mean / rstd (read at the partner's row).  dual returns the plain sums over
    ALL rows, those whose partner lies outside the sequence included."""
    for rows, C in ((L, 1), (3 * L, 65), (L * (1000 // L), 64), (L * 27, 257)):
        for name, dual in itertools.product(("y", "mean_rstd", "relu_y_y", "everything"), (False, True)):
            _colsum_check(rows, C, name, shift, L, dual, seed=rows + C + 7 * L + shift)


@pytest.mark.parametrize("rows,L", [(65537, 65537), (65601, 37), (65538, 2)])
def test_colsum_capped_chunk_count(rows, L):
    """Past 65536 rows the chunk count stays at 1024 and a chunk is longer than 64 rows (65 here, the last chunk shorter): more than
    one round of a wave's four-rows-in-flight loop, which ends inside a group of four."""
    for n, (C, name, shift, dual) in enumerate(((65, "plain", 0, False), (64, "mean_rstd", 1 if L < rows else 0, True),
                                                (63, "everything", -1 if L < rows else 0, True), (1, "y", 0, False))):
        _colsum_check(rows, C, name, shift, L, dual, seed=rows + n)


def test_colsum_wrapper_matches_the_direct_call():
    gen = _gen(3)
    x, y = _rn(gen, 74, 65), _rn(gen, 74, 65)
    a, b = T_.colsum(x, y=y, shift=1, L=37, dual=True)
    ref = _colsum_hip(x, y, None, None, None, None, None, False, 1, 37, True)
    assert torch.equal(a, ref["out"]) and torch.equal(b, ref["plain"])


# ---- normalize_rows ----------------------------------------------------------------------------------------------------------------
def _normalize_ref(x, dy):
    n = x.norm(dim=-1).clamp_min(1e-12)
    y = x / n[:, None]
    return {"y": y, "nrm": n, "dx": (dy - y * (dy * y).sum(-1, keepdim=True)) / n[:, None]}


def _normalize_hip(x, dy):
    rows, C = x.shape
    nrm, y, dx = torch.empty(rows, device=DEV), torch.empty_like(x), torch.empty_like(x)
    T_._call("gmf_normalize_rows", x, 0, x, None, nrm, y, rows, C)
    T_._call("gmf_normalize_rows", y, 1, y, dy, nrm, dx, rows, C)
    return {"y": y, "nrm": nrm, "dx": dx}


@pytest.mark.parametrize("C", [1, 64, 65, 128])
@pytest.mark.parametrize("rows", ROWS)
def test_normalize_rows_forward_backward(rows, C):
    """y and dx as one group, the saved norm (up to 3 sqrt(C)) on its own.  At C = 1 the true dx is 0 and what the kernel returns
    is the rounding of y = x / |x| times dy / |x|: the entries stay away from 0 there, so that this is held by y's size."""
    gen = _gen(10 * C + rows)
    x = _rn(gen, rows, C) * 3
    if C == 1:
        x = torch.sign(x) * (1 + x.abs())
    args = [x, _rn(gen, rows, C)]
    _each(_normalize_hip(*args), _normalize_ref, args, alone=("nrm",), what=f"normalize rows={rows} C={C}: ")


@pytest.mark.parametrize("C", [1, 64, 65, 128])
def test_normalize_rows_zero_and_tiny_rows(C):
    """A zero row: the norm is clamped at 1e-12, the output is 0, the gradient dy / 1e-12 is finite.  A row of norm 1e-20 (its
    square is below fp32): clamped as well, y = x / 1e-12."""
    gen = _gen(C)
    dy = _rn(gen, 2, C)
    x = torch.zeros(2, C, device=DEV)
    x[1, C - 1] = 1e-20
    got = _normalize_hip(x, dy)
    assert torch.equal(got["nrm"], torch.full((2,), 1e-12, device=DEV))
    assert torch.equal(got["y"][0], torch.zeros(C, device=DEV)) and bool(torch.isfinite(got["dx"]).all())
    _each(got, _normalize_ref, [x, dy], alone=("y", "nrm", "dx"), what=f"normalize zero / tiny rows C={C}: ")


# ---- relu_backward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [1, 255, 256, 257])
def test_relu_backward_exact(total):
    """out = y > 0 ? dy : 0, exactly: -0.0, 0.0 and NaN are not above zero, a subnormal is."""
    gen = _gen(total)
    dy = torch.randn(total, generator=gen)
    y = torch.randn(total, generator=gen)
    special = torch.tensor([-0.0, 0.0, 1e-40, float("nan"), -1e-40])
    pos = [0, total - 1, total // 2, total // 3, total // 5]
    for p, v in zip(pos[:min(total, 5)], special):
        y[p] = v
    want = torch.where(y > 0, dy, torch.zeros(()))
    got = T_.relu_backward(dy.to(DEV), y.to(DEV)).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    if total >= 5:
        assert float(got[total // 2]) == float(dy[total // 2]) and float(got[total // 3]) == 0.0


# ---- the fused ReLU keeps a NaN ----------------------------------------------------------------------------------------------------
def test_batchnorm_relu_keeps_a_nan():
    """One NaN in x makes its column's statistics NaN: with the fused ReLU the column of y is still NaN (fmaxf(NaN, 0) would
    return 0 and hide it; torch's relu, which the reference runs, keeps it).  The other columns are unaffected."""
    gen = _gen(5)
    rows, C = 9, 65
    x = _rn(gen, rows, C)
    gamma, beta = _rn(gen, C), _rn(gen, C)
    ref = torch.relu(F.batch_norm(x.double(), None, None, gamma.double(), beta.double(), training=True, eps=1e-5))
    ref32 = torch.relu(F.batch_norm(x, None, None, gamma, beta, training=True, eps=1e-5))
    x[4, 64] = float("nan")
    y, mean, rstd = torch.empty_like(x), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    T_._call("gmf_batchnorm_train_forward", x, x, gamma, beta, y, mean, rstd, None, None, rows, C, 1e-5, 0.1, 1)
    assert bool(torch.isnan(y[:, 64]).all())
    check_close({"y": y[:, :64]}, {"y": ref[:, :64]}, {"y": ref32[:, :64]}, what="batchnorm + relu beside a NaN column: ")
