"""Every form of the sparse convolution, its gradients, the FCGF head and the masked BatchNorm (csrc/sparse_kernels.hip,
csrc/sparse_train_kernels.hip) against float64, at the edges of their branches.

The cases are the lines of tests/golden/sparse_forms_table.txt over small generated coordinate sets; tests/test_sparse_forms_host.py
proves on the CPU, from the plans of csrc/sparse_conv_plan.hpp and the reference maps, which edges they reach (empty row groups, rows
and offsets without pairs, pair lists of 1 / 63 / 64 / 65, nsplit = K, chunks of several tiles in the weight gradients, every lane
group width of the narrow kernels, W in LDS and in global memory, grid-stride loops, 1 / a few / 64 BatchNorm chunks, ...).

  a. Every case on integers in [-4, 4] (scale in {1, 0.5, -2}): every partial sum is an integer, or a half, below 2^24, so fp32 is
     exact in any summation order and the result must EQUAL the float64 reference (tests/sparse_reference.py's conv and the explicit
     gradient sums), which is itself checked to be exact.  `out` holds a NaN-free sentinel: rows past the output level's count must
     be unchanged.  Rows of every input past its level's count are NaN: they must not be read.  Where a square root or a division
     enters (normalised head, BatchNorm) the comparison is check_close's.
  b. Poison first: the flagged cases run once with every float input NaN, which leaves NaN in the arena's partial rows / slots; the
     exact run afterwards must not see it.
  c. A NaN and a +inf in one input row: exactly the output rows whose pairs read that row are non-finite (BatchNorm: the columns),
     with and without the ReLU; every other row keeps the bits of the clean run.
  d. The flagged case of each kernel (its longest sum) on real-valued data through check_close of test_train_gradients.py.
  e. Same bits: two runs; a row permutation of the input; the per-batch plans of the ragged set.
  f. normalize_rows_eps forward / backward at its layout edges."""
import collections

import numpy as np
import pytest
import torch

from gmf_amd import sparse as SP
from gmf_amd import train as T

import sparse_reference as R
from test_sparse_forms_host import (KERNELS, NONFINITE, POISON, REPEAT, ROUNDING, SET_PLANS, SETS, case_id, coord_set, geometry,
                                    layer_nsplit, read_table, set_levels, set_map)
from test_train_gradients import check_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN, INF = float("nan"), float("inf")
F64, F32 = torch.float64, torch.float32

TABLE = read_table()
IDS = [case_id(i, c) for i, c in enumerate(TABLE)]


def _cases(kernels=None, flag=0):
    return [pytest.param(i, id=IDS[i]) for i, c in enumerate(TABLE)
            if (kernels is None or KERNELS[c["kernel"]] in kernels) and (not flag or c["flags"] & flag)]


_PLANS = {}


def _plan(name, rows=None):
    """The device plan of a named set (cached), its levels and maps held to the reference's once."""
    if rows is not None:
        return SP.SparsePlan(torch.as_tensor(rows).to(DEV).int(), *SET_PLANS[name])
    if name not in _PLANS:
        plan = _plan(name, coord_set(name))
        host = plan.to_host()
        lv = set_levels(name)
        assert host["counts"] == [len(r) for r in lv]
        for m, kmap in enumerate(SET_PLANS[name][1]):
            rp, pairs = set_map(name, kmap)
            assert np.array_equal(host["maps"][m][0].numpy(), rp) and np.array_equal(host["maps"][m][1].numpy(), pairs), (name, kmap)
        _PLANS[name] = plan
    return _PLANS[name]


def _pad(t, M, fill=NAN):
    """float32 [M, C] on the device: the rows of t, then `fill`"""
    if t is None:
        return None
    out = torch.full((M, t.shape[1]), fill, dtype=F32)
    out[:t.shape[0]] = t.float()
    return out.to(DEV)


def _sentinel(M, C):
    return (1.0e6 + (torch.arange(M * C, device=DEV) % 1021)).float().reshape(M, C)


def _dev(t):
    return None if t is None else t.float().to(DEV)


def _relu(v, on):
    return torch.relu(v) if on else v


def _exact(ref, scale=2):
    """the float64 reference is exact (integers, or halves after a scale of 0.5) and fits fp32"""
    return bool(((scale * ref).round() == scale * ref).all()) and float(ref.abs().max()) < 2 ** 23


class Run:
    """One table case with drawn data: .run() -> {name: device tensor of the valid part}, .ref(dtype) -> the same on the CPU."""

    def __init__(self, i, seed, integer=True, relu=None, plan=None, perm=None):
        self.i, self.c = i, dict(TABLE[i])
        c = self.c
        if relu is not None:
            c["relu"] = relu
        self.g = g = geometry(c)
        self.kern = g["kern"]
        self.plan = plan or _plan(g["set"])
        self.M = self.plan.M
        self.kmap = g["kmap"]
        self.m = None if self.kmap is None else SET_PLANS[g["set"]][1].index(self.kmap)
        self.cmap0 = None if self.kmap is None else set_map(g["set"], self.kmap)       # the case's own map (dgrad: not the launch's)
        self.n_out, self.n_in = len(set_levels(g["set"])[c["out"]]), len(set_levels(g["set"])[c["in"]])
        gen = torch.Generator().manual_seed(seed)

        def draw(*shape):
            if integer:
                return torch.randint(-4, 5, shape, generator=gen).double()
            return torch.randn(shape, generator=gen, dtype=F32).double()

        ca, cb, cout, K = c["ca"], c["cb"], c["cout"], g["K"]
        cin = ca + cb
        n_in, n_out = self.n_in, self.n_out
        d = self.d = {}
        if self.kern in ("conv", "dgrad", "wgrad", "narrow", "narrow_wgrad"):
            d["xa"], d["xb"] = draw(n_in, ca), (draw(n_in, cb) if cb else None)
            d["W"] = draw(K, cin, cout) if integer else draw(K, cin, cout) / (cin * min(K, 27)) ** 0.5
            d["dy"] = draw(n_out, cout)
            d["scale"] = (torch.tensor([1.0, 0.5, -2.0], dtype=F64)[torch.randint(0, 3, (cout,), generator=gen)] if integer
                          else 1 + 0.2 * draw(cout)) if c["scale"] else None
            d["shift"] = draw(cout) if c["shift"] else None
            d["res"] = draw(n_out, cout) if c["res"] else None
        elif self.kern == "head":
            d["xa"], d["xb"] = draw(n_in, ca), (draw(n_in, cb) if cb else None)
            d["W1"], d["W2"] = draw(cin, c["hid"]), draw(c["hid"], cout)
            if not integer:
                d["W1"], d["W2"] = d["W1"] / cin ** 0.5, d["W2"] / c["hid"] ** 0.5
            d["bias"] = draw(cout) if c["shift"] else None
        else:
            d["x"] = draw(n_in, ca) if integer else 3 + 2 * draw(n_in, ca)
            d["res"] = draw(n_in, ca) if c["res"] else None
            d["dy"] = draw(n_in, ca)
            d["gamma"], d["beta"] = 1 + 0.125 * draw(ca), 0.125 * draw(ca)
            d["rm"], d["rv"] = draw(ca), 1 + draw(ca).abs()
        self.perm = perm            # level-0 tensors are given to the device in this row order (a plan built from permuted rows)

    def _l0(self, t, level):
        return t if (self.perm is None or level != 0 or t is None) else t[self.perm]

    # -- the device ---------------------------------------------------------------------------------------------------------------
    def run(self, poison=False):
        c, d, M, plan = self.c, self.d, self.M, self.plan
        nanlike = (lambda t: None if t is None else torch.full_like(t, NAN)) if poison else (lambda t: t)
        lin, lout = c["in"], c["out"]
        kern = self.kern
        if kern in ("conv", "narrow"):
            xa, xb = _pad(self._l0(nanlike(d["xa"]), lin), M), _pad(self._l0(nanlike(d["xb"]), lin), M)
            out = _sentinel(M, c["cout"])
            self.out = out
            kw = dict(scale=_dev(nanlike(d["scale"])), shift=_dev(nanlike(d["shift"])), residual=_pad(self._l0(nanlike(d["res"]), lout), M),
                      relu=bool(c["relu"]), out=out)
            if kern == "conv":
                SP.sparse_conv(plan, self.m, lout, xa, _dev(nanlike(d["W"])), xb=xb, nsplit=c["nsplit"], **kw)
            else:
                SP.sparse_conv_narrow(plan, self.m, lout, xa, _dev(nanlike(d["W"])), **kw)
            return {"y": out[:self.n_out]}
        if kern == "dgrad":
            dx = SP.sparse_conv_dgrad(plan, self.m, lout, _pad(self._l0(nanlike(d["dy"]), lout), M), _dev(nanlike(d["W"])))
            self.out = dx
            return {"dx": dx[:self.n_in]}
        if kern in ("wgrad", "narrow_wgrad"):
            xa, xb = _pad(self._l0(nanlike(d["xa"]), lin), M), _pad(self._l0(nanlike(d["xb"]), lin), M)
            dy = _pad(self._l0(nanlike(d["dy"]), lout), M)
            if kern == "wgrad":
                return {"dW": SP.sparse_conv_wgrad(plan, self.m, lout, xa, dy, xb=xb)}
            return {"dW": SP.sparse_conv_narrow_wgrad(plan, self.m, lout, xa, dy)}
        if kern == "head":
            out = _sentinel(M, c["cout"])
            self.out = out
            SP.sparse_head_l2(plan, lout, _pad(self._l0(nanlike(d["xa"]), lin), M), _dev(nanlike(d["W1"])), _dev(nanlike(d["W2"])),
                              xb=_pad(self._l0(nanlike(d["xb"]), lin), M), bias=_dev(nanlike(d["bias"])), normalize=bool(c["scale"]), out=out)
            return {"y": out[:self.n_out]}
        C, n = c["ca"], self.n_in
        bn = torch.nn.BatchNorm1d(C).to(DEV).train()
        with torch.no_grad():
            for p, v in ((bn.weight, "gamma"), (bn.bias, "beta"), (bn.running_mean, "rm"), (bn.running_var, "rv")):
                p.copy_(d[v].float())
        x = _pad(d["x"], M).requires_grad_(True)
        res = None if d["res"] is None else _pad(d["res"], M).requires_grad_(True)
        y = T.batchnorm_masked(x, bn, plan, lout, residual=res, relu=bool(c["relu"]))
        y.backward(_pad(d["dy"], M))
        self.out = y
        got = {"y": y[:n], "dx": x.grad[:n], "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
               "running_var": bn.running_var}
        self.zero_rows = [y[n:], x.grad[n:]]
        if res is not None:
            got["dres"] = res.grad[:n]
            self.zero_rows.append(res.grad[n:])
        return got

    def untouched(self):
        """rows of `out` past the output level's count: the sentinel (conv, narrow, head), zeros (dgrad: its contract, BatchNorm)"""
        if self.kern == "dgrad":
            return bool((self.out[self.n_in:] == 0).all())
        if self.kern == "bnm":
            return all(bool((z == 0).all()) for z in self.zero_rows)
        return bool((self.out[self.n_out:] == _sentinel(*self.out.shape)[self.n_out:]).all())

    # -- the reference ------------------------------------------------------------------------------------------------------------
    def ref(self, dt=F64):
        c, d, g, kern = self.c, self.d, self.g, self.kern
        to = lambda t: None if t is None else t.to(dt)       # noqa: E731
        if kern in ("conv", "narrow"):
            x = torch.cat([d["xa"]] + ([d["xb"]] if d["xb"] is not None else []), 1)
            v = R.conv(x, self.cmap0, d["W"], self.n_out, dt)
            if d["scale"] is not None:
                v = v * to(d["scale"])
            if d["shift"] is not None:
                v = v + to(d["shift"])
            if d["res"] is not None:
                v = v + to(d["res"])
            return {"y": _relu(v, c["relu"])}
        if kern == "dgrad":                              # dx[i] = sum over the pairs (o, d, i) of dy[o] W[d]^T
            W, dy = to(d["W"]), to(d["dy"])
            dx = torch.zeros((self.n_in, W.shape[1]), dtype=dt)
            if self.cmap0 is None:
                return {"dx": dy @ W[0].t()}
            o, dd, ii = self._pairs()
            for k in torch.unique(dd).tolist():
                s = dd == k
                dx.index_add_(0, ii[s], dy[o[s]] @ W[k].t())
            return {"dx": dx}
        if kern in ("wgrad", "narrow_wgrad"):            # dW[d] = sum over the pairs (o, d, i) of x[i]^T dy[o]
            x = to(torch.cat([d["xa"]] + ([d["xb"]] if d["xb"] is not None else []), 1))
            dy = to(d["dy"])
            if self.cmap0 is None:
                return {"dW": (x.t() @ dy).unsqueeze(0)}
            dW = torch.zeros((g["K"], x.shape[1], dy.shape[1]), dtype=dt)
            o, dd, ii = self._pairs()
            for k in torch.unique(dd).tolist():
                s = dd == k
                dW[k] = x[ii[s]].t() @ dy[o[s]]
            return {"dW": dW}
        if kern == "head":
            x = to(torch.cat([d["xa"]] + ([d["xb"]] if d["xb"] is not None else []), 1))
            y = torch.relu(x @ to(d["W1"])) @ to(d["W2"])
            if d["bias"] is not None:
                y = y + to(d["bias"])
            if c["scale"]:
                y = y / (y.norm(dim=1, keepdim=True) + 1e-8)
            return {"y": y}
        C = c["ca"]
        b = torch.nn.BatchNorm1d(C).to(dt).train()
        b.load_state_dict({"weight": to(d["gamma"]), "bias": to(d["beta"]), "running_mean": to(d["rm"]), "running_var": to(d["rv"]),
                           "num_batches_tracked": torch.tensor(0)})
        x = d["x"].clone().to(dt).requires_grad_(True)
        res = None if d["res"] is None else d["res"].clone().to(dt).requires_grad_(True)
        y = b(x)
        if res is not None:
            y = y + res
        y = _relu(y, c["relu"])
        y.backward(to(d["dy"]))
        out = {"y": y.detach(), "dx": x.grad, "dgamma": b.weight.grad, "dbeta": b.bias.grad, "running_mean": b.running_mean,
               "running_var": b.running_var}
        if res is not None:
            out["dres"] = res.grad
        return out

    def _pairs(self):
        row_ptr, pairs = self.cmap0
        o = torch.as_tensor(np.repeat(np.arange(self.n_out), np.diff(row_ptr)))
        return o, torch.as_tensor(pairs[:, 0]), torch.as_tensor(pairs[:, 1])

    def readers(self, r):
        """the output rows whose pairs read input row r"""
        if self.cmap0 is None:
            return torch.tensor([r])
        o, _, ii = self._pairs()
        return torch.unique(o[ii == r])

    @property
    def approximate(self):
        """a square root or a division enters: no equality on integers"""
        return self.kern == "bnm" or (self.kern == "head" and bool(self.c["scale"]))


def test_layer_nsplit_restated():
    for K, cin, cout in [(1, 5, 5), (27, 32, 32), (729, 80, 72), (729, 128, 128), (729, 3, 5), (343, 1, 32), (3, 2, 2)]:
        assert layer_nsplit(K, cin, cout) == SP.layer_nsplit(K, cin, cout)


_worst = collections.defaultdict(float)


def _close(run, got, what):
    rep = check_close({k: v.cpu() for k, v in got.items()}, run.ref(F64), run.ref(F32), what=what)
    worst = max((e / t if t > 0 else (0.0 if e == 0 else INF)) for e, t in rep.values())
    _worst[run.kern] = max(_worst[run.kern], worst)
    print(f"{what}worst err/tol {worst:.4f}; worst so far per kernel {dict(_worst)}")


def _assert_equal(run, got, what):
    ref = run.ref(F64)
    for name, r in ref.items():
        assert _exact(r), f"{what}{name}: the float64 reference is not exact on these integers"
        g = got[name].cpu().double().reshape(r.shape)
        bad = (g != r).nonzero()
        assert bad.numel() == 0, (f"{what}{name}: {bad.shape[0]} of {r.numel()} entries differ, first at {bad[0].tolist()}: "
                                  f"got {float(g[tuple(bad[0])])}, want {float(r[tuple(bad[0])])}")


# ---- a. every case on integers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", _cases())
def test_sparse_form_exact_on_integers(i):
    run = Run(i, 1000 + i)
    g = run.g
    assert 16 * g["K"] * max(g["cin"], 1) + 8 < 2 ** 23          # every partial sum of integers in [-4, 4] fits fp32 exactly
    got = run.run()
    what = f"case {IDS[i]}: "
    if run.approximate:
        _close(run, got, what)
    else:
        _assert_equal(run, got, what)
    assert run.kern in ("wgrad", "narrow_wgrad") or run.untouched(), f"{what}rows past the level count were written"
    if run.kern in ("wgrad", "narrow_wgrad") and run.cmap0 is not None:     # offsets without pairs: exact zeros
        empty = np.nonzero(np.bincount(run.cmap0[1][:, 0], minlength=g["K"]) == 0)[0]
        assert bool((got["dW"][torch.as_tensor(empty, device=DEV)] == 0).all())


# ---- b. poison first ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", _cases(flag=POISON))
def test_sparse_form_exact_after_a_call_that_left_nan_in_the_workspace(i):
    """The partial rows of k_sparse_conv are written on a row's first offset of a slice and read back by k_split_reduce only for
    the slices the row has pairs in; the weight gradient's slots only up to the chunk count.  A wrong first-touch flag, slice test
    or chunk count reads what the call before left there."""
    run = Run(i, 1500 + i)
    assert run.kern in ("conv", "wgrad", "narrow_wgrad") and (run.kern != "conv" or run.c["nsplit"] > 1)
    left = run.run(poison=True)
    assert bool(torch.isnan(next(iter(left.values()))).any()), "the poison run itself gives NaN"
    if run.kern != "conv":                                # other maps of the same K leave other chunk tables behind
        for m, kmap in enumerate(SET_PLANS[run.g["set"]][1]):
            if kmap[0] == run.kmap[0] and kmap != run.kmap:
                other = torch.full((run.M, run.c["ca"] + run.c["cb"]), NAN, device=DEV), torch.full((run.M, run.c["cout"]), NAN, device=DEV)
                (SP.sparse_conv_wgrad if run.kern == "wgrad" else SP.sparse_conv_narrow_wgrad)(run.plan, m, kmap[1], *other)
        run.run(poison=True)
    got = run.run()
    _assert_equal(run, got, f"case {IDS[i]} after poison: ")
    assert run.kern != "conv" or run.untouched()


# ---- c. a NaN and an inf reach exactly the rows that read them ----------------------------------------------------------------------
def _nonfinite(i, relu):
    run = Run(i, 2000 + i, relu=relu)
    what = f"case {IDS[i]} relu {relu}: "
    clean = {k: v.clone() for k, v in run.run().items()}
    if run.kern == "bnm":
        n, C = run.n_in, run.c["ca"]
        r, c0, c1 = n // 2, 1, C - 2
        run.d["x"][r, c0], run.d["x"][r, c1] = NAN, INF
        got = run.run()
        hit = torch.zeros(C, dtype=torch.bool, device=DEV)
        hit[[c0, c1]] = True
        for name in ("y", "dx"):
            assert not bool(torch.isfinite(got[name][:, hit]).any()), f"{what}{name}: finite entries in the columns of the NaN / inf"
            assert torch.equal(_bits(got[name][:, ~hit]), _bits(clean[name][:, ~hit])), f"{what}{name}: another column changed"
        assert run.untouched()
        return
    xa, xb = run.d["xa"], run.d["xb"]
    r = run.n_in // 2
    xa[r, 0] = NAN
    if xb is not None:
        xb[r, -1] = INF
    elif xa.shape[1] > 1:
        xa[r, -1] = INF                                    # a single input channel holds the NaN alone
    got = run.run()["y"]
    readers = run.readers(r)
    assert len(readers) > 0
    hit = torch.zeros(run.n_out, dtype=torch.bool, device=DEV)
    hit[readers.to(DEV)] = True
    finite = torch.isfinite(got[hit]).any(1).cpu()
    assert not bool(finite.any()), (f"{what}{int(finite.sum())} of the {len(readers)} rows that read the NaN row hold finite entries; the "
                                    f"first is row {int(readers[int(finite.nonzero()[0])])}: {got[hit][finite.to(DEV)][0][:8].tolist()}")
    assert torch.equal(_bits(got[~hit]), _bits(clean["y"][~hit])), f"{what}a row that does not read it changed"
    assert run.untouched()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("i", _cases(("conv", "narrow", "bnm"), NONFINITE))
def test_sparse_nonfinite_entries_reach_exactly_their_readers(i, relu):
    """A ReLU written as fmaxf(v, 0) returns 0 for a NaN and hands on a clean row; torch's relu keeps the NaN."""
    _nonfinite(i, relu)


@pytest.mark.parametrize("i", _cases(("head",), NONFINITE))
def test_sparse_head_nonfinite_row_stays_nonfinite(i):
    """The head's hidden ReLU has no switch: with fmaxf a NaN input row came out as the bias."""
    _nonfinite(i, None)


# ---- d. real-valued data against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", _cases(flag=ROUNDING))
def test_sparse_form_against_float64(i):
    run = Run(i, 3000 + i, integer=False)
    got = run.run()
    _close(run, got, f"case {IDS[i]}: ")
    assert run.kern in ("wgrad", "narrow_wgrad") or run.untouched()


# ---- e. same bits ------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("i", _cases(flag=REPEAT))
def test_sparse_form_bits_do_not_depend_on_the_run_or_the_row_order(i):
    """Two runs give the same bits.  conv, dgrad, narrow: a plan built from the rows in another order gives the same bits row for
    row (level 0 follows the input order; coarser levels are sorted and do not move).  Not asserted for the weight gradients: an
    offset's pairs are added in ascending output row, so the order of the sum follows the input order by design."""
    run = Run(i, 4000 + i, integer=False)
    first = {k: v.clone() for k, v in run.run().items()}
    second = run.run()
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(second[k])), f"case {IDS[i]}: two runs differ in {k}"
    if run.kern in ("wgrad", "narrow_wgrad"):
        return
    name = run.g["set"]
    perm = np.random.default_rng(i).permutation(len(coord_set(name)))
    other = Run(i, 4000 + i, integer=False, plan=_plan(name, coord_set(name)[perm]), perm=torch.as_tensor(perm))
    got = other.run()
    out_level = run.c["in"] if run.kern == "dgrad" else run.c["out"]
    for k in first:
        want = first[k][torch.as_tensor(perm, device=DEV)] if out_level == 0 else first[k]
        assert torch.equal(_bits(got[k]), _bits(want)), f"case {IDS[i]}: {k} depends on the input row order"


@pytest.mark.parametrize("i", [p for p in _cases(("conv",), REPEAT) if SETS[TABLE[p.values[0]]["set"]] == "ragged-d3"])
def test_sparse_conv_sliced_equals_per_batch_plans(i):
    """The same sliced convolution on the plan of one batch alone (other row groups, other partial rows) gives the bits of that
    batch's rows."""
    run = Run(i, 4500 + i, integer=False)
    c = run.c
    assert c["nsplit"] > 1 and c["out"] == 0 and c["in"] == 0
    whole = run.run()["y"].clone()
    rows = coord_set(run.g["set"])
    d = run.d
    for b in np.unique(rows[:, 0]):
        sel = torch.as_tensor(np.nonzero(rows[:, 0] == b)[0])
        pb = _plan(run.g["set"], rows[sel.numpy()])
        y = SP.sparse_conv(pb, run.m, 0, _dev(d["xa"][sel]), _dev(d["W"]), xb=None if d["xb"] is None else _dev(d["xb"][sel]),
                           scale=_dev(d["scale"]), shift=_dev(d["shift"]), residual=None if d["res"] is None else _dev(d["res"][sel]),
                           relu=bool(c["relu"]), nsplit=c["nsplit"])
        assert torch.equal(_bits(y), _bits(whole[sel.to(DEV)])), f"case {IDS[i]}: batch {int(b)} alone differs"


# ---- f. FCGF's row normalisation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("rows,C", [(1, 65), (6, 130), (5, 64)])
def test_normalize_rows_eps_against_float64(rows, C, zero):
    """x / (||x|| + 1e-8) and its backward across the 64-lane stride (C = 64, 65, 130).  An all-zero row gives a zero row and, by
    the kernel's contract, a zero gradient (the quotient's own derivative there is 1 / 1e-8)."""
    g = torch.Generator().manual_seed(rows * 1000 + C)
    x = torch.randn(rows, C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    if zero:
        x[rows - 1] = 0
    keep = torch.arange(rows) < (rows - 1 if zero else rows)
    xd = x.to(DEV).requires_grad_(True)
    y = T.normalize_rows_eps(xd)
    y.backward(dy.to(DEV))
    if zero:
        assert bool((y[rows - 1] == 0).all()) and bool((xd.grad[rows - 1] == 0).all())
    if not bool(keep.any()):
        return
    ref = {}
    for dt in (F64, F32):
        xr = x[keep].to(dt).requires_grad_(True)
        yr = xr / (xr.norm(dim=1, keepdim=True) + 1e-8)
        yr.backward(dy[keep].to(dt))
        ref[dt] = {"y": yr.detach(), "dx": xr.grad}
    check_close({"y": y[keep.to(DEV)].cpu(), "dx": xd.grad[keep.to(DEV)].cpu()}, ref[F64], ref[F32], what=f"normalize_rows_eps {rows}x{C}: ")
