"""gmf_gemm_f32 in every launch form (csrc/gemm_plan.hpp): exactly on integer data, and against float64 on real-valued data.

The cases are the lines of tests/golden/gemm_forms_table.txt; tests/test_gemm_plan_host.py proves on the CPU that they reach all 12
k_gemm_lds and all 8 k_gemm_f32 instantiations with and without split-K, every reduce group count, every pipeline tail and both
loaders of the direct kernel.

  1. Every case on small integers: entries of A and B in [-8, 8], alpha in {1, 0.5, -2}, integer bias and residual.  Every partial
     sum is an integer of magnitude at most 64 K <= 2^19, so the fp32 MFMA result is exact in any summation order and the output
     must EQUAL the reference.  The reference is the float64 product on the device - on these integers it is exact too, which the
     test asserts by comparing it with its own rounding to int64.  Every float of A, B and the residual outside the addressed
     sub-matrix (row padding beyond lda's used part, gaps between batches, the floats before the offset and behind the end) is
     NaN; C holds a NaN-free sentinel pattern outside the written sub-matrix, which must be unchanged afterwards.
  2. One case per kernel family without and one with split-K, each without and with the ReLU, with one NaN and one +inf inside a
     row of op(A): exactly that row of C is non-finite.
  3. The flagged case of every instantiation (its longest K) on real-valued data through check_close: float64 reference, the fp32
     CPU product as the noise floor, the tolerances of test_train_gradients.py.
  4. One batched case per reduce group count: two runs give the same bits, and batch element 1 gives the bits of the same product
     computed by a call of its own."""
import collections

import pytest
import torch

from gmf_amd import train as T_
from test_gemm_plan_host import read_table
from test_train_gradients import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
TAIL = 8                       # poisoned floats behind the last addressed one of every buffer

TABLE = read_table()


def _id(i):
    c = TABLE[i]
    return f"{i}-{'NT'[c['ta']]}{'NT'[c['tb']]}-{c['M']}x{c['N']}x{c['K']}-b{c['batch']}"


class Operands:
    """The device buffers of one case around given op(A) [nbA, M, K], op(B) [nbB, K, N] (nb = 1 for a shared operand), bias [N] or
    None, residual [batch, M, N] or None - all CPU tensors of any float type."""

    def __init__(self, c, A, B, bias, res):
        self.c = c
        M, N, batch = c["M"], c["N"], c["batch"]
        self.a = self._place(A.transpose(1, 2) if c["ta"] else A, c["a_off"], c["sa"], c["lda"])
        self.b = self._place(B.transpose(1, 2) if c["tb"] else B, c["b_off"], c["sb"], c["ldb"])
        self.bias = None if bias is None else bias.float().to(DEV)
        self.res = None if res is None else self._place(res, c["c_off"], c["sc"], c["ldc"])
        n_c = c["c_off"] + (batch - 1) * c["sc"] + M * c["ldc"] + TAIL
        self.sentinel = (1.0e6 + (torch.arange(n_c, device=DEV) % 1021)).float()
        self.written = torch.zeros(n_c, dtype=torch.bool, device=DEV)
        self._view(self.written, batch, M, N, c["c_off"], c["sc"], c["ldc"]).fill_(True)

    @staticmethod
    def _view(buf, nb, rows, width, off, stride, ld):
        return torch.as_strided(buf, (nb, rows, width), (stride, ld, 1), off)

    def _place(self, x, off, stride, ld):
        nb, rows, width = x.shape
        buf = torch.full((off + (nb - 1) * stride + rows * ld + TAIL,), NAN, dtype=torch.float32)
        self._view(buf, nb, rows, width, off, stride, ld).copy_(x)
        return buf.to(DEV)

    def run(self, batch=None, element=0):
        """-> (C sub-matrices [batch, M, N], the whole C buffer).  batch = 1, element = e: batch element e as a call of its own."""
        c = self.c
        nb = c["batch"] if batch is None else batch
        out = self.sentinel.clone()
        T_.gemm(self.a, self.b, ta=bool(c["ta"]), tb=bool(c["tb"]), bias=self.bias, residual=self.res, alpha=c["alpha2"] / 2, out=out,
                m=c["M"], n=c["N"], k=c["K"], lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"], a_off=c["a_off"] + element * c["sa"],
                b_off=c["b_off"] + element * c["sb"], c_off=c["c_off"] + element * c["sc"], batch=nb, sa=c["sa"], sb=c["sb"], sc=c["sc"],
                relu=bool(c["relu"]))
        return self._view(out, nb, c["M"], c["N"], c["c_off"] + element * c["sc"], c["sc"], c["ldc"]), out

    def untouched(self, out):
        return bool((out == self.sentinel)[~self.written].all())


def _reference(c, A, B, bias, res, dtype, dev):
    """relu?(alpha op(A) op(B) + bias + residual) [batch, M, N] in `dtype` on `dev`"""
    y = (c["alpha2"] / 2) * torch.matmul(A.to(dev, dtype), B.to(dev, dtype)).expand(c["batch"], -1, -1)
    if bias is not None:
        y = y + bias.to(dev, dtype)
    if res is not None:
        y = y + res.to(dev, dtype)
    return torch.relu(y) if c["relu"] else y


def _data(c, seed, integer):
    gen = torch.Generator().manual_seed(seed)
    M, N, K, batch = c["M"], c["N"], c["K"], c["batch"]
    nbA = 1 if (batch > 1 and c["sa"] == 0) else batch
    nbB = 1 if (batch > 1 and c["sb"] == 0) else batch

    def draw(*shape):
        if integer:
            return torch.randint(-8, 9, shape, generator=gen).double()
        return torch.randn(shape, generator=gen, dtype=torch.float32).double()

    A, B = draw(nbA, M, K), draw(nbB, K, N)
    bias = draw(N) if c["bias"] else None
    res = draw(batch, M, N) if c["res"] else None
    return A, B, bias, res


# ---- 1. every case, exactly ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(TABLE)), ids=_id)
def test_gemm_form_exact_on_integers(i):
    c = TABLE[i]
    A, B, bias, res = _data(c, 1000 + i, integer=True)
    ops = Operands(c, A, B, bias, res)
    got, out = ops.run()
    torch.cuda.synchronize()
    ref = _reference(c, A, B, bias, res, torch.float64, DEV)
    assert bool(((2 * ref).round().long().double() == 2 * ref).all()) and float(ref.abs().max()) < 2 ** 23     # exact in float64 and in fp32
    bad = (got.double() != ref).nonzero()
    assert bad.numel() == 0, (f"case {_id(i)} {c}: {bad.shape[0]} of {ref.numel()} entries differ, first at (b, row, col) = {bad[0].tolist()}: "
                              f"got {float(got[tuple(bad[0])])}, want {float(ref[tuple(bad[0])])}")
    assert ops.untouched(out), f"case {_id(i)}: C was written outside the [{c['M']}, {c['N']}] sub-matrices"


# ---- 2. a NaN and an inf stay in their row -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("i", [i for i, c in enumerate(TABLE) if c["flags"] & 4], ids=_id)
def test_gemm_nonfinite_entries_stay_in_their_row(i, relu):
    """Both kernels and the split-K reduction, without and with the ReLU: a ReLU written as fmaxf(v, 0) returns 0 for a NaN
    and would hand on a clean row (torch's relu keeps the NaN)."""
    c = dict(TABLE[i], relu=relu)
    A, B, bias, res = _data(c, 2000 + i, integer=True)
    r = c["M"] // 2
    A[0, r, 1], A[0, r, c["K"] - 2] = NAN, INF
    ops = Operands(c, A, B, bias, res)
    got, out = ops.run()
    hit = torch.zeros(c["batch"], c["M"], dtype=torch.bool, device=DEV)
    hit[(slice(None) if A.shape[0] == 1 else 0), r] = True          # a shared A carries its row into every batch element
    assert bool((~torch.isfinite(got[hit])).all()), f"case {_id(i)}: finite entries in the row of the NaN"
    A[0, r, 1], A[0, r, c["K"] - 2] = 0.0, 0.0
    ref = _reference(c, A, B, bias, res, torch.float64, DEV)
    assert bool((got.double() == ref)[~hit].all()), f"case {_id(i)}: a row without NaN / inf is not exact"
    assert ops.untouched(out)


# ---- 3. real-valued data against float64 -------------------------------------------------------------------------------------------
ROUNDING = [i for i, c in enumerate(TABLE) if c["flags"] & 1]
_worst = collections.defaultdict(float)


@pytest.mark.parametrize("i", ROUNDING, ids=_id)
def test_gemm_form_against_float64(i):
    c = TABLE[i]
    A, B, bias, res = _data(c, 3000 + i, integer=False)
    ops = Operands(c, A, B, bias, res)
    got, out = ops.run()
    ref = _reference(c, A, B, bias, res, torch.float64, DEV)
    ref32 = _reference(c, A, B, bias, res, torch.float32, "cpu")
    rep = check_close({"C": got}, {"C": ref}, {"C": ref32}, what=f"gemm case {_id(i)}: ")
    err, tol = rep["C"]
    # the kernel family, for the printed figure only (the plan itself is held by tests/test_gemm_plan_host.py)
    friendly = all(c[k] % 4 == 0 for k in ("a_off", "b_off", "lda", "ldb", "sa", "sb"))
    family = ("lds" if friendly and (c["M"] if c["ta"] else c["K"]) % 4 == 0 and (c["K"] if c["tb"] else c["N"]) % 4 == 0 and
              min(c["M"], c["N"], c["K"]) >= 4 else "f32")
    _worst[family] = max(_worst[family], err / tol)
    print(f"gemm case {_id(i)}: family {family} err {err:.3e} tol {tol:.3e} err/tol {err / tol:.3f}; worst so far {dict(_worst)}")
    assert ops.untouched(out)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("i", [i for i, c in enumerate(TABLE) if c["flags"] & 2], ids=_id)
def test_gemm_split_k_bits_do_not_depend_on_the_run_or_the_batch(i):
    c = TABLE[i]
    assert c["batch"] > 1
    A, B, bias, res = _data(c, 4000 + i, integer=False)
    ops = Operands(c, A, B, bias, res)
    first, _ = ops.run()
    second, _ = ops.run()
    assert torch.equal(_bits(first), _bits(second)), f"case {_id(i)}: two runs differ"
    alone, out = ops.run(batch=1, element=1)
    assert torch.equal(_bits(alone[0]), _bits(first[1])), f"case {_id(i)}: batch element 1 alone differs from the batched call"
    written = ops.written.clone()
    ops.written.zero_()
    ops._view(ops.written, 1, c["M"], c["N"], c["c_off"] + c["sc"], c["sc"], c["ldc"]).fill_(True)
    assert ops.untouched(out)
    ops.written = written
