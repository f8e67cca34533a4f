"""Sparse convolution over up to 6-D coordinates and DGR's inlier network ResUNetBN2C
(reference: GMF_DeepGlobalRegistration/*/model/resunet_new.py:424-721, model/residual_block.py, model/common.py).  The module's
forward is eval-mode; `sparse_conv_train` (the convolution's autograd Function: weight gradient `sparse_conv_wgrad`, data
gradient `sparse_conv_dgrad`) and gmf_amd.train.resunet_train are the train-mode path.  Kernels: csrc/sparse_kernels.hip,
csrc/sparse_train_kernels.hip.

The coordinate engine (`SparsePlan`) takes MinkowskiEngine's batched coordinates, int32 [M, 1 + D] with the batch index in
column 0, and builds on the device every coarser level (unique floor(c / 2t) * 2t, batch kept, ascending in (batch, c_1 ..
c_D); level 0 is the input rows in input order) and every kernel map the network needs.  All buffers are sized from M and k^D
and the row counts stay on the device, so a forward makes no host synchronisation and can be captured into a graph.
`sparse_conv` is one convolution over a map of a plan with the fused epilogue (folded BatchNorm, residual, ReLU, bias) and
two-source input ([x_a | x_b], MinkowskiEngine's ME.cat without materialising it).  fp32 throughout; each output element sums
its offsets in ascending order and its input channels in order, without float atomics, so results are bitwise repeatable and
independent of the input row order.

Conventions read from MinkowskiEngine v0.5 and not verified against it ("Sparse inlier network"): the offset
index inside `kernel` has the first spatial axis varying fastest (`kernel_offsets`); `kernel` is [Cin, Cout] when k^D = 1
(`kernel_shape`); `bias` is [1, Cout]; a coarse coordinate is floor(c / 2t) * 2t for negative c too (csrc: coarse_coord).
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _lib
from ._args import fail
from ._util import WeightWatcher, handle_and_stream
from .perceiver_io import PerceiverIO
from .pointdsc import ImageEncoder

MAX_D = 6
MAX_KERNEL_VOLUME = 1024
MAX_LEVELS = 8
MAX_MAPS = 16


def kernel_volume(kernel_size: int, D: int) -> int:
    return int(kernel_size) ** int(D)


def kernel_offsets(kernel_size: int, D: int):
    """The offset of each index d of a hypercube kernel, the first spatial axis varying fastest (MinkowskiEngine's order, an
    assumption: INTEGRATION.md).  The device maps (csrc: neighbour_key) follow the same rule."""
    k = int(kernel_size)
    out = []
    for d in range(k ** D):
        out.append(tuple((d // k ** a) % k - k // 2 for a in range(D)))
    return out


def kernel_shape(kernel_size: int, D: int, cin: int, cout: int):
    """MinkowskiEngine's `kernel` parameter: [k^D, Cin, Cout], or [Cin, Cout] when k^D = 1 (an assumption: INTEGRATION.md)."""
    K = kernel_volume(kernel_size, D)
    return (K, cin, cout) if K > 1 else (cin, cout)


def _check_map_desc(maps, D, levels, what):
    out = []
    for m in maps:
        k, o, i = (int(v) for v in m)
        if k < 1 or k % 2 == 0:
            fail(what, f"kernel size {k} must be odd and >= 1")
        if k ** D > MAX_KERNEL_VOLUME:
            fail(what, f"kernel volume {k}^{D} = {k ** D} exceeds {MAX_KERNEL_VOLUME}", NotImplementedError)
        if not (0 <= o < levels and 0 <= i < levels and abs(o - i) <= 1):
            fail(what, f"map ({k}, {o}, {i}): levels must exist and differ by at most one")
        out.append((k, o, i))
    if len(out) > MAX_MAPS:
        fail(what, f"at most {MAX_MAPS} kernel maps")
    return out


def check_coords(coords, what="SparsePlan"):
    """Shape / dtype / device checks of MinkowskiEngine batched coordinates [M, 1 + D] int32; returns (M, D)."""
    if not isinstance(coords, torch.Tensor):
        fail(what, "`coords` must be a torch tensor")
    if coords.dtype != torch.int32:
        fail(what, f"`coords` must be int32 (got {coords.dtype})")
    if coords.dim() != 2 or coords.shape[0] == 0 or not (2 <= coords.shape[1] <= 1 + MAX_D):
        fail(what, f"`coords` must be a non-empty [M, 1 + D] tensor with D in 1..{MAX_D} (got {tuple(coords.shape)})")
    if not coords.is_cuda:
        fail(what, f"`coords` must live on a HIP device (got {coords.device}); the HIP path is mandatory, there is no CPU fallback")
    return coords.shape[0], coords.shape[1] - 1


class SparsePlan:
    """Levels and kernel maps of one coordinate set, on the device (`gmf_sparse_build_plan`).

    maps: (k, out level, in level) triples.  Same level: output o reads input o + d t; out = in + 1 (downsampling): o + d t with
    t the input stride; out = in - 1 (transposed): fine output p reads coarse input o when p = o + d t.  Every level has M
    row slots; `counts[l]` (device int32) says how many are used.  A duplicate input row raises at the next
    `gmf_amd.check_status()` (or the next forward of a module on the device)."""

    def __init__(self, coords, levels: int, maps=()):
        self.M, self.D = check_coords(coords)
        if not (1 <= levels <= MAX_LEVELS):
            fail("SparsePlan", f"levels must be in 1..{MAX_LEVELS}")
        self.levels = int(levels)
        self.maps = _check_map_desc(maps, self.D, self.levels, "SparsePlan")
        self.K = [kernel_volume(k, self.D) for k, _, _ in self.maps]
        coords = coords.contiguous()
        h, st = handle_and_stream(coords)
        flat = [v for m in self.maps for v in m] or [0]
        desc = (ctypes.c_int * len(flat))(*flat)
        nbytes = ctypes.c_longlong(0)
        h.check(h.lib.gmf_sparse_plan_bytes(h.h, self.M, self.D, self.levels, len(self.maps), desc, ctypes.byref(nbytes)),
                "gmf_sparse_plan_bytes")
        self.buf = torch.empty(nbytes.value, dtype=torch.uint8, device=coords.device)
        offs = (ctypes.c_longlong * (1 + self.levels + 4 * len(self.maps)))()
        h.call("gmf_sparse_build_plan", coords.data_ptr(), self.M, self.D, self.levels, len(self.maps), desc,
               self.buf.data_ptr(), nbytes.value, offs, st)
        self._offs = list(offs)
        self._coords_keepalive = coords

    def _view(self, off, n, dtype):
        b = self.buf[off:off + n * torch.empty((), dtype=dtype).element_size()]
        return b.view(dtype)

    @property
    def counts(self) -> torch.Tensor:
        """int32 [levels] on the device: rows used in each level."""
        return self._view(self._offs[0], 16, torch.int32)[:self.levels]

    def count_ptr(self, level: int) -> int:
        return self.buf.data_ptr() + self._offs[0] + 4 * int(level)

    def level_coords(self, level: int) -> torch.Tensor:
        """int32 [M, 1 + D] on the device: the rows of a level (only the first counts[level] are valid)."""
        v = self._view(self._offs[1 + level], self.M * 8, torch.int32).view(self.M, 8)
        return v[:, :1 + self.D]

    def kernel_map(self, m: int):
        """(row_ptr int32 [M + 1], pairs int32 [M * K, 2]) of map m, on the device: CSR over the output rows of
        (offset index, input row), ascending offset per row."""
        base = 1 + self.levels + 4 * m
        rp = self._view(self._offs[base], self.M + 1, torch.int32)
        pairs = self._view(self._offs[base + 1], self.M * self.K[m] * 2, torch.int32).view(self.M * self.K[m], 2)
        return rp, pairs

    def offset_lists(self, m: int):
        """(by_off int32 [M * K], off_start int32 [K + 1]) of map m, on the device: the CSR pair indices sorted by offset
        (ascending output row within one offset); offset d's pairs are by_off[off_start[d]:off_start[d + 1]]."""
        base = 1 + self.levels + 4 * m
        return (self._view(self._offs[base + 2], self.M * self.K[m], torch.int32),
                self._view(self._offs[base + 3], self.K[m] + 1, torch.int32))

    def to_host(self):
        """Levels and maps as host tensors (synchronises; for tests and tools): {"counts", "levels": [[n_l, 1 + D]], "maps":
        [(row_ptr [n_out + 1], pairs [nnz, 2])]}."""
        n = self.counts.cpu().tolist()
        lv = [self.level_coords(l)[:n[l]].cpu() for l in range(self.levels)]
        mp = []
        for m, (_, o, _) in enumerate(self.maps):
            rp, pairs = self.kernel_map(m)
            rp = rp[:n[o] + 1].cpu()
            mp.append((rp, pairs[:int(rp[-1])].cpu()))
        return {"counts": n, "levels": lv, "maps": mp}


def _f32_dev(t, name, what):
    if not isinstance(t, torch.Tensor):
        fail(what, f"`{name}` must be a torch tensor")
    if not t.is_cuda:
        fail(what, f"`{name}` must live on a HIP device (got {t.device}); the HIP path is mandatory, there is no CPU fallback")
    if t.dtype != torch.float32:
        fail(what, f"`{name}` must be float32 (got {t.dtype})")
    return t.contiguous()


def _check_sources(xa, xb, M, what):
    """The two-source input [xa | xb] of a convolution, xa already through `_f32_dev`: (xb or None, ca, cb)."""
    if xa.dim() != 2 or xa.shape[0] != M:
        fail(what, f"`xa` must be [M = {M}, ca] (got {tuple(xa.shape)})")
    if xb is None:
        return None, xa.shape[1], 0
    xb = _f32_dev(xb, "xb", what)
    if xb.dim() != 2 or xb.shape[0] != M:
        fail(what, f"`xb` must be [M = {M}, cb] (got {tuple(xb.shape)})")
    return xb, xa.shape[1], xb.shape[1]


def _check_epilogue(scale, shift, residual, M, cout, what):
    """[scale, shift, residual] of a convolution's fused epilogue, each None or checked: scale / shift hold cout values,
    residual is [M, cout]."""
    vecs = []
    for name, v, shape in (("scale", scale, (cout,)), ("shift", shift, (cout,)), ("residual", residual, (M, cout))):
        if v is not None:
            v = _f32_dev(v, name, what)
            if tuple(v.shape) != shape and not (name != "residual" and v.numel() == cout):
                fail(what, f"`{name}` must be {list(shape)} (got {tuple(v.shape)})")
        vecs.append(v)
    return vecs


def _check_out(out, M, cout, inputs, what, device):
    if out is None:
        return torch.empty((M, cout), dtype=torch.float32, device=device)
    if out.shape != (M, cout) or out.dtype != torch.float32 or not out.is_contiguous():
        fail(what, f"`out` must be a contiguous float32 [{M}, {cout}] tensor")
    for name, t in inputs:
        if t is not None and _overlap(out, t):
            fail(what, f"`out` overlaps `{name}`: the convolution cannot run in place")
    return out


def _map_arrays(plan, map_index, out_level, what):
    if map_index is None:
        return 1, None, None, None, None
    if plan.maps[map_index][1] != out_level:
        fail(what, f"map {map_index} writes level {plan.maps[map_index][1]}, not {out_level}")
    rp, pairs = plan.kernel_map(map_index)
    by_off, off_start = plan.offset_lists(map_index)
    return plan.K[map_index], rp, pairs, by_off, off_start


def sparse_conv(plan: SparsePlan, map_index, out_level: int, xa, W, xb=None, scale=None, shift=None, residual=None,
                relu: bool = False, nsplit: int = 1, out=None):
    """One sparse convolution over kernel map `map_index` of `plan` (None: the identity map, k = 1) into level `out_level`.

    xa [M, ca] (and xb [M, cb]: the input is [xa | xb]) hold the input level's rows; W is MinkowskiEngine's `kernel`,
    [K, ca + cb, cout] (or [ca + cb, cout] when K = 1).  y = v * scale + shift (one fma; absent: 1 / 0), + residual [M, cout],
    then ReLU if `relu` (a NaN stays a NaN, as in torch.relu).  Returns out [M, cout]; only the first counts[out_level] rows are written.  `out` must not overlap any
    input (other workgroups would read rows it has already overwritten).  nsplit (1..K; 1 for the identity map) cuts the
    offsets into fixed slices that run on separate workgroups: it changes how the sum is grouped, so keep it fixed per layer
    for bitwise-equal results."""
    what = "sparse_conv"
    xa = _f32_dev(xa, "xa", what)
    W = _f32_dev(W, "W", what)
    M = plan.M
    xb, ca, cb = _check_sources(xa, xb, M, what)
    K, rp, pairs, by_off, off_start = _map_arrays(plan, map_index, out_level, what)
    if W.dim() == 2 and K == 1:
        W = W.unsqueeze(0)
    if W.dim() != 3 or W.shape[0] != K or W.shape[1] != ca + cb:
        fail(what, f"`W` must be [K = {K}, Cin = {ca + cb}, Cout] (got {tuple(W.shape)})")
    cout = W.shape[2]
    vecs = _check_epilogue(scale, shift, residual, M, cout, what)
    if not (1 <= int(nsplit) <= K):
        fail(what, f"nsplit must be in 1..K = {K}")
    out = _check_out(out, M, cout, (("xa", xa), ("xb", xb), ("W", W), ("scale", vecs[0]), ("shift", vecs[1]),
                                    ("residual", vecs[2])), what, xa.device)
    h, st = handle_and_stream(xa)
    h.call("gmf_sparse_conv", _lib.ptr(rp), _lib.ptr(pairs), _lib.ptr(by_off), _lib.ptr(off_start), K, plan.count_ptr(out_level), M,
           xa.data_ptr(), ca, _lib.ptr(xb), cb, W.data_ptr(), cout, _lib.ptr(vecs[0]), _lib.ptr(vecs[1]), _lib.ptr(vecs[2]),
           1 if relu else 0, int(nsplit), out.data_ptr(), st)
    return out


def sparse_conv_wgrad(plan: SparsePlan, map_index, out_level: int, xa, dy, xb=None):
    """Weight gradient of `sparse_conv` (`gmf_sparse_conv_wgrad`): dW [K, ca + cb, cout] = per offset d the sum over d's pairs
    (i -> o, o < counts[out_level]) of [xa | xb][i]^T dy[o]; exactly 0 for an offset without pairs.  Each offset's pair list is
    cut into fixed chunks added in chunk order (a function of the map and K): bitwise repeatable."""
    what = "sparse_conv_wgrad"
    xa = _f32_dev(xa, "xa", what)
    dy = _f32_dev(dy, "dy", what)
    M = plan.M
    if xa.dim() != 2 or xa.shape[0] != M or dy.dim() != 2 or dy.shape[0] != M:
        fail(what, f"`xa` and `dy` must be [M = {M}, C] (got {tuple(xa.shape)}, {tuple(dy.shape)})")
    xb, ca, cb = _check_sources(xa, xb, M, what)
    K, rp, pairs, by_off, off_start = _map_arrays(plan, map_index, out_level, what)
    cout = dy.shape[1]
    dW = torch.empty((K, ca + cb, cout), dtype=torch.float32, device=xa.device)
    h, st = handle_and_stream(xa)
    h.call("gmf_sparse_conv_wgrad", _lib.ptr(rp), _lib.ptr(pairs), _lib.ptr(by_off), _lib.ptr(off_start), K, plan.count_ptr(out_level),
           xa.data_ptr(), ca, _lib.ptr(xb), cb, dy.data_ptr(), cout, dW.data_ptr(), st)
    return dW


def transposed_map(plan: SparsePlan, map_index):
    """(index of the map (k, in, out) of `plan`, flip): the data gradient of a convolution over map (k, out, in) is a convolution
    over its transposed map with W'[d] = W[s(d)]^T, s the identity for a strided map (down <-> transposed, same offset index) and
    the flip d -> K - 1 - d for a same-level map (the map is its own transpose; the offset of K - 1 - d is minus that of d).  The
    identity map (None) is its own transpose."""
    if map_index is None:
        return None, False
    k, o, i = plan.maps[map_index]
    if o == i:
        return map_index, True
    if (k, i, o) not in plan.maps:
        fail("sparse_conv_dgrad", f"the plan has no map ({k}, {i}, {o}), the transpose of map {map_index}")
    return plan.maps.index((k, i, o)), False


def sparse_conv_dgrad(plan: SparsePlan, map_index, out_level: int, dy, W):
    """Data gradient of `sparse_conv` over map `map_index` (out level `out_level`): dx [M, cin] = `sparse_conv` of dy over the
    transposed map with W'[d] = W[s(d)]^T ([K, cout, cin]), into the input level; rows >= counts[in level] are 0."""
    W = W if W.dim() == 3 else W.unsqueeze(0)
    if map_index is None:
        in_level, tmap, flip = out_level, None, False
    else:
        in_level = plan.maps[map_index][2]
        tmap, flip = transposed_map(plan, map_index)
    Wt = (W.flip(0) if flip else W).transpose(1, 2).contiguous()
    K, cout, cin = Wt.shape
    dx = torch.zeros((plan.M, cin), dtype=torch.float32, device=dy.device)
    return sparse_conv(plan, tmap, in_level, dy, Wt, nsplit=layer_nsplit(K, cout, cin), out=dx)


class _SparseConvFn(torch.autograd.Function):
    """y = relu?(sparse_conv([xa | xb], W) + bias) over one map of a plan, differentiable in xa, xb, W and bias.  Backward:
    dW by `sparse_conv_wgrad`, [dxa | dxb] by `sparse_conv_dgrad` (only for an input that needs it), dbias by a column sum; the
    ReLU masks dy by the saved output (gmf_relu_backward).  Rows of y past counts[out_level] are not written; rows of dx past
    the input level's count are 0."""

    @staticmethod
    def forward(ctx, plan, map_index, out_level, xa, xb, W, bias, relu):
        W3 = W.detach() if W.dim() == 3 else W.detach().unsqueeze(0)
        y = sparse_conv(plan, map_index, out_level, xa.detach(), W3, xb=None if xb is None else xb.detach(),
                        shift=None if bias is None else bias.detach().reshape(-1), relu=relu,
                        nsplit=layer_nsplit(W3.shape[0], W3.shape[1], W3.shape[2]))
        ctx.plan, ctx.map_index, ctx.out_level, ctx.relu = plan, map_index, out_level, relu
        ctx.wshape, ctx.has_b, ctx.ca, ctx.has_xb = W.shape, bias is not None, xa.shape[1], xb is not None
        ctx.save_for_backward(xa.detach(), xb.detach() if xb is not None else None, W3, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .train import colsum, relu_backward
        xa, xb, W3, y = ctx.saved_tensors
        plan = ctx.plan
        dy = _f32_dev(dy, "grad", "sparse_conv backward")
        if ctx.relu:
            dy = relu_backward(dy, y)
        dW = db = dxa = dxb = None
        if ctx.needs_input_grad[5]:
            dW = sparse_conv_wgrad(plan, ctx.map_index, ctx.out_level, xa, dy, xb=xb).reshape(ctx.wshape)
        if ctx.has_b and ctx.needs_input_grad[6]:
            db = colsum(dy).reshape(1, -1)
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            dx = sparse_conv_dgrad(plan, ctx.map_index, ctx.out_level, dy, W3)
            dxa = dx[:, :ctx.ca] if ctx.needs_input_grad[3] else None
            dxb = dx[:, ctx.ca:] if ctx.has_xb and ctx.needs_input_grad[4] else None
        return None, None, None, dxa, dxb, dW, db, None


def sparse_conv_train(plan: SparsePlan, map_index, out_level: int, xa, W, xb=None, bias=None, relu: bool = False):
    """Differentiable `sparse_conv` (no folded BatchNorm, no residual): relu?([xa | xb] (*) W + bias).  W is MinkowskiEngine's
    `kernel` ([K, Cin, Cout], or [Cin, Cout] when K = 1); a bias [1, Cout] only into level 0, where every row is valid (its
    gradient sums all M rows)."""
    if bias is not None and out_level != 0:
        fail("sparse_conv_train", "a bias is supported into level 0 only")
    return _SparseConvFn.apply(plan, map_index, out_level, xa, xb, W, bias, bool(relu))


def sparse_conv_narrow(plan: SparsePlan, map_index: int, out_level: int, x, W, scale=None, shift=None, residual=None,
                       relu: bool = False, out=None):
    """`sparse_conv` for a narrow input (Cin <= 8, Cout <= 64; FCGF's conv1), on `gmf_sparse_conv_narrow`: one fma chain per
    output element over its row's pairs in ascending offset, channels in order inside a pair.  x [M, Cin], W [K, Cin, Cout]
    (or [Cin, Cout] for a k = 1 map); map_index must name a map of the plan (the identity map has no CSR).  Same epilogue, row
    count rule and `out` rule as `sparse_conv`."""
    what = "sparse_conv_narrow"
    x = _f32_dev(x, "x", what)
    W = _f32_dev(W, "W", what)
    M = plan.M
    if x.dim() != 2 or x.shape[0] != M:
        fail(what, f"`x` must be [M = {M}, cin] (got {tuple(x.shape)})")
    if map_index is None or not (0 <= int(map_index) < len(plan.maps)):
        fail(what, "`map_index` must name a kernel map of the plan")
    K = plan.K[map_index]
    if plan.maps[map_index][1] != out_level:
        fail(what, f"map {map_index} writes level {plan.maps[map_index][1]}, not {out_level}")
    if W.dim() == 2 and K == 1:
        W = W.unsqueeze(0)
    cin = x.shape[1]
    if W.dim() != 3 or W.shape[0] != K or W.shape[1] != cin:
        fail(what, f"`W` must be [K = {K}, Cin = {cin}, Cout] (got {tuple(W.shape)})")
    cout = W.shape[2]
    if not (1 <= cin <= 8 and 1 <= cout <= 64):
        fail(what, f"Cin must be in 1..8 and Cout in 1..64 (got {cin}, {cout})", NotImplementedError)
    vecs = _check_epilogue(scale, shift, residual, M, cout, what)
    out = _check_out(out, M, cout, (("x", x), ("W", W), ("scale", vecs[0]), ("shift", vecs[1]), ("residual", vecs[2])), what,
                     x.device)
    rp, pairs = plan.kernel_map(map_index)
    h, st = handle_and_stream(x)
    h.call("gmf_sparse_conv_narrow", rp.data_ptr(), pairs.data_ptr(), K, plan.count_ptr(out_level), M, x.data_ptr(), cin,
           W.data_ptr(), cout, _lib.ptr(vecs[0]), _lib.ptr(vecs[1]), _lib.ptr(vecs[2]), 1 if relu else 0, out.data_ptr(), st)
    return out


def sparse_conv_narrow_wgrad(plan: SparsePlan, map_index: int, out_level: int, x, dy):
    """Weight gradient of `sparse_conv_narrow` (`gmf_sparse_conv_narrow_wgrad`; Cin <= 8, Cout <= 64, FCGF's conv1): dW [K, Cin,
    Cout] as `sparse_conv_wgrad` defines it, exactly 0 for an offset without pairs.  x [M, Cin], dy [M, Cout]; map_index must name
    a map of the plan.  One wave per chunk of an offset's pair list, lane = output channel; chunks of a fixed size added in chunk
    order (a function of the map, K and Cout): bitwise repeatable."""
    what = "sparse_conv_narrow_wgrad"
    x = _f32_dev(x, "x", what)
    dy = _f32_dev(dy, "dy", what)
    M = plan.M
    if x.dim() != 2 or x.shape[0] != M or dy.dim() != 2 or dy.shape[0] != M:
        fail(what, f"`x` and `dy` must be [M = {M}, C] (got {tuple(x.shape)}, {tuple(dy.shape)})")
    if map_index is None or not (0 <= int(map_index) < len(plan.maps)):
        fail(what, "`map_index` must name a kernel map of the plan")
    cin, cout = x.shape[1], dy.shape[1]
    if not (1 <= cin <= 8 and 1 <= cout <= 64):
        fail(what, f"Cin must be in 1..8 and Cout in 1..64 (got {cin}, {cout})", NotImplementedError)
    K, rp, pairs, by_off, off_start = _map_arrays(plan, map_index, out_level, what)
    dW = torch.empty((K, cin, cout), dtype=torch.float32, device=x.device)
    h, st = handle_and_stream(x)
    h.call("gmf_sparse_conv_narrow_wgrad", rp.data_ptr(), pairs.data_ptr(), by_off.data_ptr(), off_start.data_ptr(), K,
           plan.count_ptr(out_level), x.data_ptr(), cin, dy.data_ptr(), cout, dW.data_ptr(), st)
    return dW


class _SparseConvNarrowFn(torch.autograd.Function):
    """y = sparse_conv_narrow(x, W) over one map of a plan, differentiable in W only (a network's first convolution: its input
    needs no gradient).  Backward: `sparse_conv_narrow_wgrad`."""

    @staticmethod
    def forward(ctx, plan, map_index, out_level, x, W):
        W3 = W.detach() if W.dim() == 3 else W.detach().unsqueeze(0)
        ctx.plan, ctx.map_index, ctx.out_level, ctx.wshape = plan, map_index, out_level, W.shape
        ctx.save_for_backward(x.detach())
        return sparse_conv_narrow(plan, map_index, out_level, x.detach(), W3)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dW = None
        if ctx.needs_input_grad[4]:
            dy = _f32_dev(dy, "grad", "sparse_conv_narrow backward")
            dW = sparse_conv_narrow_wgrad(ctx.plan, ctx.map_index, ctx.out_level, x, dy).reshape(ctx.wshape)
        return None, None, None, None, dW


def sparse_conv_narrow_train(plan: SparsePlan, map_index: int, out_level: int, x, W):
    """`sparse_conv_narrow` with its weight gradient (`sparse_conv_narrow_wgrad`); x gets no gradient and must not need one."""
    if isinstance(x, torch.Tensor) and x.requires_grad:
        fail("sparse_conv_narrow_train", "`x` requires a gradient: the narrow convolution has no data gradient "
             "(use sparse_conv_train)", NotImplementedError)
    return _SparseConvNarrowFn.apply(plan, map_index, out_level, x, W)


def sparse_head_l2(plan: SparsePlan, level: int, xa, W1, W2, xb=None, bias=None, normalize: bool = False, out=None):
    """FCGF's head (resunet.py:641-648) on `gmf_sparse_head_l2`, one launch: y = relu([xa | xb] W1) W2 + bias, then, if
    `normalize`, y / (||y||_2 + 1e-8) per row.  xa [M, ca], xb [M, cb], W1 [ca + cb, hid] (or [1, ca + cb, hid]), W2 [hid, cout]
    (or [1, hid, cout]), bias [cout] or [1, cout]; every width at most 64.  Only the first counts[level] rows are written."""
    what = "sparse_head_l2"
    xa = _f32_dev(xa, "xa", what)
    M = plan.M
    xb, ca, cb = _check_sources(xa, xb, M, what)
    W1 = _f32_dev(W1, "W1", what)
    W2 = _f32_dev(W2, "W2", what)
    W1 = W1[0] if W1.dim() == 3 and W1.shape[0] == 1 else W1
    W2 = W2[0] if W2.dim() == 3 and W2.shape[0] == 1 else W2
    if W1.dim() != 2 or W1.shape[0] != ca + cb:
        fail(what, f"`W1` must be [ca + cb = {ca + cb}, hid] (got {tuple(W1.shape)})")
    hid = W1.shape[1]
    if W2.dim() != 2 or W2.shape[0] != hid:
        fail(what, f"`W2` must be [hid = {hid}, cout] (got {tuple(W2.shape)})")
    cout = W2.shape[1]
    if max(ca, cb, hid, cout) > 64:
        fail(what, f"every width must be at most 64 (ca {ca}, cb {cb}, hid {hid}, cout {cout})", NotImplementedError)
    if bias is not None:
        bias = _f32_dev(bias, "bias", what)
        if bias.numel() != cout:
            fail(what, f"`bias` must hold {cout} values (got {tuple(bias.shape)})")
    W1, W2 = W1.contiguous(), W2.contiguous()
    out = _check_out(out, M, cout, (("xa", xa), ("xb", xb), ("W1", W1), ("W2", W2), ("bias", bias)), what, xa.device)
    h, st = handle_and_stream(xa)
    h.call("gmf_sparse_head_l2", plan.count_ptr(level), M, xa.data_ptr(), ca, _lib.ptr(xb), cb, W1.data_ptr(), hid, W2.data_ptr(),
           cout, _lib.ptr(bias), 1 if normalize else 0, out.data_ptr(), st)
    return out


def _overlap(a, b) -> bool:
    """Whether two contiguous tensors share any byte."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def layer_nsplit(K: int, cin: int, cout: int) -> int:
    """Offset slices of one convolution of the network, a function of its shape alone (so every call groups its sums the same
    way).  A kernel of more than 16 MiB is read once per 64 pairs of an offset by one output-row group, and the slices give the
    parallelism: about 256 workgroups (slices x 64-channel blocks).  A smaller kernel runs in 9 slices and the device is filled
    by output-row groups (csrc/sparse_conv_plan.hpp: sparse_conv_row_groups).  The workspace holds nsplit x M x cout floats."""
    if K == 1:
        return 1
    if K * cin * cout * 4 > (16 << 20):
        return min(K, -(-256 // -(-cout // 64)))
    return min(K, 9)


def pack_resunet(sd, device):
    """The 23 convolutions of a ResUNetBN2C state_dict (the inlier network's or FCGF's: the same names) packed on `device` with
    their BatchNorms folded (`gmf_sparse_pack_resunet`): (blob, [(W [K, Cin, Cout], scale or None, shift or None)] in forward
    order, views into blob)."""
    arr, keep = _lib.tensor_list(sd)
    h, _ = handle_and_stream(torch.empty(0, device=device))
    layout = (ctypes.c_longlong * (6 * 23))()
    need = ctypes.c_longlong(0)
    h.check(h.lib.gmf_sparse_pack_resunet(h.h, arr, len(arr), None, 0, layout, ctypes.byref(need)), "gmf_sparse_pack_resunet")
    blob = torch.empty(need.value, dtype=torch.float32, device=device)
    h.check(h.lib.gmf_sparse_pack_resunet(h.h, arr, len(arr), ctypes.c_void_p(blob.data_ptr()), need.value, layout,
                                          ctypes.byref(need)), "gmf_sparse_pack_resunet")
    del keep
    layers = []
    for i in range(23):
        wo, so, ho, K, cin, cout = layout[6 * i:6 * i + 6]
        W = blob[wo:wo + K * cin * cout].view(K, cin, cout)
        layers.append((W, None if so < 0 else blob[so:so + cout], None if ho < 0 else blob[ho:ho + cout]))
    return blob, layers


# ---- ResUNetBN2C ------------------------------------------------------------------------------------------------------------
# The modules below only HOLD parameters under the reference's names (MinkowskiConvolution.kernel / .bias,
# MinkowskiBatchNorm.bn.*); the forward is `sparse_conv` over one plan per call.

class _MinkowskiConvolution(nn.Module):
    def __init__(self, cin, cout, kernel_size, D, bias=False):
        super().__init__()
        self.kernel_size = int(kernel_size)
        self.kernel = nn.Parameter(torch.empty(kernel_shape(kernel_size, D, cin, cout)))
        nn.init.normal_(self.kernel, std=(2.0 / (kernel_volume(kernel_size, D) * cin)) ** 0.5)
        if bias:
            self.bias = nn.Parameter(torch.zeros(1, cout))     # [1, Cout] (an assumption: INTEGRATION.md)


class _MinkowskiBatchNorm(nn.Module):
    def __init__(self, C, momentum):
        super().__init__()
        self.bn = nn.BatchNorm1d(C, momentum=momentum)


class _BasicBlockBN(nn.Module):          # residual_block.py:82-123 (no downsample)
    def __init__(self, C, momentum, D):
        super().__init__()
        self.conv1 = _MinkowskiConvolution(C, C, 3, D)
        self.norm1 = _MinkowskiBatchNorm(C, momentum)
        self.conv2 = _MinkowskiConvolution(C, C, 3, D)
        self.norm2 = _MinkowskiBatchNorm(C, momentum)


# Kernel maps of one forward: (k, out level, in level).  0-3 same-stride, 4-6 downsampling, 7-9 their transposes.
_NET_MAPS = [(3, 0, 0), (3, 1, 1), (3, 2, 2), (3, 3, 3), (3, 1, 0), (3, 2, 1), (3, 3, 2), (3, 0, 1), (3, 1, 2), (3, 2, 3)]

# The 23 convolutions of the network in forward order: (conv, its norm or None, index into _NET_MAPS, output level).  This is
# the order of kResunetLayers (csrc/gmf_api.cpp), so entry i is also entry i of `pack_resunet`'s list.  Map None is the identity
# map (k = 1); conv1's map stands for conv1_kernel_size = 3, `_ResUNet._plan` chooses it for the others.
TRUNK = (
    ("conv1", "norm1", 0, 0), ("block1.conv1", "block1.norm1", 0, 0), ("block1.conv2", "block1.norm2", 0, 0),                  # 0
    ("conv2", "norm2", 4, 1), ("block2.conv1", "block2.norm1", 1, 1), ("block2.conv2", "block2.norm2", 1, 1),                  # 3
    ("conv3", "norm3", 5, 2), ("block3.conv1", "block3.norm1", 2, 2), ("block3.conv2", "block3.norm2", 2, 2),                  # 6
    ("conv4", "norm4", 6, 3), ("block4.conv1", "block4.norm1", 3, 3), ("block4.conv2", "block4.norm2", 3, 3),                  # 9
    ("conv4_tr", "norm4_tr", 9, 2), ("block4_tr.conv1", "block4_tr.norm1", 2, 2), ("block4_tr.conv2", "block4_tr.norm2", 2, 2),   # 12
    ("conv3_tr", "norm3_tr", 8, 1), ("block3_tr.conv1", "block3_tr.norm1", 1, 1), ("block3_tr.conv2", "block3_tr.norm2", 1, 1),   # 15
    ("conv2_tr", "norm2_tr", 7, 0), ("block2_tr.conv1", "block2_tr.norm1", 0, 0), ("block2_tr.conv2", "block2_tr.norm2", 0, 0),   # 18
    ("conv1_tr", None, None, 0), ("final", None, None, 0))                                                                     # 21
CONV1_TR, FINAL = 21, 22


def resunet_trunk(layer, x, bottleneck=None):
    """conv1 .. block2_tr of the network (resunet_new.py:637-704, resunet.py:598-640) on level-0 features x: (out_s1_tr, out_s1),
    the two inputs of the head (conv1_tr on their ME.cat).  `layer(i, xa, xb=None, residual=None, relu=False)` runs convolution i
    of TRUNK on [xa | xb] with its norm, then the residual, then the ReLU; `bottleneck(out_s8)`, if given, stands between block4
    and conv4_tr.  Each block ends in a ReLU, so the reference's MEF.relu after it is a no-op."""
    def block(i, x):                           # residual_block.py:104-123
        h = layer(i, x, relu=True)
        return layer(i + 1, h, residual=x, relu=True)

    s1 = block(1, layer(0, x))
    s2 = block(4, layer(3, s1))
    s4 = block(7, layer(6, s2))
    s8 = block(10, layer(9, s4))
    if bottleneck is not None:
        s8 = bottleneck(s8)
    t4 = block(13, layer(12, s8))
    t2 = block(16, layer(15, t4, xb=s4))       # ME.cat(out_s4_tr, out_s4)
    t1 = block(19, layer(18, t2, xb=s2))
    return t1, s1


def _folded_conv(plan, where, L, i, xa, xb=None, residual=None, relu=False, out=None):
    """Convolution i of TRUNK in eval mode: `sparse_conv` with the folded BatchNorm of L (`pack_resunet`'s list) over the
    (map, level) of `where` (`_ResUNet._plan`)."""
    W, sc, sh = L[i]
    m, lvl = where[i]
    return sparse_conv(plan, m, lvl, xa, W, xb=xb, scale=sc, shift=sh, residual=residual, relu=relu,
                       nsplit=layer_nsplit(W.shape[0], W.shape[1], W.shape[2]), out=out)


class _ResUNet(nn.Module):
    """What DGR's two ResUNetBN2C networks share (the inlier network below, FCGF in fcgf.py): the constructor checks, the modules
    of TRUNK under the reference's names, the packed-weight cache, the input checks and the plan of one forward."""

    CHANNELS = [None, 32, 64, 128, 256]
    TR_CHANNELS = [None, 64, 64, 64, 128]
    REGION_TYPE = "HYPER_CUBE"
    _MODULE = ""                 # "fcgf." in gmf_amd.fcgf: the error texts name the class by its import path
    _NOT_PACKED = ()             # state_dict prefixes that `pack_resunet` does not read
    _NOT_WATCHED = None          # a prefix of parameters whose changes leave the packed weights valid

    def __init__(self, in_channels, out_channels, conv1_kernel_size, normalize_feature, D):
        super().__init__()
        what = self._what = self._MODULE + type(self).__name__
        if self.REGION_TYPE != "HYPER_CUBE":
            fail(what, f"only the hypercube kernel region is built (got {self.REGION_TYPE})", NotImplementedError)
        if not (1 <= int(D) <= MAX_D):
            fail(what, f"D must be in 1..{MAX_D} (got {D})", ValueError)
        for k in (conv1_kernel_size, 3):
            if k % 2 == 0 or k < 1:
                fail(what, f"kernel size {k} must be odd", ValueError)
            if kernel_volume(k, D) > MAX_KERNEL_VOLUME:
                fail(what, f"kernel volume {k}^{D} exceeds {MAX_KERNEL_VOLUME}", NotImplementedError)
        self.D, self.conv1_kernel_size = int(D), int(conv1_kernel_size)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.normalize_feature = bool(normalize_feature)
        self._packed, self._packed_version = None, None
        self._watch = WeightWatcher(self, skip_prefix=self._NOT_WATCHED)

    def _build_trunk(self, bn_momentum, before_block4=None):
        """Registers the modules of TRUNK in the reference's order (it fixes the state_dict's key order and the order of the
        constructor's random draws); `before_block4()` registers what the reference builds between norm4 and block4."""
        CH, TR, D = self.CHANNELS, self.TR_CHANNELS, self.D

        def stage(s, cin, cout, k=3):
            setattr(self, "conv" + s, _MinkowskiConvolution(cin, cout, k, D))
            setattr(self, "norm" + s, _MinkowskiBatchNorm(cout, bn_momentum))
            if s == "4" and before_block4 is not None:
                before_block4()
            setattr(self, "block" + s, _BasicBlockBN(cout, bn_momentum, D))

        stage("1", self.in_channels, CH[1], self.conv1_kernel_size)
        stage("2", CH[1], CH[2])
        stage("3", CH[2], CH[3])
        stage("4", CH[3], CH[4])
        stage("4_tr", CH[4], TR[4])
        stage("3_tr", CH[3] + TR[4], TR[3])
        stage("2_tr", CH[2] + TR[3], TR[2])
        self.conv1_tr = _MinkowskiConvolution(CH[1] + TR[2], TR[1], 1, D)
        self.final = _MinkowskiConvolution(TR[1], self.out_channels, 1, D, bias=True)

    # -- weights --------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._watch.invalidate()
        self._packed = None
        return out

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        if hasattr(self, "_watch"):
            self._watch.invalidate()
        return out

    def _weights(self, device):
        """The 23 convolutions packed with their BatchNorms folded (`gmf_sparse_pack_resunet`), rebuilt when a weight changes:
        [(W [K, Cin, Cout], scale or None, shift or None)] in the order of TRUNK."""
        key = (self._watch.version(), torch.device(device))
        if self._packed is None or self._packed_version != key:
            sd = {k: v for k, v in self.state_dict().items() if not k.startswith(self._NOT_PACKED)}
            self._packed, self._packed_version = pack_resunet(sd, device), key
        return self._packed[1]

    # -- forward --------------------------------------------------------------------------------------------------------------
    def _check_input(self, coords, feats):
        what = self._what
        M, D = check_coords(coords, what)
        if D != self.D:
            fail(what, f"coords have D = {D}, the network was built for D = {self.D}")
        feats = _f32_dev(feats, "feats", what)
        if feats.dim() != 2 or feats.shape != (M, self.in_channels):
            fail(what, f"`feats` must be [{M}, {self.in_channels}] (got {tuple(feats.shape)})")
        return feats

    def _plan(self, coords, conv1_needs_pairs=False):
        """(the plan of one forward, the (map index, level) of every convolution of TRUNK).  conv1 runs over map 0 for
        conv1_kernel_size 3, over the identity map (None) for 1, and over a map (k, 0, 0) of its own, appended to the plan, for
        any other size - and for 1 too when its kernel reads the map's pairs (`sparse_conv_narrow` has no identity form)."""
        maps = list(_NET_MAPS)
        k = self.conv1_kernel_size
        if k == 3:
            c1_map = 0
        elif k == 1 and not conv1_needs_pairs:
            c1_map = None
        else:
            c1_map = len(maps)
            maps.append((k, 0, 0))
        return SparsePlan(coords, 4, maps), [(c1_map, 0)] + [(m, lvl) for _, _, m, lvl in TRUNK[1:]]


# state_dict prefixes of the reference's image encoder that its forward never runs (resnet.py:147-152, 209-211); a strict
# load_state_dict of a DGR checkpoint hands them in, and they are accepted and dropped
_UNUSED_IMAGE_KEYS = ("img_encoder.backbone.layer3.", "img_encoder.backbone.layer4.", "img_encoder.backbone.fc.")


class ResUNetBN2C(_ResUNet):
    """DGR's inlier network (resunet_new.py:424-721 with ResUNetBN2C's channels), eval-mode forward on the device.

    forward(coords [M, 1 + D] int32, feats [M, in_channels] float32, p_image, q_image [1, 3, H, W]) -> [M, out_channels],
    aligned with the input rows.  p_tokens / q_tokens [1, T, 128] may replace the images (the image encoder's output, as in
    `PointDSC`).  The image pair has batch size 1 and the bottleneck's queries are all stride-8 rows as one sequence
    (resunet_new.py:694-701), in ascending (batch, coordinates) order: with pe=True the position encoding runs along that order
    (MinkowskiEngine's order there depends on its hash, so ours is a definition, not parity)."""

    _NOT_PACKED = ("img_encoder.", "image_fusion.", "perceiver_io.")
    _NOT_WATCHED = "img_encoder."

    def __init__(self, in_channels=3, out_channels=32, bn_momentum=0.1, conv1_kernel_size=3, normalize_feature=False, D=3,
                 pe=False):
        super().__init__(in_channels, out_channels, conv1_kernel_size, normalize_feature, D)
        if normalize_feature:
            fail(self._what, "normalize_feature=True is not built (DGR's inlier network uses False)", NotImplementedError)
        self.pe = bool(pe)
        CH = self.CHANNELS

        def perceiver_io():
            self.perceiver_io = PerceiverIO(depth=0, dim=128, latent_dim=CH[4], cross_heads=1, latent_heads=8,
                                            cross_dim_head=CH[4] // 2, latent_dim_head=CH[4] // 2, pe=self.pe)
        self._build_trunk(bn_momentum, before_block4=perceiver_io)
        self.img_encoder = ImageEncoder()
        self.image_fusion = PerceiverIO(depth=0, dim=128, latent_dim=128, cross_heads=1, latent_heads=8, cross_dim_head=64,
                                        latent_dim_head=64)
        for f in (self.image_fusion, self.perceiver_io):      # fp32 throughout, as the sparse convolutions
            f.split_fp16_ff = False
            f.split_fp16_attn = False

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = {k: v for k, v in state_dict.items() if not k.startswith(_UNUSED_IMAGE_KEYS)}
        return super().load_state_dict(sd, strict=strict, **kw)

    # -- forward --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_images(p_image, q_image, p_tokens, q_tokens):
        """Shapes only (no device needed).  The reference fuses ONE image pair: its bottleneck queries are all stride-8 rows as one
        sequence (resunet_new.py:697), which is ill-defined for an image batch > 1."""
        if p_tokens is not None or q_tokens is not None:
            pairs, shape = (("p_tokens", p_tokens), ("q_tokens", q_tokens)), "[1, T, 128]"
            ok = lambda t: t is not None and t.dim() == 3 and t.shape[0] == 1 and t.shape[2] == 128   # noqa: E731
        else:
            pairs, shape = (("p_image", p_image), ("q_image", q_image)), "[1, 3, H, W]"
            ok = lambda t: t is not None and t.dim() == 4 and t.shape[0] == 1 and t.shape[1] == 3     # noqa: E731
        for name, t in pairs:
            if t is None:
                raise RuntimeError("gmf_amd.ResUNetBN2C: pass p_image and q_image, or p_tokens and q_tokens")
            if not ok(t):
                raise RuntimeError(f"gmf_amd.ResUNetBN2C: `{name}` must be {shape}: the reference fuses one image pair "
                                   f"(got {tuple(t.shape)})")

    def _tokens(self, p_image, q_image, p_tokens, q_tokens):
        if p_tokens is None:
            p_tokens = self.img_encoder(p_image).flatten(2).permute(0, 2, 1).contiguous()
            q_tokens = self.img_encoder(q_image).flatten(2).permute(0, 2, 1).contiguous()
        return p_tokens, q_tokens

    def forward(self, coords, feats, p_image=None, q_image=None, p_tokens=None, q_tokens=None):
        if self.training:
            raise RuntimeError("gmf_amd.ResUNetBN2C: forward() is the eval-mode forward - call eval(); the differentiable "
                               "train-mode forward is gmf_amd.train.resunet_train(model, coords, feats, ...)")
        self._check_images(p_image, q_image, p_tokens, q_tokens)
        feats = self._check_input(coords, feats)
        with torch.no_grad():                     # forward-only: the image encoder takes its fused eval path too
            p_tok, q_tok = self._tokens(p_image, q_image, p_tokens, q_tokens)
            return self._forward(coords, feats, p_tok, q_tok)

    def _forward(self, coords, feats, p_tok, q_tok):
        L = self._weights(coords.device)
        plan, where = self._plan(coords)
        image_feat = self.image_fusion(p_tok, queries_encoder=q_tok)       # resunet_new.py:636

        def layer(i, xa, **kw):
            if TRUNK[i][0] == "block4.conv2":
                # the bottleneck's rows beyond counts[3] are zero: they pad the query sequence of the position encoding
                # (pe=True) as Conv1d's zero padding does
                kw["out"] = torch.zeros((plan.M, self.CHANNELS[4]), dtype=torch.float32, device=feats.device)
            return _folded_conv(plan, where, L, i, xa, **kw)

        def fuse(s8):                              # resunet_new.py:694-704
            return self.perceiver_io(image_feat, queries_encoder=s8.unsqueeze(0))[0]

        t1, s1 = resunet_trunk(layer, feats, bottleneck=fuse)
        o = layer(CONV1_TR, t1, xb=s1, relu=True)                     # conv1_tr on ME.cat(out_s1_tr, out_s1), MEF.relu
        return layer(FINAL, o)                                        # final (+ bias)


class ResUNetBN2CX(ResUNetBN2C):
    """resunet_new.py:724-725: the hyper-cross kernel region.  Not built: constructing it raises NotImplementedError."""
    REGION_TYPE = "HYPER_CROSS"


def inlier_coordinates(coords0, coords1, idx0, idx1):
    """The [M, 7] int32 rows of DGR's inlier network (deep_global_registration.py:297-298): (batch, voxel of the source point,
    voxel of its correspondence) = cat(coords0[idx0], coords1[idx1, 1:]).  coords0 / coords1 [N, 4] int (batch, x, y, z)."""
    for name, c in (("coords0", coords0), ("coords1", coords1)):
        if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 4 or c.dtype.is_floating_point:
            fail("inlier_coordinates", f"`{name}` must be an integer [N, 4] tensor (batch, x, y, z)")
    if idx0.shape != idx1.shape or idx0.dim() != 1:
        fail("inlier_coordinates", "`idx0` and `idx1` must be 1-D and of equal length")
    return torch.cat((coords0[idx0.long()], coords1[idx1.long(), 1:]), dim=1).to(torch.int32).contiguous()
