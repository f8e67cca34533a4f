"""The maximum-clique baseline of the reference's evaluation on the device: PMC(...) of
GMF_PointDSC/baseline_scripts/baseline_3DMatch.py:56-77, batched over ragged pairs and exact.  Kernels: csrc/clique_kernels.hip;
C ABI: gmf_max_clique, gmf_pmc_graph.

The reference builds the edge list of the pairwise-compatibility graph in a double Python loop and hands it to a prebuilt x86
binary.  Here the graph is a bit matrix built by one kernel, the search is a branch and bound with one wave per root, B pairs
share one chain of launches, nothing is read back and the call can be captured into a graph.  Differences from the reference:
INTEGRATION.md, "Maximum-clique baseline"."""
from __future__ import annotations

import torch

from ._args import (check_offsets, check_rows, device_offsets, fail, int_in_range, positive_finite, require_device, same_device,
                    uniform_offsets)
from ._util import handle_and_stream

MAX_ROWS = 8192                     # rows of one pair, at most (kPmcMaxN)
STEP_SLACK = 256                    # `steps` can pass `max_steps` by this much: one search wave per count (kPmcWaves)
DEFAULT_MAX_STEPS = 64 * 595_416    # 64 x the largest step count measured to the end of a search at N = 1000: DESIGN.md section 4n
_METRICS = {"squared": 0, "length": 1}


def _check_common(what, inlier_threshold, metric):
    tau = positive_finite(what, "inlier_threshold", inlier_threshold)
    if metric not in _METRICS:
        fail(what, f"metric must be 'squared' or 'length' (got {metric!r})")
    return tau, _METRICS[metric]


def max_clique_batched(corr, src_keypts, tgt_keypts, inlier_threshold, metric="squared", offsets=None, max_steps=None,
                       return_info=False):
    """A maximum clique of the pairwise-compatibility graph of each of B pairs, and Kabsch on its members (the reference's PMC,
    batched).

    corr [B,N,6], src_keypts, tgt_keypts [B,N,3] float32 (offsets None), or packed [sum N, .] with `offsets` (B + 1 ints, or
    an int32 device tensor; a pair may be empty).  Per pair of N <= 8192 rows:
      graph: in fp32, every operation rounded on its own, a = ((dx^2 + dy^2) + dz^2) on the differences of columns 0..2 of two
      rows and b alike on columns 3..5.  metric "squared" (the reference's rule): edge iff |a - b| < inlier_threshold;
      "length" (PointDSC's and SM's): edge iff |sqrt(a) - sqrt(b)| < inlier_threshold.  No diagonal;
      labels = 1 on the members of a maximum clique.  Where several exist the choice is the implementation's, and a function of
      the pair's rows alone: the same alone, in any batch and on every run, whenever `exact` is 1.  A graph without edges gives
      the smallest row alone (the reference raises there);
      T = rigid_transform_3d(src_keypts, tgt_keypts, labels): centroids over sum w + 1e-6, R = V diag(1, 1, det) U^T.  An empty
      pair gives the identity.
    max_steps bounds the branch-and-bound nodes expanded per pair (None: DEFAULT_MAX_STEPS); `steps` can pass it by STEP_SLACK at
    most.  Where the budget ends a search `exact` is 0 and the labels are the largest clique found.

    Returns trans [B,4,4] and labels (float 0 / 1, [B,N] or [sum N]); with return_info also size [B] int32, exact [B] int32,
    steps [B] int64 and degree (labels' shape, int32: the graph's row sums).
    No host synchronisation; the call can be captured into a graph."""
    what = "max_clique_batched"
    dims = 3 if offsets is None else 2
    check_rows(what, "corr", corr, dims, 6)
    check_rows(what, "src_keypts", src_keypts, dims, 3)
    check_rows(what, "tgt_keypts", tgt_keypts, dims, 3)
    if not corr.shape[:-1] == src_keypts.shape[:-1] == tgt_keypts.shape[:-1]:
        fail(what, f"corr, src_keypts and tgt_keypts must have equal row counts (got {tuple(corr.shape)} / "
                   f"{tuple(src_keypts.shape)} / {tuple(tgt_keypts.shape)})")
    if dims == 3 and corr.shape[0] == 0:
        fail(what, "the batch must hold at least one pair")
    tau, met = _check_common(what, inlier_threshold, metric)
    budget = DEFAULT_MAX_STEPS if max_steps is None else int_in_range(what, "max_steps", max_steps, 1, 2 ** 62 - 1, rule=">= 1")
    n_rows = corr.shape[0] * corr.shape[1] if dims == 3 else corr.shape[0]
    off = uniform_offsets(*corr.shape[:2]) if dims == 3 else check_offsets(what, "offsets", offsets, n_rows, allow_empty=True)
    for x, name in ((corr, "corr"), (src_keypts, "src_keypts"), (tgt_keypts, "tgt_keypts")):
        require_device(x, name, what)
    dev = corr.device
    same_device(what, corr=corr, src_keypts=src_keypts, tgt_keypts=tgt_keypts)
    if isinstance(off, list):
        if max(b - a for a, b in zip(off, off[1:])) > MAX_ROWS:
            raise NotImplementedError(f"gmf_amd.{what}: a pair holds at most {MAX_ROWS} rows "
                                      f"(got {max(b - a for a, b in zip(off, off[1:]))})")
        dev_off, max_n = device_offsets(off, n_rows, dev, what, allow_empty=True, checked=True)
    else:
        dev_off, _ = device_offsets(off, n_rows, dev, what)
        max_n = min(n_rows, MAX_ROWS)                       # the largest pair is not known without a read-back
    B = dev_off.numel() - 1
    Cc = corr.reshape(-1, 6).contiguous()
    S = src_keypts.reshape(-1, 3).contiguous()
    Q = tgt_keypts.reshape(-1, 3).contiguous()
    T = torch.empty((B, 4, 4), device=dev, dtype=torch.float32)
    labels = torch.empty(corr.shape[:-1], device=dev, dtype=torch.float32)
    degree = torch.empty(corr.shape[:-1], device=dev, dtype=torch.int32)
    info = torch.empty((2, B), device=dev, dtype=torch.int32)
    steps = torch.empty(B, device=dev, dtype=torch.int64)
    h, st = handle_and_stream(Cc)
    h.call("gmf_max_clique", Cc.data_ptr(), S.data_ptr(), Q.data_ptr(), dev_off.data_ptr(), B, n_rows, max_n, tau, met, budget,
           labels.data_ptr(), T.data_ptr(), info[0].data_ptr(), info[1].data_ptr(), steps.data_ptr(), degree.data_ptr(), st)
    return (T, labels, info[0], info[1], steps, degree) if return_info else (T, labels)


def PMC(corr, src_keypts, tgt_keypts, args):
    """Drop-in for the reference's PMC (GMF_PointDSC/baseline_scripts/baseline_3DMatch.py:56-77): corr [1,N,6], src_keypts,
    tgt_keypts [1,N,3], `args.inlier_threshold` read -> (pred_trans [1,4,4], pred_labels [1,N]).  The reference's rule on squared
    lengths; one pair per call; the inputs are not written.  Ties and the empty graph: see max_clique_batched."""
    if not isinstance(corr, torch.Tensor) or corr.dim() != 3 or corr.shape[0] != 1:
        fail("PMC", f"corr must be [1,N,6]: one pair per call, as in the reference (got {tuple(getattr(corr, 'shape', ()))})")
    return max_clique_batched(corr, src_keypts, tgt_keypts, args.inlier_threshold)


def compatibility_graph(corr, inlier_threshold, metric="squared"):
    """The graph max_clique_batched searches, for one pair: corr [N,6] float32 on the device -> [N, ceil(N / 64)] int64 bit rows,
    bit j % 64 of word j / 64 of row i = edge (i, j).  No diagonal; the bits past column N - 1 are zero."""
    what = "compatibility_graph"
    check_rows(what, "corr", corr, 2, 6)
    tau, met = _check_common(what, inlier_threshold, metric)
    require_device(corr, "corr", what)
    N = corr.shape[0]
    if N > MAX_ROWS:
        raise NotImplementedError(f"gmf_amd.{what}: a pair holds at most {MAX_ROWS} rows (got {N})")
    bits = torch.empty((N, (N + 63) // 64), device=corr.device, dtype=torch.int64)
    if N == 0:
        return bits
    Cc = corr.contiguous()
    dev_off, _ = device_offsets([0, N], N, corr.device, what, checked=True)
    degree = torch.empty(N, device=corr.device, dtype=torch.int32)
    h, st = handle_and_stream(Cc)
    h.call("gmf_pmc_graph", Cc.data_ptr(), dev_off.data_ptr(), 1, N, N, tau, met, bits.data_ptr(), degree.data_ptr(), st)
    return bits
