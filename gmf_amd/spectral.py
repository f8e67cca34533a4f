"""The spectral-matching baseline of the reference's evaluation on the device: SM(...) of
GMF_PointDSC/baseline_scripts/baseline_3DMatch.py:19-53 (called with top_ratio = 0.05 at baseline_KITTI.py:51), batched over
ragged pairs and matrix-free.  Kernels: csrc/spectral_kernels.hip; C ABI: gmf_spectral_matching.

The reference forms the dense [N, N] compatibility matrix (100 MB at N = 5000) and multiplies it ten times, one pair at a time.
Here every product recomputes its entries from the seven floats of a column, B pairs share one chain of launches, nothing is read
back and the call can be captured into a graph.  Differences from the reference: INTEGRATION.md, "Spectral-matching baseline"."""
from __future__ import annotations

import ctypes as C

import torch

from ._args import (cached_upload, check_offsets, check_rows, device_offsets, fail, int_in_range, positive_finite, require_device,
                    same_device, uniform_offsets)
from ._util import handle_and_stream

_MAX_SPLITS = 32


def spectral_matching_batched(corr, src_keypts, tgt_keypts, inlier_threshold, top_ratio=0.1, num_iterations=10, offsets=None,
                              return_eigenvector=False, _col_splits=None):
    """Spectral matching over B pairs (the reference's SM, batched).

    corr [B,N,6], src_keypts, tgt_keypts [B,N,3] float32 (offsets None), or packed [sum N, .] with `offsets` (B + 1 ints, or
    an int32 device tensor; a pair may be empty).  Per pair of N rows, in fp32:
      d_ij = |c_i[0:3] - c_j[0:3]| - |c_i[3:6] - c_j[3:6]|, m_ij = max(0, 4.5 - d_ij^2 / (2 sigma^2)) with
      sigma = inlier_threshold / 3, and m_ii = 0;
      v = ones, `num_iterations` times v <- M v, v <- v / (|v| + 1e-6);
      labels = 1 on the k = int(N * top_ratio) rows of largest v.  Equal values go to the smaller row: the reference's
      `argsort` leaves the order of ties open, so on exact ties its labels are one of several valid answers and this is another;
      T = rigid_transform_3d(src_keypts, tgt_keypts, v * labels): weights not normalised, centroids over sum w + 1e-6,
      R = V diag(1, 1, det) U^T.  k = 0, an all-zero v or an empty pair give the identity.
    A pair returns the same bits alone, in any batch and on every run.

    Returns trans [B,4,4] and labels (float 0 / 1, [B,N] or [sum N]); with return_eigenvector also v in labels' shape.
    No host synchronisation; the call can be captured into a graph."""
    what = "spectral_matching_batched"
    dims = 3 if offsets is None else 2
    check_rows(what, "corr", corr, dims, 6)
    check_rows(what, "src_keypts", src_keypts, dims, 3)
    check_rows(what, "tgt_keypts", tgt_keypts, dims, 3)
    if not corr.shape[:-1] == src_keypts.shape[:-1] == tgt_keypts.shape[:-1]:
        fail(what, f"corr, src_keypts and tgt_keypts must have equal row counts (got {tuple(corr.shape)} / "
                   f"{tuple(src_keypts.shape)} / {tuple(tgt_keypts.shape)})")
    if dims == 3 and corr.shape[0] == 0:
        fail(what, "the batch must hold at least one pair")
    tau = positive_finite(what, "inlier_threshold", inlier_threshold)
    ratio = float(top_ratio)
    if not 0 <= ratio <= 1:
        fail(what, f"top_ratio must be in [0, 1] (got {top_ratio})")
    its = int_in_range(what, "num_iterations", num_iterations, 1, 1000)
    forced = 0 if _col_splits is None else int_in_range(what, "_col_splits", _col_splits, 1, _MAX_SPLITS)
    n_rows = corr.shape[0] * corr.shape[1] if dims == 3 else corr.shape[0]
    off = uniform_offsets(*corr.shape[:2]) if dims == 3 else check_offsets(what, "offsets", offsets, n_rows, allow_empty=True)
    for x, name in ((corr, "corr"), (src_keypts, "src_keypts"), (tgt_keypts, "tgt_keypts")):
        require_device(x, name, what)
    dev = corr.device
    same_device(what, corr=corr, src_keypts=src_keypts, tgt_keypts=tgt_keypts)
    if isinstance(off, list):
        dev_off, max_n = device_offsets(off, n_rows, dev, what, allow_empty=True, checked=True)
        # k = int(N * top_ratio) per pair, uploaded once per list of sizes and ratio like the offsets themselves
        topk = cached_upload(tuple(int((b - a) * ratio) for a, b in zip(off, off[1:])), dev)[0]
    else:
        dev_off, _ = device_offsets(off, n_rows, dev, what)
        max_n = n_rows                                      # the largest pair is not known without a read-back
        topk = ((dev_off[1:] - dev_off[:-1]).double() * ratio).floor().to(torch.int32)      # int(N * top_ratio), Python's arithmetic
    B = dev_off.numel() - 1
    Cc = corr.reshape(-1, 6).contiguous()
    S = src_keypts.reshape(-1, 3).contiguous()
    Q = tgt_keypts.reshape(-1, 3).contiguous()
    T = torch.empty((B, 4, 4), device=dev, dtype=torch.float32)
    eig = torch.empty(corr.shape[:-1], device=dev, dtype=torch.float32)
    labels = torch.empty(corr.shape[:-1], device=dev, dtype=torch.float32)
    h, st = handle_and_stream(Cc)
    args = (Cc.data_ptr(), S.data_ptr(), Q.data_ptr(), dev_off.data_ptr(), B, max_n, tau, topk.data_ptr(), its, eig.data_ptr(),
            labels.data_ptr(), T.data_ptr(), st)
    if forced:
        # test-only: the knob belongs to the handle, and the three calls do not hold its lock together, so another thread on the
        # same handle would run with the forced count meanwhile
        cur = C.c_int(0)
        h.call("gmf_get_tuning", b"spectral_col_splits", C.byref(cur))
        h.call("gmf_set_tuning", b"spectral_col_splits", forced)
        try:
            h.call("gmf_spectral_matching", *args)
        finally:
            h.call("gmf_set_tuning", b"spectral_col_splits", cur.value)
    else:
        h.call("gmf_spectral_matching", *args)
    return (T, labels, eig) if return_eigenvector else (T, labels)


def SM(corr, src_keypts, tgt_keypts, args, top_ratio=0.1):
    """Drop-in for the reference's SM (GMF_PointDSC/baseline_scripts/baseline_3DMatch.py:19-53): corr [1,N,6], src_keypts,
    tgt_keypts [1,N,3], `args.inlier_threshold` read -> (pred_trans [1,4,4], pred_labels [1,N]).  One pair per call, as the
    reference's label assignment implies; the inputs are not written.  Ties: see spectral_matching_batched."""
    if not isinstance(corr, torch.Tensor) or corr.dim() != 3 or corr.shape[0] != 1:
        fail("SM", f"corr must be [1,N,6]: one pair per call, as in the reference (got {tuple(getattr(corr, 'shape', ()))})")
    return spectral_matching_batched(corr, src_keypts, tgt_keypts, args.inlier_threshold, top_ratio=top_ratio)
