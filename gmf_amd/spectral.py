"""The spectral-matching baseline of the reference's evaluation on the device: SM(...) of
GMF_PointDSC/baseline_scripts/baseline_3DMatch.py:19-53 (called with top_ratio = 0.05 at baseline_KITTI.py:51), batched over
ragged pairs and matrix-free.  Kernels: csrc/spectral_kernels.hip; C ABI: gmf_spectral_matching.

The reference forms the dense [N, N] compatibility matrix (100 MB at N = 5000) and multiplies it ten times, one pair at a time.
Here every product recomputes its entries from the seven floats of a column, B pairs share one chain of launches, nothing is read
back and the call can be captured into a graph.  Differences from the reference: INTEGRATION.md, "Spectral-matching baseline"."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._util import handle_and_stream
from .registration import _cached_upload, _device_offsets

_MAX_SPLITS = 32


def _fail(what, msg):
    raise RuntimeError(f"gmf_amd.{what}: {msg}")


def _check_rows(x, name, what, dims, width):
    if not isinstance(x, torch.Tensor):
        _fail(what, f"`{name}` must be a torch tensor")
    if x.dtype != torch.float32:
        _fail(what, f"`{name}` must be float32 (got {x.dtype})")
    if x.dim() != dims or x.shape[-1] != width:
        _fail(what, f"`{name}` must be a [{'B,N' if dims == 3 else 'sum N'},{width}] tensor (got {tuple(x.shape)})")


def _check_offsets(offsets, n_rows, what):
    """Host-side checks of an offset list; a pair may be empty.  A device int32 tensor is checked by _device_offsets."""
    if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
        return offsets
    off = offsets.tolist() if isinstance(offsets, (torch.Tensor, np.ndarray)) else list(offsets)
    try:
        off = [int(o) for o in off]
    except (TypeError, ValueError):
        _fail(what, "offsets must be B + 1 integers")
    if len(off) < 2 or off[0] != 0 or off[-1] != n_rows or any(b < a for a, b in zip(off, off[1:])):
        _fail(what, "offsets must not decrease, start at 0 and end at sum N")
    return off


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
    _check_rows(corr, "corr", what, dims, 6)
    _check_rows(src_keypts, "src_keypts", what, dims, 3)
    _check_rows(tgt_keypts, "tgt_keypts", what, dims, 3)
    if not corr.shape[:-1] == src_keypts.shape[:-1] == tgt_keypts.shape[:-1]:
        _fail(what, f"corr, src_keypts and tgt_keypts must have equal row counts (got {tuple(corr.shape)} / "
                    f"{tuple(src_keypts.shape)} / {tuple(tgt_keypts.shape)})")
    if dims == 3 and corr.shape[0] == 0:
        _fail(what, "the batch must hold at least one pair")
    tau = float(inlier_threshold)
    if not (tau > 0 and np.isfinite(tau)):
        _fail(what, f"inlier_threshold must be finite and > 0 (got {inlier_threshold})")
    ratio = float(top_ratio)
    if not 0 <= ratio <= 1:
        _fail(what, f"top_ratio must be in [0, 1] (got {top_ratio})")
    its = int(num_iterations)
    if its != num_iterations or not 1 <= its <= 1000:
        _fail(what, f"num_iterations must be an integer in 1..1000 (got {num_iterations})")
    forced = 0
    if _col_splits is not None:
        forced = int(_col_splits)
        if forced != _col_splits or not 1 <= forced <= _MAX_SPLITS:
            _fail(what, f"_col_splits must be an integer in 1..{_MAX_SPLITS} (got {_col_splits})")
    n_rows = corr.shape[0] * corr.shape[1] if dims == 3 else corr.shape[0]
    if dims == 3:
        off = list(range(0, n_rows + 1, corr.shape[1])) if corr.shape[1] else [0] * (corr.shape[0] + 1)
    else:
        off = _check_offsets(offsets, n_rows, what)
    for x, name in ((corr, "corr"), (src_keypts, "src_keypts"), (tgt_keypts, "tgt_keypts")):
        if not x.is_cuda:
            _fail(what, f"`{name}` must live on a HIP device (got {x.device}); the HIP path is mandatory, there is no CPU fallback")
    dev = corr.device
    if src_keypts.device != dev or tgt_keypts.device != dev:
        _fail(what, "corr, src_keypts and tgt_keypts must live on the same device")
    if isinstance(off, list):
        dev_off, max_n = _device_offsets(off, n_rows, dev, what, allow_empty=True)
        # k = int(N * top_ratio) per pair, uploaded once per list of sizes and ratio like the offsets themselves
        topk = _cached_upload(tuple(int((b - a) * ratio) for a, b in zip(off, off[1:])), dev)[0]
    else:
        dev_off, _ = _device_offsets(off, n_rows, dev, what)
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
        _fail("SM", f"corr must be [1,N,6]: one pair per call, as in the reference (got {tuple(getattr(corr, 'shape', ()))})")
    return spectral_matching_batched(corr, src_keypts, tgt_keypts, args.inlier_threshold, top_ratio=top_ratio)
