"""Descriptor-space nearest-neighbour matching: the step that produces the putative
correspondences on both plugin surfaces.

  nn_match(Fs, Ft)            PointDSC: datasets/ThreeDMatch.py:164-166, demo_registration.py:101-103
  find_knn_gpu(F0, F1, ...)   DGR: core/knn.py:23-74 (knn = 1), distances as core/metrics.py:62-69
  find_knn_gpu_batch, find_knn_batch, find_pairs
                              DGR: core/knn.py:77-140 and core/trainer.py:680-699 for B ragged pairs in three launches
"""
from __future__ import annotations

import torch

from ._args import c_ints, fail
from ._util import handle_and_stream, require_cuda_f32


def _match(F0, F1, mode):
    F0 = require_cuda_f32(F0, "F0").contiguous()
    F1 = require_cuda_f32(F1, "F1").contiguous()
    if F0.dim() != 2 or F1.dim() != 2 or F0.shape[1] != F1.shape[1]:
        fail("matching", f"expected [N0,d] and [N1,d], got {tuple(F0.shape)} / {tuple(F1.shape)}")
    if F0.shape[1] > 128:
        fail("matching", "descriptor width above 128 has no HIP kernel", NotImplementedError)
    idx = torch.empty(F0.shape[0], device=F0.device, dtype=torch.int32)
    dist = torch.empty(F0.shape[0], device=F0.device, dtype=torch.float32)
    h, st = handle_and_stream(F0)
    h.call("gmf_nn_match", F0.data_ptr(), F1.data_ptr(), F0.shape[0], F1.shape[0], F0.shape[1], mode,
           idx.data_ptr(), dist.data_ptr(), st)
    return idx.long(), dist


def nn_match(src_desc, tgt_desc):
    """PointDSC matching for unit descriptors: (source_idx [Ns], source_dis [Ns]) with
    distance = sqrt(2 - 2 <s,t> + 1e-6) and argmin over the target rows."""
    return _match(src_desc, tgt_desc, 0)


def find_knn_gpu(F0, F1, nn_max_n=-1, knn=1, return_distance=False):
    """DGR find_knn_gpu.  `nn_max_n` only selects the reference's distance convention (L2 when chunked, squared L2
    otherwise); no chunking is needed here because the N0 x N1 matrix is never materialised."""
    if knn != 1:
        fail("find_knn_gpu", "GMF-DGR only uses knn = 1 (deep_global_registration.py:300)", NotImplementedError)
    idx, dist = _match(F0, F1, 1 if nn_max_n > 1 else 2)
    if nn_max_n > 1:
        idx = idx[:, None]          # the reference concatenates [rows, knn] blocks (knn.py:40-41,62-63)
    return (idx, dist[:, None]) if return_distance else idx


def _batch_offsets(len_batch, n0, n1, what):
    """len_batch, B entries (N0, N1) -> the two host offset lists of B + 1 entries; checked against the row counts."""
    try:
        lens = [(int(a), int(b)) for a, b in len_batch]
    except (TypeError, ValueError):
        fail(what, "len_batch must be a sequence of (N0, N1) pairs")
    if not lens:
        fail(what, "len_batch is empty")
    if any(a < 0 or b < 0 for a, b in lens):
        fail(what, "len_batch holds a negative size")
    off0, off1 = [0], [0]
    for a, b in lens:
        off0.append(off0[-1] + a)
        off1.append(off1[-1] + b)
    if off0[-1] != n0 or off1[-1] != n1:
        fail(what, f"len_batch sums to ({off0[-1]}, {off1[-1]}) rows, F0 / F1 have ({n0}, {n1})")
    return off0, off1


def _match_batched(F0, F1, len_batch, mode, global_index, what):
    """-> (idx [sum N0] int64, dist [sum N0] float32, off0, off1) of gmf_nn_match_batched."""
    for name, F in (("F0", F0), ("F1", F1)):
        if not isinstance(F, torch.Tensor) or F.dim() != 2:
            fail(what, f"`{name}` must be a [rows, d] tensor")
    if F0.shape[1] != F1.shape[1]:
        fail(what, f"F0 and F1 differ in width ({F0.shape[1]} / {F1.shape[1]})")
    if F0.shape[1] > 128:
        fail(what, "descriptor width above 128 has no HIP kernel", NotImplementedError)
    off0, off1 = _batch_offsets(len_batch, F0.shape[0], F1.shape[0], what)
    F0 = require_cuda_f32(F0, "F0").contiguous()
    F1 = require_cuda_f32(F1, "F1").contiguous()
    B = len(off0) - 1
    idx = torch.empty(F0.shape[0], device=F0.device, dtype=torch.int32)
    dist = torch.empty(F0.shape[0], device=F0.device, dtype=torch.float32)
    h, st = handle_and_stream(F0)
    h.call("gmf_nn_match_batched", F0.data_ptr(), F1.data_ptr(), c_ints(off0), c_ints(off1),
           B, F0.shape[1], mode, 1 if global_index else 0, idx.data_ptr(), dist.data_ptr(), st)
    return idx, dist, off0, off1


def find_knn_gpu_batch(F0, F1, len_batch, nn_max_n=-1, knn=1, return_distance=False, concat_results=False):
    """DGR find_knn_gpu_batch (core/knn.py:106-140): `find_knn_gpu` of every pair of a collated batch, in three launches for the
    whole batch.  F0 [sum N0, d], F1 [sum N1, d]; len_batch: B entries (N0, N1) on the host.  Returns a list with one entry per
    pair, shaped as `find_knn_gpu` returns it ([N0], or [N0, 1] when nn_max_n > 1; distances [N0, 1]), or, with concat_results,
    one tensor whose indices are rows of F1.  Indices and distances equal those of B `find_knn_gpu` calls on the slices bit for
    bit.  A pair without source rows gives an empty entry; one with source rows and no target rows raises RuntimeError."""
    what = "find_knn_gpu_batch"
    if knn != 1:
        fail(what, "GMF-DGR only uses knn = 1 (deep_global_registration.py:300)", NotImplementedError)
    chunked = nn_max_n > 1
    idx32, dist, off0, _ = _match_batched(F0, F1, len_batch, 1 if chunked else 2, concat_results, what)
    idx = idx32.long()
    if chunked:
        idx = idx[:, None]
    dist = dist[:, None]
    if concat_results:
        return (idx, dist) if return_distance else idx
    nns = [idx[a:b] for a, b in zip(off0, off0[1:])]
    if return_distance:
        return nns, [dist[a:b] for a, b in zip(off0, off0[1:])]
    return nns


def find_knn_batch(F0, F1, len_batch, return_distance=False, nn_max_n=-1, knn=1, search_method=None, concat_results=False):
    """DGR find_knn_batch (core/knn.py:77-103).  search_method None or 'gpu' is `find_knn_gpu_batch`; 'cpu' (the reference's
    cKDTree search) raises NotImplementedError - nothing falls back to the host; anything else raises ValueError."""
    if search_method is None or search_method == "gpu":
        return find_knn_gpu_batch(F0, F1, len_batch, nn_max_n=nn_max_n, knn=knn, return_distance=return_distance,
                                  concat_results=concat_results)
    if search_method == "cpu":
        fail("find_knn_batch", "the 'cpu' search method is not built; there is no CPU fallback", NotImplementedError)
    raise ValueError(f"Search method {search_method} not defined")


def find_pairs(F0, F1, len_batch, nn_max_n=-1, knn=1):
    """WeightedProcrustesTrainer.find_pairs (core/trainer.py:680-699): per pair the [N0, 2] int64 device tensor of (source row,
    nearest target row), both local to the pair.  (The reference returns them on the CPU.)"""
    what = "find_pairs"
    if knn != 1:
        fail(what, "GMF-DGR only uses knn = 1 (deep_global_registration.py:300)", NotImplementedError)
    idx32, _, off0, _ = _match_batched(F0, F1, len_batch, 1 if nn_max_n > 1 else 2, False, what)
    rows = torch.arange(idx32.shape[0], device=idx32.device)
    starts = torch.repeat_interleave(torch.tensor(off0[:-1], device=idx32.device),
                                     torch.tensor([b - a for a, b in zip(off0, off0[1:])], device=idx32.device),
                                     output_size=idx32.shape[0])
    pairs = torch.stack([rows - starts, idx32.long()], 1)
    return [pairs[a:b] for a, b in zip(off0, off0[1:])]
