"""PointDSC's correspondence set from descriptors and keypoints, on the device: the body of the
reference's loaders, for B ragged pairs in one chain of five launches.

  nn_match_mutual(Fs, Ft, len_batch)        datasets/ThreeDMatch.py:164-170, KITTI.py:94-101: argmin both ways, mutual flag
  build_correspondences(...)                datasets/ThreeDMatch.py:163-210, KITTI.py:94-129, demo_registration.py:101-107:
                                            the kept pairs in source order, gathered keypoints, labels, centred corr_pos
"""
from __future__ import annotations

import torch

from ._args import c_ints, fail
from ._util import handle_and_stream, require_cuda_f32
from .matching import _batch_offsets


def _check_desc(src_desc, tgt_desc, len_batch, what):
    """Shapes and len_batch, before any device call -> (off0, off1)."""
    for name, F in (("src_desc", src_desc), ("tgt_desc", tgt_desc)):
        if not isinstance(F, torch.Tensor) or F.dim() != 2:
            fail(what, f"`{name}` must be a [rows, d] tensor")
    if src_desc.shape[1] != tgt_desc.shape[1]:
        fail(what, f"src_desc and tgt_desc differ in width ({src_desc.shape[1]} / {tgt_desc.shape[1]})")
    if src_desc.shape[1] > 128:
        fail(what, "descriptor width above 128 has no HIP kernel", NotImplementedError)
    if len_batch is None:
        len_batch = [(src_desc.shape[0], tgt_desc.shape[0])]
    off0, off1 = _batch_offsets(len_batch, src_desc.shape[0], tgt_desc.shape[0], what)
    for b in range(len(off0) - 1):
        if off0[b + 1] > off0[b] and off1[b + 1] == off1[b]:
            fail(what, f"pair {b} has source rows and no target rows")
    return off0, off1


def nn_match_mutual(src_desc, tgt_desc, len_batch=None):
    """PointDSC matching with the mutual-nearest-neighbour flag: (source_idx int64, source_dis float32, mutual bool), each
    [sum Ns].  One pair: src_desc [Ns, d], tgt_desc [Nt, d]; a batch: the packed rows with `len_batch`, B entries (Ns, Nt), as
    in `find_knn_gpu_batch`.  source_idx (local to the pair) and source_dis equal `nn_match` of every pair bit for bit;
    mutual[i] says that row i is the best source row of its own match (target_idx[source_idx[i]] == i).  Every score is formed
    once and folded both ways; equal scores go to the smaller index on both sides.  No host read."""
    what = "nn_match_mutual"
    off0, off1 = _check_desc(src_desc, tgt_desc, len_batch, what)
    F0 = require_cuda_f32(src_desc, "src_desc").contiguous()
    F1 = require_cuda_f32(tgt_desc, "tgt_desc").contiguous()
    n = F0.shape[0]
    idx = torch.empty(n, device=F0.device, dtype=torch.int32)
    dist = torch.empty(n, device=F0.device, dtype=torch.float32)
    mutual = torch.empty(n, device=F0.device, dtype=torch.uint8)
    h, st = handle_and_stream(F0)
    h.call("gmf_nn_match_mutual_batched", F0.data_ptr(), F1.data_ptr(), c_ints(off0), c_ints(off1), len(off0) - 1, F0.shape[1],
           idx.data_ptr(), dist.data_ptr(), mutual.data_ptr(), st)
    return idx.long(), dist, mutual.bool()


def build_correspondences(src_keypts, tgt_keypts, src_desc, tgt_desc, len_batch=None, use_mutual=True, gt_trans=None,
                          inlier_threshold=None, in_dim=6, gather_desc=False):
    """The correspondence set of B ragged pairs, as the reference's loaders build it one pair at a time on the host: descriptor
    matching, the mutual filter (use_mutual; otherwise every source row is kept), the kept pairs in source order with their
    keypoints gathered, `corr_pos` ([src, tgt] minus the pair's means for in_dim 6; src - tgt for in_dim 3) and, with `gt_trans`
    [B, 4, 4] (or [4, 4] for one pair) and `inlier_threshold`, the labels |R x_src + t - x_tgt| < inlier_threshold as float 0 / 1.

    src_keypts [sum Ns, 3], tgt_keypts [sum Nt, 3], src_desc [sum Ns, d], tgt_desc [sum Nt, d] (unit rows), len_batch: B entries
    (Ns, Nt) on the host (None: one pair).  Returns a dict that `PointDSC.forward` takes in its ragged form once "p_tokens" /
    "q_tokens" (or the images) are added: packed "corr_pos" [M, in_dim], "src_keypts" / "tgt_keypts" [M, 3], "n_points" (a host
    list of B counts), "corr" [M, 2] int64 (source row, target row, local to the pair), "offsets" [B + 1] int32 on the device,
    "gt_labels" [M] with gt_trans, "src_desc" / "tgt_desc" [M, d] with gather_desc.  The tensors are views, cut to M rows, of
    buffers sized for sum Ns rows.

    The whole chain runs on the device in five launches whatever B.  There is exactly ONE device-to-host copy, the B + 1
    offsets, because `forward_ragged` needs `n_points` on the host; nothing else is read back.  A pair may come out empty
    (n_points[b] == 0, or fewer than the reference's 10): the counts are returned and the caller decides."""
    what = "build_correspondences"
    off0, off1 = _check_desc(src_desc, tgt_desc, len_batch, what)
    B = len(off0) - 1
    for name, P, n in (("src_keypts", src_keypts, off0[-1]), ("tgt_keypts", tgt_keypts, off1[-1])):
        if not isinstance(P, torch.Tensor) or P.dim() != 2 or tuple(P.shape) != (n, 3):
            fail(what, f"`{name}` must be [{n}, 3], one row per descriptor row")
    if in_dim not in (3, 6):
        raise NotImplementedError(f"gmf_amd.{what}: in_dim {in_dim} is not built (3 and 6 are; the 9, 12 and 70 forms are not what "
                                  "GMF instantiates)")
    if gt_trans is not None:
        if inlier_threshold is None:
            fail(what, "gt_trans needs an inlier_threshold")
        if not (float(inlier_threshold) > 0):
            fail(what, "inlier_threshold must be > 0")
        if not isinstance(gt_trans, torch.Tensor) or tuple(gt_trans.shape) not in ((B, 4, 4),) + (((4, 4),) if B == 1 else ()):
            fail(what, f"gt_trans must be [{B}, 4, 4]")
    F0 = require_cuda_f32(src_desc, "src_desc").contiguous()
    F1 = require_cuda_f32(tgt_desc, "tgt_desc").contiguous()
    P0 = require_cuda_f32(src_keypts, "src_keypts").contiguous()
    P1 = require_cuda_f32(tgt_keypts, "tgt_keypts").contiguous()
    T = require_cuda_f32(gt_trans, "gt_trans").contiguous() if gt_trans is not None else None
    dev, cap, d = F0.device, off0[-1], F0.shape[1]
    offsets = torch.empty(B + 1, device=dev, dtype=torch.int32)
    corr = torch.empty((cap, 2), device=dev, dtype=torch.int64)
    src = torch.empty((cap, 3), device=dev)
    tgt = torch.empty((cap, 3), device=dev)
    pos = torch.empty((cap, in_dim), device=dev)
    sdesc = torch.empty((cap, d), device=dev) if gather_desc else None
    tdesc = torch.empty((cap, d), device=dev) if gather_desc else None
    labels = torch.empty(cap, device=dev) if T is not None else None
    h, st = handle_and_stream(F0)
    h.call("gmf_build_correspondences", F0.data_ptr(), F1.data_ptr(), P0.data_ptr(), P1.data_ptr(), c_ints(off0), c_ints(off1),
           B, d, 1 if use_mutual else 0, in_dim, T.data_ptr() if T is not None else None,
           float(inlier_threshold) if T is not None else 0.0, offsets.data_ptr(), corr.data_ptr(), src.data_ptr(), tgt.data_ptr(),
           pos.data_ptr(), sdesc.data_ptr() if gather_desc else None, tdesc.data_ptr() if gather_desc else None,
           labels.data_ptr() if labels is not None else None, st)
    host = offsets.tolist()                                # the one device-to-host copy
    M = host[-1]
    out = {"corr_pos": pos[:M], "src_keypts": src[:M], "tgt_keypts": tgt[:M], "n_points": [b - a for a, b in zip(host, host[1:])],
           "corr": corr[:M], "offsets": offsets}
    if labels is not None:
        out["gt_labels"] = labels[:M]
    if gather_desc:
        out["src_desc"], out["tgt_desc"] = sdesc[:M], tdesc[:M]
    return out
