"""Correspondence RANSAC, feature-matching RANSAC and point-to-point, point-to-plane and coloured ICP on the device: the solvers the reference's evaluation scripts run after the network
through open3d 0.9 / 0.10 on the CPU (GMF_PointDSC/evaluation/test_3DMatch.py:76-96, benchmark_utils.py:40-56;
GMF_DeepGlobalRegistration/*/core/deep_global_registration.py:26-85, 256-276, 385-405).  Kernels: csrc/solver_kernels.hip.

The batched forms take one stream, make no host synchronisation and can be captured into a graph.  The open3d-shaped wrappers
read back once to size their correspondence set (and the RANSAC wrapper once more to check the indices of `corres`).
Differences from open3d: INTEGRATION.md, "Evaluation solvers"."""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _lib
from ._args import (check_offsets, check_rows, device_offsets, fail, int_in_range, positive_finite, require_device, same_device,
                    uniform_offsets, unit_interval)
from ._util import handle_and_stream
from .features import color_gradients_batched, color_intensity

RegistrationResult = collections.namedtuple("RegistrationResult", "transformation correspondence_set fitness inlier_rmse")

_MAX_HYPOTHESES = 1 << 24
_MAX_VALIDATION = 1 << 16
_ICP_SEARCH = {"brute": 0, "grid": 1}
_ICP_ESTIMATION = ("point_to_point", "point_to_plane")
ICP_PLANE_ROWS = 512          # csrc/icp_plane_plan.hpp kIcpPlaneRows: the source rows of one partial sum of the point-to-plane step


def ransac_correspondence_batched(src, tgt, max_correspondence_distance, offsets=None, mask=None, ransac_n=3,
                                  num_hypotheses=1000, seed=0, first_pair=0):
    """Correspondence RANSAC over B pairs: row i of `src` corresponds to row i of `tgt`.

    src, tgt: [B,N,3] float32 (offsets None) or ragged [sum N,3] with `offsets` (B + 1 ints, or an int32 device tensor).
    mask: optional bool tensor of src's leading shape; only its rows take part (PointDSC: pred_labels > 0).
    Hypothesis h of pair b draws `ransac_n` distinct participating rows with the counter-based sampler of
    csrc/ransac_sampler.hpp (pair index first_pair + b, so a batch split into calls gives the same results), fits them with the
    fp64 Kabsch and counts the rows with |R s + t - q|^2 < tau^2.  The winner has the most inliers, then the smaller sum of their
    d^2, then the smaller h; its T is returned without a final refit.

    Returns T [B,4,4] f32, inliers (bool, src's leading shape), fitness [B] (inliers / participating rows), inlier_rmse [B],
    hypothesis [B] int64 (-1 if the pair had fewer than ransac_n rows: T = identity) and sample [B, ransac_n] int64 (the winner's
    rows, numbered within the pair)."""
    what = "ransac_correspondence_batched"
    dims = 3 if offsets is None else 2
    check_rows(what, "src", src, dims, 3, non_empty=True)
    check_rows(what, "tgt", tgt, dims, 3, non_empty=True)
    if src.shape != tgt.shape:
        fail(what, f"src and tgt must have the same shape (got {tuple(src.shape)} / {tuple(tgt.shape)})")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.shape != src.shape[:-1]:
            fail(what, f"mask must be a bool tensor of shape {tuple(src.shape[:-1])}")
    n = int_in_range(what, "ransac_n", ransac_n, 3, 8)
    H = int_in_range(what, "num_hypotheses", num_hypotheses, 1, _MAX_HYPOTHESES, rule="in 1..2**24")
    tau = positive_finite(what, "max_correspondence_distance", max_correspondence_distance, rule="> 0")
    if int(first_pair) < 0:
        fail(what, "first_pair must be >= 0")
    n_rows = src.shape[0] * src.shape[1] if dims == 3 else src.shape[0]
    off = uniform_offsets(*src.shape[:2]) if dims == 3 else check_offsets(what, "offsets", offsets, n_rows)
    require_device(src, "src", what)
    require_device(tgt, "tgt", what)
    same_device(what, src=src, tgt=tgt, mask=mask)
    dev_off, max_rows = device_offsets(off, n_rows, src.device, what, checked=True)
    B = dev_off.numel() - 1
    S = src.reshape(-1, 3).contiguous()
    Q = tgt.reshape(-1, 3).contiguous()
    m = None if mask is None else mask.reshape(-1).contiguous()
    dev = src.device
    T = torch.empty((B, 4, 4), device=dev, dtype=torch.float32)
    inliers = torch.empty(src.shape[:-1], device=dev, dtype=torch.bool)
    stats = torch.empty((2, B), device=dev, dtype=torch.float32)
    ids = torch.empty((B, 1 + n), device=dev, dtype=torch.int64)
    h, st = handle_and_stream(S)
    h.call("gmf_ransac_correspondence", S.data_ptr(), Q.data_ptr(), dev_off.data_ptr(), None if m is None else m.data_ptr(), B,
           n_rows, max_rows, n, H, tau, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_pair), T.data_ptr(),
           inliers.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), ids.data_ptr(), ids.data_ptr() + 8 * B, st)
    # ids holds hypothesis [B] followed by sample [B, n] (one allocation)
    flat = ids.view(-1)
    return T, inliers, stats[0], stats[1], flat[:B], flat[B:].view(B, n)


def icp_point_to_point_batched(source, target, init, max_correspondence_distance, source_offsets=None, target_offsets=None,
                               max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, search="brute"):
    """Point-to-point ICP over B pairs (open3d's registration_icp loop).

    source [B,Ns,3] / ragged [sum Ns,3] with `source_offsets`, target [B,Nt,3] / ragged with its own `target_offsets`,
    init [B,4,4] float32.  C = the exact nearest target row of each transformed source row, kept when d^2 < tau^2.  The loop
    evaluates C at init, then up to `max_iteration` times: dT = Umeyama over C, T <- dT T (fp64), the ORIGINAL source
    transformed by T, C again; it stops when |d fitness| < relative_fitness and |d rmse| < relative_rmse.  Decided on the device.
    search: "brute" tests every target of the pair per pass; "grid" builds a hashed grid of cell edge tau over the targets once
    and tests the 27 cells around each transformed source row.  Both return the same bits ("Evaluation solvers").

    Returns T [B,4,4] f32, fitness [B] (|C| / Ns), inlier_rmse [B], iterations [B] int32 (loop passes run) and nn (int64,
    source's leading shape: the matched target row within the pair, -1 outside C)."""
    return _icp_batched("icp_point_to_point_batched", source, target, None, init, max_correspondence_distance, source_offsets,
                        target_offsets, max_iteration, relative_fitness, relative_rmse, search)


def icp_point_to_plane_batched(source, target, target_normals, init, max_correspondence_distance, source_offsets=None,
                               target_offsets=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, search="brute"):
    """Point-to-plane ICP over B pairs (open3d 0.9's registration_icp with TransformationEstimationPointToPlane).

    The arguments of `icp_point_to_point_batched` and target_normals: float32 of target's shape, one normal per target row, used
    as given (not renormalised; negating any of them changes no output bit).  C, nn, fitness, inlier_rmse (Euclidean), the loop
    and the stopping rule are the point-to-point form's; only the update differs.  Over the rows of C whose normal is finite,
    with p the transformed source row, q its target and n the normal: r = (p - q) . n, J = [p x n ; n], A = sum J J^T,
    b = sum J r in fp64; A x = -b by LDL^T without pivoting, where a pivot d_k is accepted when it is finite and
    d_k > 2^-40 A_kk; T <- [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)] T (fp64).  A rejected pivot or an empty C leaves T alone for
    that pass.  The sums are taken per ICP_PLANE_ROWS source rows of a pair in a fixed tree: a pair's bits do not depend on
    the batch or on the search.  tests/icp_plane_reference.py restates all of it in float64.

    Returns T [B,4,4] f32, fitness [B], inlier_rmse [B], iterations [B] int32 and nn (int64, source's leading shape), as the
    point-to-point form does.  No host synchronisation; the call can be captured into a graph."""
    return _icp_batched("icp_point_to_plane_batched", source, target, target_normals, init, max_correspondence_distance,
                        source_offsets, target_offsets, max_iteration, relative_fitness, relative_rmse, search, plane=True)


def icp_colored_batched(source, target, source_colors, target_colors, target_normals, init, max_correspondence_distance,
                        source_offsets=None, target_offsets=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                        search="brute", lambda_geometric=0.968, target_gradients=None):
    """Coloured ICP over B pairs (open3d 0.9's registration_colored_icp; Park, Zhou, Koltun, ICCV 2017).

    The arguments of `icp_point_to_plane_batched`, and: source_colors and target_colors, float32 of the points' shape (colours in
    0..1, reduced to the intensity fp32(((r + g) + b) / 3) evaluated in fp64) or of their leading shape (the intensity itself);
    lambda_geometric in [0, 1]; target_gradients, float32 of target's shape: the targets' colour gradients, by default
    `color_gradients_batched` of every pair's target with radius 2 x max_correspondence_distance and 30 neighbours (open3d's
    choice).  C, nn, fitness, inlier_rmse (Euclidean), the loop, the stopping rule, the solve and the sum tree are the
    point-to-plane form's; the sums run over the rows of C whose normal, gradient and two intensities are finite.  With p the
    transformed source row, q its target, n and g the target's normal and gradient, I_s and I_t the intensities, in fp64:
    r_G = (p - q) . n, J_G = [p x n ; n], u = (p - q) - r_G n, r_I = I_s - (g . u + I_t), m = -(g - (g . n) n),
    J_I = [p x m ; m]; A = sum lambda J_G J_G^T + (1 - lambda) J_I J_I^T, b = sum lambda J_G r_G + (1 - lambda) J_I r_I.
    Negating normals changes no output bit; a pair's bits do not depend on the batch or on the search.
    tests/colored_icp_reference.py restates all of it in float64.

    Returns T [B,4,4] f32, fitness [B], inlier_rmse [B], iterations [B] int32 and nn (int64, source's leading shape), as the
    other two forms do.  No host synchronisation; the call can be captured into a graph."""
    return _icp_batched("icp_colored_batched", source, target, target_normals, init, max_correspondence_distance, source_offsets,
                        target_offsets, max_iteration, relative_fitness, relative_rmse, search, plane=True,
                        color=(source_colors, target_colors, lambda_geometric, target_gradients))


def _icp_batched(what, source, target, normals, init, max_correspondence_distance, source_offsets, target_offsets, max_iteration,
                 relative_fitness, relative_rmse, search, plane=False, color=None):
    """The argument checks, the outputs and the call of the three ICP forms (plane: target normals and gmf_icp_point_to_plane;
    color, with plane: (source_colors, target_colors, lambda_geometric, target_gradients) and gmf_icp_colored)."""
    if not isinstance(search, str) or search not in _ICP_SEARCH:
        fail(what, f'search must be "brute" or "grid" (got {search!r})')
    if (source_offsets is None) != (target_offsets is None):
        fail(what, "give both source_offsets and target_offsets, or neither")
    dims = 3 if source_offsets is None else 2
    check_rows(what, "source", source, dims, 3, non_empty=True)
    check_rows(what, "target", target, dims, 3, non_empty=True)
    if dims == 3 and source.shape[0] != target.shape[0]:
        fail(what, f"source and target must hold the same number of pairs (got {source.shape[0]} / {target.shape[0]})")
    if plane:
        if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or normals.shape != target.shape:
            fail(what, f"target_normals must be a float32 tensor of target's shape {tuple(target.shape)}, one normal per target row")
        if normals.device != target.device:
            fail(what, f"target_normals must live on target's device ({target.device}; got {normals.device})")
    if not isinstance(init, torch.Tensor) or init.dtype != torch.float32 or init.dim() != 3 or init.shape[1:] != (4, 4):
        fail(what, "init must be a float32 [B,4,4] tensor")
    tau = positive_finite(what, "max_correspondence_distance", max_correspondence_distance, rule="> 0")
    it = int_in_range(what, "max_iteration", max_iteration, 0, 100000)
    rf, rr = float(relative_fitness), float(relative_rmse)
    if not (rf >= 0 and rr >= 0):
        fail(what, "relative_fitness and relative_rmse must be >= 0")
    ns_rows = source.shape[0] * source.shape[1] if dims == 3 else source.shape[0]
    nt_rows = target.shape[0] * target.shape[1] if dims == 3 else target.shape[0]
    if dims == 3:
        soff, toff = uniform_offsets(*source.shape[:2]), uniform_offsets(*target.shape[:2])
    else:
        soff = check_offsets(what, "source_offsets", source_offsets, ns_rows)
        toff = check_offsets(what, "target_offsets", target_offsets, nt_rows)
        if isinstance(soff, list) and isinstance(toff, list) and len(soff) != len(toff):
            fail(what, "source_offsets and target_offsets must describe the same number of pairs")
    if color is not None:
        Is = color_intensity(what, "source_colors", color[0], source.shape[:-1])
        It = color_intensity(what, "target_colors", color[1], target.shape[:-1])
        lam = unit_interval(what, "lambda_geometric", color[2])
        G = color[3]
        if G is not None and (not isinstance(G, torch.Tensor) or G.dtype != torch.float32 or G.shape != target.shape):
            fail(what, f"target_gradients must be None or a float32 tensor of target's shape {tuple(target.shape)}, one gradient "
                       "per target row")
    for x, name in ((source, "source"), (target, "target"), (init, "init")):
        require_device(x, name, what)
    same_device(what, source=source, target=target, init=init)
    if color is not None:
        same_device(what, source=source, source_colors=Is, target_colors=It, target_gradients=G)
    dev = source.device
    dso, max_s = device_offsets(soff, ns_rows, dev, what, checked=True)
    dto, max_t = device_offsets(toff, nt_rows, dev, what, checked=True)
    B = dso.numel() - 1
    if dto.numel() != B + 1:
        fail(what, "source_offsets and target_offsets must describe the same number of pairs")
    if init.shape[0] != B:
        fail(what, f"init must hold one [4,4] transformation per pair ({B}; got {init.shape[0]})")
    S = source.reshape(-1, 3).contiguous()
    Q = target.reshape(-1, 3).contiguous()
    T0 = init.contiguous()
    T = torch.empty((B, 4, 4), device=dev, dtype=torch.float32)
    stats = torch.empty((2, B), device=dev, dtype=torch.float32)
    iters = torch.empty(B, device=dev, dtype=torch.int32)
    nn = torch.empty(source.shape[:-1], device=dev, dtype=torch.int64)
    h, st = handle_and_stream(S)
    args = (S.data_ptr(), dso.data_ptr(), Q.data_ptr(), dto.data_ptr(), B, ns_rows, max_s, max_t, T0.data_ptr(), tau, it, rf, rr,
            T.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), iters.data_ptr(), nn.data_ptr())
    if color is not None:
        Nn = normals.reshape(-1, 3).contiguous()
        if G is None:
            G = color_gradients_batched(Q, Nn, It, dto, 2.0 * tau, 30)
        h.call("gmf_icp_colored", *args[:3], Nn.data_ptr(), *args[3:], nt_rows, _ICP_SEARCH[search], Is.data_ptr(), It.data_ptr(),
               G.reshape(-1, 3).contiguous().data_ptr(), lam, st)
    elif plane:
        Nn = normals.reshape(-1, 3).contiguous()
        h.call("gmf_icp_point_to_plane", *args[:3], Nn.data_ptr(), *args[3:], nt_rows, _ICP_SEARCH[search], st)
    elif search == "brute":
        h.call("gmf_icp_point_to_point", *args, st)
    else:
        h.call("gmf_icp_point_to_point_ex", *args, nt_rows, _ICP_SEARCH[search], st)
    return T, stats[0], stats[1], iters, nn


def ransac_feature_matching_batched(source, target, nn, max_correspondence_distance, source_offsets=None, target_offsets=None,
                                    ransac_n=4, max_iteration=100000, max_validation=1000, checker_distance=None,
                                    edge_length_threshold=None, seed=0, first_pair=0, search="grid", return_hypotheses=False):
    """Feature-matching RANSAC over B pairs (open3d's registration_ransac_based_on_feature_matching loop, point-to-point
    estimate without scaling, one similar feature per row).

    source [B,Ns,3] / ragged [sum Ns,3] with `source_offsets`, target [B,Nt,3] / ragged with its own `target_offsets` (a pair
    may have no targets), nn (integer tensor of source's leading shape): the feature-space nearest target row of every source
    row, numbered within the pair (`find_knn_gpu`'s result).
    Hypothesis h in 0 .. max_iteration - 1 of pair first_pair + b draws `ransac_n` distinct source rows with the sampler of
    csrc/ransac_sampler.hpp over the pair's Ns rows and pairs row i with target nn[i].  It passes when every nn lies inside the
    pair's targets, when (edge_length_threshold = r given) every two sampled pairs have |s_i - s_j|^2 >= r^2 |q_i - q_j|^2 and
    the reverse, when the fp64 Kabsch fit succeeds, and when (checker_distance given) every sampled pair has
    |R s + t - q|^2 <= checker_distance^2 under the fit rounded to fp32.  The first `max_validation` passing h in increasing
    order are evaluated on the whole clouds (open3d's sequential rule, independent of the order of execution): C = the source
    rows whose exact nearest target has d^2 < tau^2.  The winner has the largest |C| (at least one row), then the smaller sum of
    d^2 over C (fixed point), then the smaller h; its T is returned without a refit.
    search: "grid" looks for the nearest target in the 27 cells of a hashed grid of cell edge tau around the transformed row,
    "brute" tests every target of the pair; both return the same bits ("Evaluation solvers").

    Returns T [B,4,4] f32, fitness [B] (|C| / Ns), inlier_rmse [B], hypothesis [B] int64 (-1: no winner; then T = identity and
    fitness = inlier_rmse = 0), sample [B, ransac_n] int64 (the winner's source rows within the pair), nn_out (int64, source's
    leading shape: the geometric nearest target row within the pair under T, -1 outside C) and validated [B] int32 (hypotheses
    evaluated).  With return_hypotheses also hyp [B, max_validation] int32 (the evaluated h in order, -1 padded) and their raw
    scores count [B, max_validation] int32 and sum [B, max_validation] int64 (d^2 in units of tau^2 / 2^24).
    No host synchronisation; the call can be captured into a graph."""
    what = "ransac_feature_matching_batched"
    if not isinstance(search, str) or search not in _ICP_SEARCH:
        fail(what, f'search must be "brute" or "grid" (got {search!r})')
    if (source_offsets is None) != (target_offsets is None):
        fail(what, "give both source_offsets and target_offsets, or neither")
    dims = 3 if source_offsets is None else 2
    check_rows(what, "source", source, dims, 3, non_empty=True)
    check_rows(what, "target", target, dims, 3, non_empty=True)
    if dims == 3 and source.shape[0] != target.shape[0]:
        fail(what, f"source and target must hold the same number of pairs (got {source.shape[0]} / {target.shape[0]})")
    if not isinstance(nn, torch.Tensor) or nn.dtype not in (torch.int64, torch.int32) or nn.shape != source.shape[:-1]:
        fail(what, f"nn must be an int64 or int32 tensor of shape {tuple(source.shape[:-1])}")
    n = int_in_range(what, "ransac_n", ransac_n, 3, 8)
    H = int_in_range(what, "max_iteration", max_iteration, 1, _MAX_HYPOTHESES, rule="in 1..2**24")
    V = int_in_range(what, "max_validation", max_validation, 1, _MAX_VALIDATION)
    tau = positive_finite(what, "max_correspondence_distance", max_correspondence_distance, rule="> 0")
    cd = -1.0
    if checker_distance is not None:
        cd = float(checker_distance)
        if not (cd >= 0 and np.isfinite(cd)):
            fail(what, f"checker_distance must be >= 0 or None (got {checker_distance})")
    el = 0.0
    if edge_length_threshold is not None:
        el = float(edge_length_threshold)
        if not 0 < el <= 1:
            fail(what, f"edge_length_threshold must be in (0, 1] or None (got {edge_length_threshold})")
    if int(first_pair) < 0:
        fail(what, "first_pair must be >= 0")
    ns_rows = source.shape[0] * source.shape[1] if dims == 3 else source.shape[0]
    nt_rows = target.shape[0] * target.shape[1] if dims == 3 else target.shape[0]
    if dims == 3:
        soff, toff = uniform_offsets(*source.shape[:2]), uniform_offsets(*target.shape[:2])
    else:
        soff = check_offsets(what, "source_offsets", source_offsets, ns_rows)
        toff = check_offsets(what, "target_offsets", target_offsets, nt_rows, allow_empty=True)
        if isinstance(soff, list) and isinstance(toff, list) and len(soff) != len(toff):
            fail(what, "source_offsets and target_offsets must describe the same number of pairs")
    for x, name in ((source, "source"), (target, "target"), (nn, "nn")):
        require_device(x, name, what)
    same_device(what, source=source, target=target, nn=nn)
    dev = source.device
    dso, max_s = device_offsets(soff, ns_rows, dev, what, checked=True)
    dto, _ = device_offsets(toff, nt_rows, dev, what, allow_empty=True, checked=True)
    B = dso.numel() - 1
    if dto.numel() != B + 1:
        fail(what, "source_offsets and target_offsets must describe the same number of pairs")
    S = source.reshape(-1, 3).contiguous()
    Q = target.reshape(-1, 3).contiguous()
    J = nn.reshape(-1).to(torch.int64).contiguous()
    T = torch.empty((B, 4, 4), device=dev, dtype=torch.float32)
    stats = torch.empty((2, B), device=dev, dtype=torch.float32)
    ids = torch.empty((B, 1 + n), device=dev, dtype=torch.int64)
    nn_out = torch.empty(source.shape[:-1], device=dev, dtype=torch.int64)
    validated = torch.empty(B, device=dev, dtype=torch.int32)
    hyp = count = total = None
    if return_hypotheses:
        hyp = torch.empty((B, V), device=dev, dtype=torch.int32)
        count = torch.empty((B, V), device=dev, dtype=torch.int32)
        total = torch.empty((B, V), device=dev, dtype=torch.int64)
    h, st = handle_and_stream(S)
    h.call("gmf_ransac_feature_matching", S.data_ptr(), dso.data_ptr(), Q.data_ptr(), dto.data_ptr(), J.data_ptr(), B, ns_rows,
           nt_rows, max_s, n, H, V, tau, cd, el, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_pair),
           _ICP_SEARCH[search], T.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), ids.data_ptr(), ids.data_ptr() + 8 * B,
           nn_out.data_ptr(), validated.data_ptr(), _lib.ptr(hyp), _lib.ptr(count), _lib.ptr(total), st)
    flat = ids.view(-1)                                      # hypothesis [B] followed by sample [B, n] (one allocation)
    out = (T, stats[0], stats[1], flat[:B], flat[B:].view(B, n), nn_out, validated)
    return out + (hyp, count, total) if return_hypotheses else out


def _on_device(x, dev, dtype):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    return x.to(device=dev, dtype=dtype)


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor):
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance, ransac_n=3,
                                                max_iteration=1000, max_validation=1000, seed=0):
    """open3d.registration.registration_ransac_based_on_correspondence with TransformationEstimationPointToPoint(False) and no
    checkers: source [Ns,3] and target [Nt,3] points (tensors or numpy), corres [M,2] (source row, target row).
    min(max_iteration, max_validation) hypotheses.  -> RegistrationResult(transformation [4,4] f32 on the device,
    correspondence_set [K,2] int64 on the device (the winner's inlier rows of corres), fitness, inlier_rmse)."""
    what = "registration_ransac_based_on_correspondence"
    dev = _device_of(source, target, corres)
    require_device(dev, "the points", what)
    src_pts = _on_device(source, dev, torch.float32)
    tgt_pts = _on_device(target, dev, torch.float32)
    c = _on_device(corres, dev, torch.int64)
    if c.dim() != 2 or c.shape[1] != 2:
        fail(what, f"corres must be [M,2] (got {tuple(c.shape)})")
    H = min(int(max_iteration), int(max_validation))
    if H < 1:
        fail(what, "max_iteration and max_validation must be >= 1")
    if c.shape[0] == 0:
        return RegistrationResult(torch.eye(4, device=dev), c.clone(), 0.0, 0.0)
    lo, hi0, hi1 = torch.stack([c.min(), c[:, 0].max(), c[:, 1].max()]).tolist()      # (a host read: indices are checked)
    if lo < 0 or hi0 >= src_pts.shape[0] or hi1 >= tgt_pts.shape[0]:
        fail(what, "corres holds a row outside source / target")
    T, inl, fit, rmse, _, _ = ransac_correspondence_batched(src_pts[c[:, 0]][None], tgt_pts[c[:, 1]][None],
                                                            max_correspondence_distance, ransac_n=ransac_n, num_hypotheses=H,
                                                            seed=seed)
    info = torch.stack([fit[0], rmse[0], inl[0].sum().float()]).cpu().tolist()     # the result's size
    corr = torch.nonzero_static(inl[0], size=int(info[2])).view(-1)
    return RegistrationResult(T[0], c[corr], info[0], info[1])


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, max_correspondence_distance,
                                                  ransac_n=4, checker_distance=None, edge_length_threshold=None,
                                                  max_iteration=100000, max_validation=1000, seed=0, search="grid"):
    """open3d.registration.registration_ransac_based_on_feature_matching with TransformationEstimationPointToPoint(False):
    source [Ns,3] and target [Nt,3] points, source_feature [Ns,d] and target_feature [Nt,d] descriptors (tensors or numpy),
    one row per point.  open3d's Feature objects and their [d, N] `data` layout are NOT accepted: pass `feature.data.T`.
    checker_distance is open3d's CorrespondenceCheckerBasedOnDistance(d), edge_length_threshold its
    CorrespondenceCheckerBasedOnEdgeLength(r); max_iteration and max_validation are its RANSACConvergenceCriteria.  The
    descriptors are matched with `find_knn_gpu`, then `ransac_feature_matching_batched` runs (its docstring has the rules).
    -> RegistrationResult(transformation [4,4] f32 on the device, correspondence_set [K,2] int64 on the device (source row,
    geometric nearest target row) of the winner's C, fitness, inlier_rmse).  One host read, for the result's size."""
    from .matching import find_knn_gpu
    what = "registration_ransac_based_on_feature_matching"
    for x, f, name in ((source, source_feature, "source"), (target, target_feature, "target")):
        xs, fs = tuple(np.shape(x)), tuple(np.shape(f))
        if len(xs) != 2 or xs[1] != 3 or len(fs) != 2 or fs[0] != xs[0]:
            fail(what, f"{name} must be [N,3] and {name}_feature [N,d], one row per point (got {xs} / {fs}; open3d's [d,N] "
                       "Feature layout is not accepted)")
    if np.shape(source_feature)[1] != np.shape(target_feature)[1]:
        fail(what, f"source_feature and target_feature differ in width ({np.shape(source_feature)[1]} / "
                   f"{np.shape(target_feature)[1]})")
    dev = _device_of(source, target, source_feature, target_feature)
    require_device(dev, "the points", what)
    S = _on_device(source, dev, torch.float32)
    Q = _on_device(target, dev, torch.float32)
    F0 = _on_device(source_feature, dev, torch.float32)
    F1 = _on_device(target_feature, dev, torch.float32)
    nn = find_knn_gpu(F0.contiguous(), F1.contiguous(), nn_max_n=-1, knn=1).reshape(-1)
    T, fit, rmse, _, _, nn_out, _ = ransac_feature_matching_batched(
        S[None], Q[None], nn[None], max_correspondence_distance, ransac_n=ransac_n, max_iteration=max_iteration,
        max_validation=max_validation, checker_distance=checker_distance, edge_length_threshold=edge_length_threshold, seed=seed,
        search=search)
    nn_out = nn_out[0]
    info = torch.stack([fit[0], rmse[0], (nn_out >= 0).sum().float()]).cpu().tolist()   # the one synchronisation
    rows = torch.nonzero_static(nn_out >= 0, size=int(info[2])).view(-1)
    return RegistrationResult(T[0], torch.stack([rows, nn_out[rows]], 1), info[0], info[1])


def check_estimation(what, name, estimation):
    if not isinstance(estimation, str) or estimation not in _ICP_ESTIMATION:
        fail(what, f'{name} must be "point_to_point" or "point_to_plane" (got {estimation!r})')
    return estimation == "point_to_plane"


def registration_icp(source, target, max_correspondence_distance, init=None, max_iteration=30, relative_fitness=1e-6,
                     relative_rmse=1e-6, search="brute", estimation="point_to_point", target_normals=None):
    """open3d.registration.registration_icp with TransformationEstimationPointToPoint(): source [Ns,3], target [Nt,3] (tensors
    or numpy), init [4,4] (default identity); search: "brute" or "grid", as in icp_point_to_point_batched.
    estimation="point_to_plane" is TransformationEstimationPointToPlane() and takes target_normals [Nt,3] (open3d reads them
    from the target cloud), as in icp_point_to_plane_batched.
    -> RegistrationResult(transformation [4,4] f32 on the device, correspondence_set [K,2] int64 on the device (source row,
    nearest target row) of the final C, fitness, inlier_rmse)."""
    what = "registration_icp"
    if not isinstance(search, str) or search not in _ICP_SEARCH:
        fail(what, f'search must be "brute" or "grid" (got {search!r})')
    plane = check_estimation(what, "estimation", estimation)
    if plane and target_normals is None:
        fail(what, 'estimation="point_to_plane" needs target_normals')
    if plane and not isinstance(target_normals, (torch.Tensor, np.ndarray)):
        fail(what, "target_normals must be a tensor or a NumPy array")
    dev = _device_of(source, target, init)
    require_device(dev, "the points", what)
    S = _on_device(source, dev, torch.float32)
    Q = _on_device(target, dev, torch.float32)
    T0 = torch.eye(4, device=dev) if init is None else _on_device(init, dev, torch.float32)
    if T0.shape != (4, 4):
        fail(what, f"init must be [4,4] (got {tuple(T0.shape)})")
    crit = dict(max_iteration=max_iteration, relative_fitness=relative_fitness, relative_rmse=relative_rmse, search=search)
    if plane:
        Nn = _on_device(target_normals, dev, torch.float32)
        if Nn.shape != Q.shape:
            fail(what, f"target_normals must be [Nt,3], one normal per target row (got {tuple(Nn.shape)} for {tuple(Q.shape)})")
        T, fit, rmse, _, nn = icp_point_to_plane_batched(S[None], Q[None], Nn[None], T0[None], max_correspondence_distance, **crit)
    else:
        T, fit, rmse, _, nn = icp_point_to_point_batched(S[None], Q[None], T0[None], max_correspondence_distance, **crit)
    nn = nn[0]
    info = torch.stack([fit[0], rmse[0], (nn >= 0).sum().float()]).cpu().tolist()   # the one synchronisation
    rows = torch.nonzero_static(nn >= 0, size=int(info[2])).view(-1)
    return RegistrationResult(T[0], torch.stack([rows, nn[rows]], 1), info[0], info[1])


def registration_colored_icp(source, target, source_colors, target_colors, target_normals, max_correspondence_distance, init=None,
                             lambda_geometric=0.968, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, search="brute"):
    """open3d.registration.registration_colored_icp (0.9): source [Ns,3], target [Nt,3], source_colors [Ns,3] or [Ns],
    target_colors [Nt,3] or [Nt], target_normals [Nt,3] (tensors or numpy; open3d reads the colours and the normals from the
    clouds), init [4,4] (default identity); the rest as in icp_colored_batched, which computes the targets' colour gradients.
    -> RegistrationResult(transformation [4,4] f32 on the device, correspondence_set [K,2] int64 on the device (source row,
    nearest target row) of the final C, fitness, inlier_rmse (Euclidean))."""
    what = "registration_colored_icp"
    if not isinstance(search, str) or search not in _ICP_SEARCH:
        fail(what, f'search must be "brute" or "grid" (got {search!r})')
    for x, name in ((source_colors, "source_colors"), (target_colors, "target_colors"), (target_normals, "target_normals")):
        if not isinstance(x, (torch.Tensor, np.ndarray)):
            fail(what, f"{name} must be a tensor or a NumPy array")
    unit_interval(what, "lambda_geometric", lambda_geometric)
    dev = _device_of(source, target, init)
    require_device(dev, "the points", what)
    S = _on_device(source, dev, torch.float32)
    Q = _on_device(target, dev, torch.float32)
    Cs, Ct, Nn = (_on_device(x, dev, torch.float32) for x in (source_colors, target_colors, target_normals))
    T0 = torch.eye(4, device=dev) if init is None else _on_device(init, dev, torch.float32)
    if T0.shape != (4, 4):
        fail(what, f"init must be [4,4] (got {tuple(T0.shape)})")
    if Nn.shape != Q.shape:
        fail(what, f"target_normals must be [Nt,3], one normal per target row (got {tuple(Nn.shape)} for {tuple(Q.shape)})")
    for c, x, name in ((Cs, S, "source"), (Ct, Q, "target")):
        if c.shape != x.shape and c.shape != x.shape[:1]:
            fail(what, f"{name}_colors must be [N,3] or [N], one per {name} row (got {tuple(c.shape)} for {tuple(x.shape)})")
    T, fit, rmse, _, nn = icp_colored_batched(S[None], Q[None], Cs[None], Ct[None], Nn[None], T0[None], max_correspondence_distance,
                                              max_iteration=max_iteration, relative_fitness=relative_fitness,
                                              relative_rmse=relative_rmse, search=search, lambda_geometric=lambda_geometric)
    nn = nn[0]
    info = torch.stack([fit[0], rmse[0], (nn >= 0).sum().float()]).cpu().tolist()   # the one synchronisation
    rows = torch.nonzero_static(nn >= 0, size=int(info[2])).view(-1)
    return RegistrationResult(T[0], torch.stack([rows, nn[rows]], 1), info[0], info[1])


def icp_refine(src_keypts, tgt_keypts, pred_trans):
    """Drop-in for GMF_PointDSC/evaluation/benchmark_utils.py:40-56, batched: src_keypts, tgt_keypts [B,N,3], pred_trans
    [B,4,4] -> the refined [B,4,4] float32 (point-to-point ICP, tau = 0.10, open3d's default criteria).  No host
    synchronisation."""
    T, _, _, _, _ = icp_point_to_point_batched(src_keypts, tgt_keypts, pred_trans.detach().float(), 0.10)
    return T
