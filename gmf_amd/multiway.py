"""Multiway registration of a fragment sequence on the device: what
GMF_PointDSC/multiway/test_multi_ate.py does between PointDSC's pair poses and the trajectory, where the reference calls open3d
0.9 on the host.  Kernels: csrc/posegraph_kernels.hip (plus the ICP and voxel kernels that were there).

  information_matrix_batched(...)      get_information_matrix_from_point_clouds (test_multi_ate.py:69-72, 141-146), E edges over
                                       F shared clouds in one call
  global_optimization(...)             global_optimization with GlobalOptimizationLevenbergMarquardt (166-174, 217-224), G graphs
  local_refinement_batched(...)        multi_scale_icp / local_refinement (54-83)
  loop_closure_mask(...)               the overlap filter (147)
  odometry_poses(...)                  the odometry chain (129-130)
  absolute_trajectory_error(...)       align and the RMSE (268-287)
  multiway_registration(...)           eval_redwood_scene from the pair poses on (86-227)

Which cloud an edge joins (`edge_source`, `edge_target`), the clouds' offsets and the graphs' offsets are host data (lists, NumPy
arrays or CPU tensors): the calls plan their work from them.  Everything measured - points, poses, information matrices, masks,
line processes - stays on the device."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._args import c_ints, check_offsets, fail, positive_finite, require_device, same_device, unit_interval
from ._util import handle_and_stream
from .common import rigid_transform_3d
from .features import (color_gradients_batched, color_intensity, estimate_normals_batched, voxel_down_sample_batched,
                       voxel_down_sample_colored_batched)
from .solvers import check_estimation, icp_colored_batched, icp_point_to_plane_batched, icp_point_to_point_batched

STOP_REASONS = ("max_iteration", "min_right_term", "min_relative_increment", "min_relative_residual_increment", "min_residual",
                "max_iteration_lm", "pivot")
MAX_NODES, MAX_EDGES = 256, 65536

DEFAULT_CRITERIA = dict(max_iteration=100, max_iteration_lm=20, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                        min_right_term=1e-6, min_residual=1e-6)


def _host_ints(x, name, what):
    """A host list of ints from a list, a NumPy array or a CPU tensor."""
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            fail(what, f"`{name}` is host data (a list, a NumPy array or a CPU tensor): the call plans its work from it")
        x = x.tolist()
    elif isinstance(x, np.ndarray):
        x = x.tolist()
    try:
        out = [int(v) for v in x]
    except (TypeError, ValueError):
        fail(what, f"`{name}` must be a sequence of integers")
    return out


def _check_clouds(points, cloud_offsets, what):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] == 0:
        fail(what, "`points` must be a non-empty [sum N, 3] tensor")
    if points.dtype != torch.float32:
        fail(what, f"`points` must be float32 (got {points.dtype})")
    return check_offsets(what, "cloud_offsets", _host_ints(cloud_offsets, "cloud_offsets", what), points.shape[0])


def _check_edges(edge_source, edge_target, n, what, which="cloud"):
    src, tgt = _host_ints(edge_source, "edge_source", what), _host_ints(edge_target, "edge_target", what)
    if len(src) != len(tgt):
        fail(what, "edge_source and edge_target must have the same length")
    if any(not 0 <= v < n for v in src + tgt):
        fail(what, f"an edge names a {which} outside 0..{n - 1}")
    return src, tgt


def _check_transformations(T, E, name, what):
    if not isinstance(T, torch.Tensor) or T.dtype not in (torch.float32, torch.float64) or tuple(T.shape) != (E, 4, 4):
        fail(what, f"`{name}` must be a float32 or float64 [{E}, 4, 4] tensor")


def information_matrix_batched(points, cloud_offsets, edge_source, edge_target, transformation, max_correspondence_distance,
                               return_nn=False):
    """open3d 0.9's get_information_matrix_from_point_clouds for E edges over F clouds packed once.

    points [sum N, 3] float32 on the device with `cloud_offsets` (F + 1 host ints); edge e joins the clouds edge_source[e] and
    edge_target[e] (host ints; a cloud may serve any number of edges and is put on the search grid once; source == target is
    legal); transformation [E, 4, 4] float64 or float32 maps source rows into the target's frame.  C_e = the source rows whose
    transformed row has its exact nearest target row within max_correspondence_distance - bit for bit what
    `icp_point_to_point_batched(..., max_iteration=0)` returns as `nn` for that pair - and info_e = the sum over C_e of G^T G in
    fp64, G = [-[q]x | I] at the matched TARGET row q.  So info[3:, 3:] = |C_e| I exactly and info[5, 5] = count.  No
    floating-point atomics: an edge's 36 numbers are the same bits alone or in any batch.  A non-finite transformation gives
    zeros.

    Returns info [E, 6, 6] float64, count [E] int32 and, with return_nn, nn [sum of the edges' source rows] int64 (the matched
    target row within its cloud, -1 outside C_e; edge after edge)."""
    what = "information_matrix_batched"
    off = _check_clouds(points, cloud_offsets, what)
    F = len(off) - 1
    src, tgt = _check_edges(edge_source, edge_target, F, what)
    E = len(src)
    _check_transformations(transformation, E, "transformation", what)
    tau = positive_finite(what, "max_correspondence_distance", max_correspondence_distance, rule="> 0")
    require_device(points, "points", what)
    require_device(transformation, "transformation", what)
    same_device(what, points=points, transformation=transformation)
    dev = points.device
    P = points.contiguous()
    T = transformation.to(torch.float64).contiguous()
    info = torch.zeros((E, 6, 6), device=dev, dtype=torch.float64)
    count = torch.zeros(E, device=dev, dtype=torch.int32)
    rows = sum(off[s + 1] - off[s] for s in src)
    nn = torch.empty(rows, device=dev, dtype=torch.int64) if return_nn else None
    if E:
        h, st = handle_and_stream(P)
        h.call("gmf_information_matrix", P.data_ptr(), c_ints(off), F, c_ints(src), c_ints(tgt), E, T.data_ptr(), tau,
               info.data_ptr(), count.data_ptr(), nn.data_ptr() if return_nn and rows else None, st)
    return (info, count, nn) if return_nn else (info, count)


def global_optimization(poses, edge_source, edge_target, edge_transformation, edge_information, edge_uncertain, edge_mask=None,
                        node_offsets=None, edge_offsets=None, edge_prune_threshold=0.25, preference_loop_closure=1.0,
                        reference_node=-1, criteria=None, trace=False):
    """open3d's global_optimization (Levenberg-Marquardt, a line process per uncertain edge; one call = two passes with the
    pruning in between) for G ragged pose graphs, one workgroup each.  The algorithm is written out in DESIGN.md section 4m and
    restated in float64 NumPy in tests/posegraph_reference.py.

    poses [n, 4, 4] (float64, or float32 which is widened), edge_source / edge_target [m] host ints numbering the nodes WITHIN
    their graph, edge_transformation [m, 4, 4] (maps the source node's frame into the target's: X = P_t^-1 P_s), edge_information
    [m, 6, 6], edge_uncertain [m] bool (loop closures), edge_mask [m] bool or None (False: the edge is treated as absent),
    node_offsets / edge_offsets (G + 1 host ints; None: one graph).  The defaults are open3d's; the reference passes
    edge_prune_threshold 0.25, preference_loop_closure 20.0, reference_node 0.  `criteria`: a dict over DEFAULT_CRITERIA.

    Returns poses [n, 4, 4] float64 (a reference node's pose bit for bit), line_process [m] float64 (pass 2's; 0 for an edge that
    is masked or pruned), kept [m] bool and stats: "iterations", "rejected", "stop", "edges" [G, 2] int32 per graph and pass,
    "residual" [G, 2] float64, and with trace=True "trace" [G, 2, max_iteration + 1, 2] (residual and lambda at the start and
    after every outer iteration, NaN padded).  All on the device; STOP_REASONS names the stop codes.  At most 256 nodes and
    65 536 edges per graph."""
    what = "global_optimization"
    if not isinstance(poses, torch.Tensor) or poses.dim() != 3 or poses.shape[1:] != (4, 4) or poses.shape[0] == 0 \
            or poses.dtype not in (torch.float32, torch.float64):
        fail(what, "`poses` must be a non-empty float64 or float32 [n, 4, 4] tensor")
    n = poses.shape[0]
    src, tgt = _host_ints(edge_source, "edge_source", what), _host_ints(edge_target, "edge_target", what)
    m = len(src)
    if len(tgt) != m:
        fail(what, "edge_source and edge_target must have the same length")
    if (node_offsets is None) != (edge_offsets is None):
        fail(what, "give both node_offsets and edge_offsets, or neither")
    noff = [0, n] if node_offsets is None else _host_ints(node_offsets, "node_offsets", what)
    eoff = [0, m] if edge_offsets is None else _host_ints(edge_offsets, "edge_offsets", what)
    G = len(noff) - 1
    if G < 1 or len(eoff) != G + 1 or noff[0] != 0 or eoff[0] != 0 or noff[-1] != n or eoff[-1] != m \
            or any(b <= a for a, b in zip(noff, noff[1:])) or any(b < a for a, b in zip(eoff, eoff[1:])):
        fail(what, "node_offsets must increase strictly from 0 to n and edge_offsets must not decrease from 0 to m, G + 1 entries each")
    for g in range(G):
        ng, mg = noff[g + 1] - noff[g], eoff[g + 1] - eoff[g]
        if ng > MAX_NODES or mg > MAX_EDGES:
            raise NotImplementedError(f"gmf_amd.{what}: graph {g} has {ng} nodes and {mg} edges; the kernel is built for at most "
                                      f"{MAX_NODES} nodes and {MAX_EDGES} edges per graph")
        for k in range(eoff[g], eoff[g + 1]):
            if not (0 <= src[k] < ng and 0 <= tgt[k] < ng):
                fail(what, f"edge {k} names a node outside its graph (0..{ng - 1})")
            if src[k] == tgt[k]:
                fail(what, f"edge {k} joins node {src[k]} to itself")
    _check_transformations(edge_transformation, m, "edge_transformation", what)
    if not isinstance(edge_information, torch.Tensor) or tuple(edge_information.shape) != (m, 6, 6) \
            or edge_information.dtype not in (torch.float32, torch.float64):
        fail(what, f"`edge_information` must be a float64 or float32 [{m}, 6, 6] tensor")
    for name, x in (("edge_uncertain", edge_uncertain),) + ((("edge_mask", edge_mask),) if edge_mask is not None else ()):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.bool or tuple(x.shape) != (m,):
            fail(what, f"`{name}` must be a bool [{m}] tensor")
    crit = dict(DEFAULT_CRITERIA)
    for k, v in (criteria or {}).items():
        if k not in crit:
            fail(what, f"unknown criterion {k!r} (known: {sorted(crit)})")
        crit[k] = v
    if not (0 <= int(crit["max_iteration"]) <= 100000 and 0 <= int(crit["max_iteration_lm"]) <= 100000):
        fail(what, "max_iteration and max_iteration_lm must be in 0..100000")
    p = float(preference_loop_closure)
    if not (p > 0 and np.isfinite(p)):
        fail(what, "preference_loop_closure must be > 0")
    tensors = [("poses", poses), ("edge_transformation", edge_transformation), ("edge_information", edge_information),
               ("edge_uncertain", edge_uncertain)] + ([("edge_mask", edge_mask)] if edge_mask is not None else [])
    for name, x in tensors:
        require_device(x, name, what)
        if x.device != poses.device:
            fail(what, "every tensor must live on the same device")
    dev = poses.device
    P = poses.to(torch.float64).contiguous().clone()
    X = edge_transformation.to(torch.float64).contiguous()
    L = edge_information.to(torch.float64).contiguous()
    unc = edge_uncertain.contiguous()
    mask = edge_mask.contiguous() if edge_mask is not None else None
    lp = torch.zeros(m, device=dev, dtype=torch.float64)
    kept = torch.zeros(m, device=dev, dtype=torch.bool)
    st_i = torch.zeros((G, 2, 4), device=dev, dtype=torch.int32)
    resid = torch.zeros((G, 2), device=dev, dtype=torch.float64)
    tr = torch.empty((G, 2, int(crit["max_iteration"]) + 1, 2), device=dev, dtype=torch.float64) if trace else None
    opt = _lib.PoseGraphOptions(int(crit["max_iteration"]), int(crit["max_iteration_lm"]), int(reference_node),
                                float(crit["min_relative_increment"]), float(crit["min_relative_residual_increment"]),
                                float(crit["min_right_term"]), float(crit["min_residual"]), float(edge_prune_threshold), p)
    h, st = handle_and_stream(P)
    h.call("gmf_posegraph_optimize", P.data_ptr(), c_ints(noff), c_ints(eoff), G, c_ints(src), c_ints(tgt),
           X.data_ptr() if m else None, L.data_ptr() if m else None, unc.data_ptr() if m else None,
           mask.data_ptr() if (mask is not None and m) else None, ctypes.byref(opt), lp.data_ptr() if m else None,
           kept.data_ptr() if m else None, st_i.data_ptr(), resid.data_ptr(), tr.data_ptr() if trace else None, st)
    stats = {"iterations": st_i[:, :, 0], "rejected": st_i[:, :, 1], "stop": st_i[:, :, 2], "edges": st_i[:, :, 3], "residual": resid}
    if trace:
        stats["trace"] = tr
    return P, lp, kept, stats


def loop_closure_mask(info, n_source, n_target, transformation, min_overlap=0.30):
    """The reference's filter on a loop closure (test_multi_ate.py:147): an edge is kept unless info[5, 5] / min(Ns, Nt) <
    min_overlap or trace(T) == 4.  info [E, 6, 6], n_source / n_target [E] (tensors, or host sequences), transformation
    [E, 4, 4].  -> a bool [E] device tensor, for `edge_mask`."""
    dev = info.device
    ns = torch.as_tensor(n_source, device=dev).to(torch.float64)
    nt = torch.as_tensor(n_target, device=dev).to(torch.float64)
    small = info[:, 5, 5].to(torch.float64) / torch.minimum(ns, nt) < min_overlap
    ident = torch.diagonal(transformation, dim1=1, dim2=2).sum(1) == 4.0
    return ~(small | ident)


def odometry_poses(edge_transformation):
    """The odometry chain of the n - 1 consecutive edges (i, i + 1), in order: pose_0 = I and pose_{i+1} = (X_i ... X_0)^-1 in
    float64 (test_multi_ate.py:129-130).  -> [n, 4, 4] float64 on the device of the input.  The products run as one scan of 4 x 4
    float64 matmuls (plumbing, n - 1 tiny launches); the inverse is the rigid one."""
    X = edge_transformation.to(torch.float64)
    dev = X.device
    acc = torch.eye(4, device=dev, dtype=torch.float64)
    out = [acc]
    for i in range(X.shape[0]):
        acc = X[i] @ acc
        R, t = acc[:3, :3], acc[:3, 3]
        inv = torch.eye(4, device=dev, dtype=torch.float64)
        inv[:3, :3] = R.T
        inv[:3, 3] = -(R.T @ t)
        out.append(inv)
    return torch.stack(out)


def absolute_trajectory_error(gt_poses, poses):
    """The reference's ATE (test_multi_ate.py align, 268-287): the positions of `poses` are aligned rigidly to those of `gt_poses`
    (Kabsch, `rigid_transform_3d`) and the RMSE of what is left is returned in cm, as a 0-d device tensor."""
    a = poses[:, :3, 3].to(torch.float32)[None].contiguous()
    b = gt_poses[:, :3, 3].to(device=poses.device, dtype=torch.float32)[None].contiguous()
    T = rigid_transform_3d(a, b)[0].to(torch.float64)
    err = poses[:, :3, 3].to(torch.float64) @ T[:3, :3].T + T[:3, 3] - gt_poses[:, :3, 3].to(device=poses.device, dtype=torch.float64)
    return torch.sqrt((err * err).sum(1).mean()) * 100.0


def _gather_index(off, clouds, dev):
    """Row index that packs clouds[0], clouds[1], ... one after the other, and the packed offsets (host list)."""
    parts, packed = [], [0]
    for c in clouds:
        parts.append(torch.arange(off[c], off[c + 1], device=dev))
        packed.append(packed[-1] + off[c + 1] - off[c])
    return torch.cat(parts), packed


def local_refinement_batched(points, cloud_offsets, edge_source, edge_target, init, voxel_size=(0.05, 0.025, 0.0125),
                             max_iter=(50, 30, 14), max_correspondence_distance=0.05 * 1.4, memory_budget=1 << 30,
                             estimation="point_to_point"):
    """The reference's `local_refinement` / `multi_scale_icp` (test_multi_ate.py:54-83) for E edges over F shared clouds.

    At each scale the F clouds are voxel-down-sampled ONCE (`voxel_down_sample_batched`), then every edge runs
    `icp_point_to_point_batched(search="grid")` from the previous scale's pose with max_correspondence_distance 0.05 * 1.4 and
    open3d's default relative criteria.  The information matrix is taken at the last scale with 1.4 x that voxel size
    (`information_matrix_batched`, over the shared clouds).  ICP takes one cloud pair per entry, so the edges are gathered in
    chunks whose packed source and target rows stay under `memory_budget` bytes.
    estimation="point_to_plane" is open3d's multi-scale recipe instead: each scale estimates the normals of the F down-sampled
    clouds ONCE (`estimate_normals_batched`, radius 2 x the voxel size, 30 neighbours), gathers them with each chunk's targets
    (12 more bytes per target row in the budget) and runs `icp_point_to_plane_batched(search="grid")`.  The information matrix
    is the same either way.

    init [E, 4, 4].  Returns transformation [E, 4, 4] float32 and info [E, 6, 6] float64.  Host traffic: the F + 1 offsets of the
    down-sampled clouds once per scale (the voxel call synchronises for its row count anyway); nothing per edge."""
    what = "local_refinement_batched"
    off = _check_clouds(points, cloud_offsets, what)
    F = len(off) - 1
    src, tgt = _check_edges(edge_source, edge_target, F, what)
    E = len(src)
    _check_transformations(init, E, "init", what)
    if len(voxel_size) != len(max_iter) or not len(max_iter):
        fail(what, "voxel_size and max_iter must have the same, non-zero length")
    plane = check_estimation(what, "estimation", estimation)
    require_device(points, "points", what)
    require_device(init, "init", what)
    dev = points.device
    T = init.to(torch.float32).contiguous()
    info = torch.zeros((E, 6, 6), device=dev, dtype=torch.float64)
    if E == 0:
        return T, info
    for scale, (vs, it) in enumerate(zip(voxel_size, max_iter)):
        down, doff_dev = voxel_down_sample_batched(points, off, float(vs))
        doff = doff_dev.tolist()
        normals = estimate_normals_batched(down, doff, 2.0 * float(vs), 30) if plane else None
        per_row = 3 * 4 + 8                                           # a packed fp32 row and its nn
        per_tgt = 3 * 4 if plane else 0                               # and a target row's normal
        k = 0
        while k < E:
            used, k1 = 0, k                                           # (used: the chunk's bytes so far)
            while k1 < E:
                n_tgt = doff[tgt[k1] + 1] - doff[tgt[k1]]
                need = (doff[src[k1] + 1] - doff[src[k1]] + n_tgt) * per_row + n_tgt * per_tgt
                if k1 > k and used + need > memory_budget:
                    break
                used += need
                k1 += 1
            si, soff = _gather_index(doff, src[k:k1], dev)
            ti, toff = _gather_index(doff, tgt[k:k1], dev)
            if plane:
                Tk = icp_point_to_plane_batched(down[si], down[ti], normals[ti], T[k:k1].contiguous(), max_correspondence_distance,
                                                soff, toff, max_iteration=int(it), search="grid")[0]
            else:
                Tk = icp_point_to_point_batched(down[si], down[ti], T[k:k1].contiguous(), max_correspondence_distance, soff, toff,
                                                max_iteration=int(it), search="grid")[0]
            T = torch.cat([T[:k], Tk, T[k1:]])
            k = k1
        if scale == len(max_iter) - 1:
            info = information_matrix_batched(down, doff, src, tgt, T, 1.4 * float(vs))[0]
    return T, info


def colored_refinement_batched(points, colors, cloud_offsets, edge_source, edge_target, init, voxel_size=(0.05, 0.025, 0.0125),
                               max_iter=(50, 30, 14), lambda_geometric=0.968, memory_budget=1 << 30):
    """open3d's reconstruction-system refinement of fragment pairs (multi-scale `registration_colored_icp`) for E edges over F
    shared clouds with a colour per row, laid out like `local_refinement_batched`.

    points [sum N,3] and colors [sum N,3] (float32, colours in 0..1, as `tsdf_fragments_colored` returns them).  At each scale
    the F clouds are prepared ONCE: `voxel_down_sample_colored_batched`, `estimate_normals_batched` (radius 2 x the voxel size,
    30 neighbours) and `color_gradients_batched` (radius 2 x 1.4 x the voxel size, 30 neighbours).  Then every edge runs
    `icp_colored_batched(search="grid")` from the previous scale's pose with max_correspondence_distance 1.4 x the voxel size
    and open3d's default relative criteria, in chunks whose packed rows stay under `memory_budget` bytes: a packed fp32 row and
    its nn, a source row's intensity, and a target row's intensity, normal and gradient.  The information matrix is taken at the
    last scale with 1.4 x that voxel size (`information_matrix_batched`).

    init [E, 4, 4].  Returns transformation [E, 4, 4] float32 and info [E, 6, 6] float64.  Host traffic: the F + 1 offsets of the
    down-sampled clouds once per scale; nothing per edge."""
    what = "colored_refinement_batched"
    off = _check_clouds(points, cloud_offsets, what)
    F = len(off) - 1
    src, tgt = _check_edges(edge_source, edge_target, F, what)
    E = len(src)
    _check_transformations(init, E, "init", what)
    if len(voxel_size) != len(max_iter) or not len(max_iter):
        fail(what, "voxel_size and max_iter must have the same, non-zero length")
    if not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32 or colors.shape != points.shape:
        fail(what, f"colors must be a float32 tensor of points' shape {tuple(points.shape)}, one colour per row")
    lam = unit_interval(what, "lambda_geometric", lambda_geometric)
    require_device(points, "points", what)
    require_device(init, "init", what)
    same_device(what, points=points, colors=colors)
    dev = points.device
    T = init.to(torch.float32).contiguous()
    info = torch.zeros((E, 6, 6), device=dev, dtype=torch.float64)
    if E == 0:
        return T, info
    for scale, (vs, it) in enumerate(zip(voxel_size, max_iter)):
        tau = 1.4 * float(vs)
        down, cdown, doff_dev = voxel_down_sample_colored_batched(points, colors, off, float(vs))
        doff = doff_dev.tolist()
        normals = estimate_normals_batched(down, doff, 2.0 * float(vs), 30)
        inten = color_intensity(what, "colors", cdown, cdown.shape[:1])
        grads = color_gradients_batched(down, normals, inten, doff, 2.0 * tau, 30)
        per_row = 3 * 4 + 8                                           # a packed fp32 row and its nn
        per_src, per_tgt = 4, 4 + 3 * 4 + 3 * 4                       # an intensity; an intensity, a normal and a gradient
        k = 0
        while k < E:
            used, k1 = 0, k                                           # (used: the chunk's bytes so far)
            while k1 < E:
                n_src, n_tgt = doff[src[k1] + 1] - doff[src[k1]], doff[tgt[k1] + 1] - doff[tgt[k1]]
                need = (n_src + n_tgt) * per_row + n_src * per_src + n_tgt * per_tgt
                if k1 > k and used + need > memory_budget:
                    break
                used += need
                k1 += 1
            si, soff = _gather_index(doff, src[k:k1], dev)
            ti, toff = _gather_index(doff, tgt[k:k1], dev)
            Tk = icp_colored_batched(down[si], down[ti], inten[si], inten[ti], normals[ti], T[k:k1].contiguous(), tau, soff, toff,
                                     max_iteration=int(it), search="grid", lambda_geometric=lam, target_gradients=grads[ti])[0]
            T = torch.cat([T[:k], Tk, T[k1:]])
            k = k1
        if scale == len(max_iter) - 1:
            info = information_matrix_batched(down, doff, src, tgt, T, tau)[0]
    return T, info


def multiway_registration(points, cloud_offsets, pair_source, pair_target, pair_transformation, use_icp=True,
                          refine_odometry=True, max_correspondence_distance=0.05 * 1.4, min_overlap=0.30, edge_prune_threshold=0.25,
                          preference_loop_closure=20.0, reference_node=0, criteria=None, voxel_size=(0.05, 0.025, 0.0125),
                          max_iter=(50, 30, 14), memory_budget=1 << 30, icp_estimation="point_to_point"):
    """`eval_redwood_scene` (test_multi_ate.py:86-227) from the pair poses on, for F fragments packed in `points` /
    `cloud_offsets` and E pairs (pair_source[e], pair_target[e]) with pair_transformation [E, 4, 4] (PointDSC's `final_trans` of
    `forward_ragged`, or any initial pose for the consecutive pairs).  Every consecutive pair (i, i + 1) must be among the pairs:
    those are the odometry edges (certain), refined by `local_refinement_batched` as the reference does (refine_odometry=False
    takes their poses as given); every other pair is a loop closure
    (uncertain), with its information matrix at max_correspondence_distance and the overlap filter.  The poses start from the
    odometry chain; `global_optimization` prunes the false closures.  With use_icp every pair is refined and the graph is
    optimised a second time over the edges that survived the first (the refinement runs for the others too and is masked out:
    which edges survived is not read back).  icp_estimation: the `estimation` of every `local_refinement_batched` call.

    Returns a dict: "poses" [F, 4, 4] float64, "kept" [E] bool, "line_process" [E], "mask" [E] bool (the overlap filter),
    "transformation" [E, 4, 4] float64 and "information" [E, 6, 6] of the edges as optimised last, "stats" (of the last
    optimisation) and "poses_odometry" [F, 4, 4] (the chain it started from)."""
    what = "multiway_registration"
    off = _check_clouds(points, cloud_offsets, what)
    F = len(off) - 1
    src, tgt = _check_edges(pair_source, pair_target, F, what)
    E = len(src)
    _check_transformations(pair_transformation, E, "pair_transformation", what)
    check_estimation(what, "icp_estimation", icp_estimation)
    if F > MAX_NODES or E > MAX_EDGES:
        raise NotImplementedError(f"gmf_amd.{what}: {F} fragments and {E} pairs; the optimiser is built for at most {MAX_NODES} nodes and "
                                  f"{MAX_EDGES} edges")
    odo = {s: e for e, (s, t) in enumerate(zip(src, tgt)) if t == s + 1}
    if any(i not in odo for i in range(F - 1)):
        fail(what, "every consecutive pair (i, i + 1) must be among the pairs: they are the odometry edges")
    if any(s == t for s, t in zip(src, tgt)):
        fail(what, "a pair joins a fragment to itself")
    require_device(points, "points", what)
    require_device(pair_transformation, "pair_transformation", what)
    dev = points.device
    odo_e = [odo[i] for i in range(F - 1)]
    odo_idx = torch.tensor(odo_e, device=dev, dtype=torch.long)
    unc = torch.ones(E, device=dev, dtype=torch.bool)
    unc[odo_idx] = False
    ns = [off[s + 1] - off[s] for s in src]
    nt = [off[t + 1] - off[t] for t in tgt]
    opt = dict(edge_prune_threshold=edge_prune_threshold, preference_loop_closure=preference_loop_closure,
               reference_node=reference_node, criteria=criteria)
    refine = dict(voxel_size=voxel_size, max_iter=max_iter, max_correspondence_distance=max_correspondence_distance,
                  memory_budget=memory_budget, estimation=icp_estimation)

    # first graph: refined odometry edges, loop closures as PointDSC gave them
    X = pair_transformation.to(torch.float64).clone()
    info, _ = information_matrix_batched(points, off, src, tgt, X, max_correspondence_distance)
    mask = loop_closure_mask(info, ns, nt, X, min_overlap) | ~unc
    if F > 1 and refine_odometry:
        To, Io = local_refinement_batched(points, off, [src[e] for e in odo_e], [tgt[e] for e in odo_e], X[odo_idx], **refine)
        X[odo_idx] = To.to(torch.float64)
        info[odo_idx] = Io
    poses0 = odometry_poses(X[odo_idx])
    poses, lp, kept, stats = global_optimization(poses0, src, tgt, X, info, unc, edge_mask=mask, **opt)
    if use_icp and E:
        Tr, info = local_refinement_batched(points, off, src, tgt, X, **refine)
        X = Tr.to(torch.float64)
        poses0 = odometry_poses(X[odo_idx])
        poses, lp, kept, stats = global_optimization(poses0, src, tgt, X, info, unc, edge_mask=kept, **opt)
    return {"poses": poses, "kept": kept, "line_process": lp, "mask": mask, "transformation": X, "information": info, "stats": stats,
            "poses_odometry": poses0}
