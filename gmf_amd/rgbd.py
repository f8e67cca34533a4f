"""RGB-D odometry on the device: the poses the fragment builder starts from, as the reference gets them
(GMF_PointDSC/multiway/make_fragments.py:34-109: open3d's compute_rgbd_odometry with RGBDOdometryJacobianFromHybridTerm on every
consecutive pair, chained into a pose graph, then optimize_posegraph_for_fragment and the TSDF integration).  Kernels:
csrc/rgbd_kernels.hip; C ABI: gmf_rgbd_pyramids, gmf_rgbd_correspondences, gmf_rgbd_odometry.

The contract is DESIGN.md section 4p, restated in numpy by tests/rgbd_reference.py; it follows open3d 0.9 as remembered, and where
it knowingly differs is listed there.  The colour-term Jacobian, the 5-point initialisation of non-adjacent key frames (`odo_init`
is the hook for it) and file reading are not here; rgbd_fragments(colors=True) fuses the colour frames as well
(fragments.py: tsdf_fragments_colored)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._args import cached_upload, fail, positive_finite, require_device
from ._util import handle_and_stream
from .fragments import tsdf_fragments, tsdf_fragments_colored
from .multiway import global_optimization, odometry_poses

MAX_LEVELS = 8
PLANES = ("I", "D", "Idx", "Idy", "Ddx", "Ddy")
_TRACE = 65                     # kRgbdTrace


def _intrinsic(what, intrinsic):
    try:
        fx, fy, cx, cy = (float(v) for v in intrinsic)
    except (TypeError, ValueError):
        fail(what, f"intrinsic must be four numbers (fx, fy, cx, cy) (got {intrinsic!r})")
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx > 0 and fy > 0):
        fail(what, f"intrinsic must be finite with fx, fy > 0 (got {intrinsic!r})")
    return fx, fy, cx, cy


class RGBDPyramids:
    """The planes of F frames, built once by `rgbd_pyramids`: per level l a device tensor [F,6,h,w] float32 (I, D, Idx, Idy, Ddx,
    Ddy; h = H >> l, w = W >> l), all levels views of one buffer."""

    def __init__(self, buffer, F, H, W, levels):
        self._buffer, self.frames, self.height, self.width, self.levels = buffer, F, H, W, levels
        self._views, o = [], 0
        for l in range(levels):
            h, w = H >> l, W >> l
            n = F * 6 * h * w
            self._views.append(buffer[o:o + n].view(F, 6, h, w))
            o += n

    @property
    def device(self):
        return self._buffer.device

    def planes(self, level):
        if not isinstance(level, (int, np.integer)) or not 0 <= level < self.levels:
            fail("rgbd_pyramids", f"level must be an integer in 0..{self.levels - 1} (got {level!r})")
        return self._views[level]


def rgbd_pyramids(color, depth, depth_scale=1000.0, depth_trunc=3.0, min_depth=0.0, max_depth=4.0, levels=3):
    """The image pyramids of F colour and depth frames (steps 1-3 of DESIGN.md section 4p), each frame processed once however many
    pairs use it.

    color [F,H,W] uint8 (I = v / 255), [F,H,W,3] uint8 (I = ((0.2990 R + 0.5870 G) + 0.1140 B) / 255 in float32) or [F,H,W]
    float32 (as it is); depth [F,H,W] uint16 (d = v / depth_scale) or float32 (metres), as in tsdf_fragments; d >= depth_trunc,
    d < min_depth, d > max_depth and d <= 0 are no measurement (NaN).  Level 0 is the 3 x 3 Gaussian of both; level l + 1 halves
    the Gaussian of I_l and D_l itself; Idx, Idy, Ddx, Ddy are the Sobel filters of each level.  Returns an RGBDPyramids; its
    .planes(level) is [F,6,h,w] float32 on the device.  No host synchronisation."""
    what = "rgbd_pyramids"
    for name, x in (("color", color), ("depth", depth)):
        if not isinstance(x, torch.Tensor):
            fail(what, f"`{name}` must be a torch tensor")
    if depth.dtype not in (torch.uint16, torch.float32):
        fail(what, f"`depth` must be uint16 (sensor values) or float32 (metres) (got {depth.dtype})")
    if depth.dim() != 3 or min(depth.shape) < 1:
        fail(what, f"`depth` must be a non-empty [F,H,W] tensor (got {tuple(depth.shape)})")
    F, H, W = depth.shape
    if color.dtype == torch.uint8 and color.dim() == 4 and tuple(color.shape) == (F, H, W, 3):
        kind = 1
    elif color.dtype in (torch.uint8, torch.float32) and tuple(color.shape) == (F, H, W):
        kind = 0 if color.dtype == torch.uint8 else 2
    else:
        fail(what, f"`color` must be [F,H,W] uint8, [F,H,W,3] uint8 or [F,H,W] float32 with depth's F, H, W = {F}, {H}, {W} "
                   f"(got {tuple(color.shape)} {color.dtype})")
    if 6 * F * H * W >= 2 ** 31:
        fail(what, f"the frames must hold fewer than 2^31 / 6 pixels (got {F * H * W})")
    scale = positive_finite(what, "depth_scale", depth_scale, numeric=True)
    far = positive_finite(what, "depth_trunc", depth_trunc, allow_inf=True, numeric=True)
    try:
        lo, hi = float(min_depth), float(max_depth)
    except (TypeError, ValueError):
        fail(what, f"min_depth and max_depth must be numbers (got {min_depth!r}, {max_depth!r})")
    if not (np.isfinite(lo) and lo >= 0 and hi > lo):
        fail(what, f"min_depth must be finite and >= 0 and max_depth above it (got {min_depth}, {max_depth})")
    if not isinstance(levels, (int, np.integer)) or not 1 <= levels <= MAX_LEVELS or (H >> (levels - 1)) < 1 or (W >> (levels - 1)) < 1:
        fail(what, f"levels must be an integer in 1..{MAX_LEVELS} that leaves the coarsest level a pixel (got {levels!r})")
    require_device(color, "color", what)
    require_device(depth, "depth", what)
    if color.device != depth.device:
        fail(what, "`color` and `depth` must live on the same device")
    levels = int(levels)
    col, dep = color.contiguous(), depth.contiguous()
    total = sum(F * 6 * (H >> l) * (W >> l) for l in range(levels))
    buf = torch.empty(total, device=depth.device, dtype=torch.float32)
    h, st = handle_and_stream(dep)
    h.call("gmf_rgbd_pyramids", col.data_ptr(), kind, dep.data_ptr(), 1 if dep.dtype == torch.uint16 else 0, F, H, W, scale, far, lo, hi,
           levels, buf.data_ptr(), st)
    return RGBDPyramids(buf, F, H, W, levels)


def _pairs(what, pyr, pair_source, pair_target):
    if not isinstance(pyr, RGBDPyramids):
        fail(what, "`pyr` must be what rgbd_pyramids returned")
    lists = []
    for name, x in (("pair_source", pair_source), ("pair_target", pair_target)):
        if isinstance(x, torch.Tensor) and x.is_cuda:
            fail(what, f"`{name}` is host data (a list, a NumPy array or a CPU tensor): the call plans its work from it")
        try:
            seq = x.tolist() if isinstance(x, (torch.Tensor, np.ndarray)) else list(x)
            v = [int(o) for o in seq]
            if any(a != b for a, b in zip(v, seq)):
                raise ValueError
        except (TypeError, ValueError):
            fail(what, f"`{name}` must be a sequence of integers")
        lists.append(v)
    src, tgt = lists
    if len(src) != len(tgt):
        fail(what, "pair_source and pair_target must have the same length")
    for e, (s, t) in enumerate(zip(src, tgt)):
        if not (0 <= s < pyr.frames and 0 <= t < pyr.frames):
            fail(what, f"pair {e} names a frame outside 0..{pyr.frames - 1}")
    if len(src) >= 1 << 24:
        fail(what, f"a call holds fewer than 2^24 pairs (got {len(src)})")
    return src, tgt


def _poses(what, name, T, E, dev):
    if not isinstance(T, torch.Tensor) or T.dtype != torch.float64 or tuple(T.shape) != (E, 4, 4):
        fail(what, f"`{name}` must be a float64 [{E}, 4, 4] tensor")
    require_device(T, name, what)
    if T.device != dev:
        fail(what, f"`{name}` must live on the device of the pyramids")
    return T.contiguous()


def _on_device(what, pyr):
    require_device(pyr.device, "the pyramids", what)
    return pyr.device


def _depth_diff(what, v):
    try:
        f = float(v)
    except (TypeError, ValueError):
        fail(what, f"max_depth_diff must be a number (got {v!r})")
    if not (np.isfinite(f) and f >= 0):
        fail(what, f"max_depth_diff must be finite and >= 0 (got {v})")
    return f


def rgbd_correspondence_map(pyr, pair_source, pair_target, transformation, intrinsic, level=0, max_depth_diff=0.03):
    """Step 4 of DESIGN.md section 4p for E pairs of frames of `pyr` under transformation [E,4,4] (float64, device; source camera
    to target camera) at `level` (intrinsic is the full-resolution one): [E,h,w] int32, per TARGET pixel the source pixel
    v_s * w + u_s that projects onto it within max_depth_diff with the smallest depth (then the smallest index), or -1."""
    what = "rgbd_correspondence_map"
    src, tgt = _pairs(what, pyr, pair_source, pair_target)
    E = len(src)
    K = _intrinsic(what, intrinsic)
    if not isinstance(level, (int, np.integer)) or not 0 <= level < pyr.levels:
        fail(what, f"level must be an integer in 0..{pyr.levels - 1} (got {level!r})")
    mdd = _depth_diff(what, max_depth_diff)
    T = _poses(what, "transformation", transformation, E, pyr.device)
    dev = _on_device(what, pyr)
    out = torch.empty((E, pyr.height >> level, pyr.width >> level), device=dev, dtype=torch.int32)
    if E == 0:
        return out
    h, st = handle_and_stream(pyr._buffer)
    pairs = cached_upload((tuple(src), tuple(tgt)), dev)[0]
    h.call("gmf_rgbd_correspondences", pyr._buffer.data_ptr(), pyr.frames, pyr.height, pyr.width, pyr.levels, int(level),
           pairs[0].data_ptr(), pairs[1].data_ptr(), E, T.data_ptr(), *K, mdd, out.data_ptr(), st)
    return out


def rgbd_odometry(pyr_or_color, depth=None, pair_source=(), pair_target=(), intrinsic=None, odo_init=None, max_depth_diff=0.03,
                  iterations=(20, 10, 5), return_trace=False, **pyramid_args):
    """open3d's compute_rgbd_odometry (hybrid Jacobian) for E frame pairs at once: DESIGN.md section 4p.

    pyr_or_color: what rgbd_pyramids returned (depth None), or colour frames with `depth` and rgbd_pyramids' other arguments as
    keywords; with iterations given, `levels` defaults to their number.  pair_source / pair_target: E host ints indexing frames;
    intrinsic (fx, fy, cx, cy) at full resolution; odo_init [E,4,4] float64 on the device (its last row is taken as 0 0 0 1), or
    None for the identity;
    iterations: per level, the coarsest first.
    Returns success [E] bool, transformation [E,4,4] float64 (source camera to target camera) and information [E,6,6] float64, all
    on the device; a failed pair (no correspondence, |det A| < 1e-6, anything non-finite) has success False and both the identity,
    and the pairs beside it are not affected.  With return_trace also a dict: "n" [E,N] int32 (-1: the iteration did not run),
    "A" [E,N,6,6], "b" [E,N,6], "r2" [E,N], "x" [E,N,6], "pose" [E,N,4,4] (NaN where not written) over the N = sum(iterations)
    iterations, and "scales" [E,2].  The same bits on every run, and a pair has the same bits alone and in any batch.  No host
    synchronisation."""
    what = "rgbd_odometry"
    try:
        its = [int(i) for i in iterations]
        if any(a != b for a, b in zip(its, iterations)) or not its or min(its) < 0 or max(its) > 10000:
            raise ValueError
    except (TypeError, ValueError):
        fail(what, f"iterations must be a sequence of integers in 0..10000, one per level (got {iterations!r})")
    K = _intrinsic(what, intrinsic)
    mdd = _depth_diff(what, max_depth_diff)
    if isinstance(pyr_or_color, RGBDPyramids):
        if depth is not None or pyramid_args:
            fail(what, "with pyramids, `depth` and the pyramid arguments are not taken: they went into rgbd_pyramids")
        pyr = pyr_or_color
    else:
        if depth is None:
            fail(what, "give what rgbd_pyramids returned, or colour frames and `depth`")
        unknown = set(pyramid_args) - {"depth_scale", "depth_trunc", "min_depth", "max_depth", "levels"}
        if unknown:
            fail(what, f"unknown argument {sorted(unknown)[0]!r}")
        pyramid_args.setdefault("levels", len(its))
        try:
            pyr = rgbd_pyramids(pyr_or_color, depth, **pyramid_args)
        except RuntimeError as err:
            raise RuntimeError(str(err).replace("gmf_amd.rgbd_pyramids", f"gmf_amd.{what}", 1)) from None
    if len(its) != pyr.levels:
        fail(what, f"iterations must have one entry per level: {pyr.levels} (got {len(its)})")
    src, tgt = _pairs(what, pyr, pair_source, pair_target)
    E, N = len(src), sum(its)
    init = None if odo_init is None else _poses(what, "odo_init", odo_init, E, pyr.device)
    dev = _on_device(what, pyr)
    success = torch.zeros(E, device=dev, dtype=torch.bool)
    T = torch.empty((E, 4, 4), device=dev, dtype=torch.float64)
    info = torch.empty((E, 6, 6), device=dev, dtype=torch.float64)
    if return_trace:
        scales = torch.full((E, 2), float("nan"), device=dev, dtype=torch.float64)
        tn = torch.full((E, N), -1, device=dev, dtype=torch.int32)
        td = torch.full((E, N, _TRACE), float("nan"), device=dev, dtype=torch.float64)
    if E:
        h, st = handle_and_stream(pyr._buffer)
        pairs = cached_upload((tuple(src), tuple(tgt)), dev)[0]
        h.call("gmf_rgbd_odometry", pyr._buffer.data_ptr(), pyr.frames, pyr.height, pyr.width, pyr.levels,
               pairs[0].data_ptr(), pairs[1].data_ptr(), E, init.data_ptr() if init is not None else None,
               *K, mdd, (C.c_int * len(its))(*its), success.data_ptr(), T.data_ptr(), info.data_ptr(),
               scales.data_ptr() if return_trace else None, tn.data_ptr() if return_trace and N else None,
               td.data_ptr() if return_trace and N else None, st)
    if return_trace:
        trace = dict(n=tn, A=td[:, :, :36].reshape(E, N, 6, 6), b=td[:, :, 36:42], r2=td[:, :, 42], x=td[:, :, 43:49],
                     pose=td[:, :, 49:65].reshape(E, N, 4, 4), scales=scales)
    return (success, T, info) + ((trace,) if return_trace else ())


def rgbd_fragments(color, depth, intrinsic, frame_offsets=None, max_depth_diff=0.07, min_depth=0.3, max_depth=3.0, optimize=True,
                   preference_loop_closure=0.1, **tsdf_args):
    """make_fragments.py's process_single_fragment for G ragged fragments: RGB-D odometry on every consecutive pair inside a
    fragment (rgbd_odometry with max_depth_diff, min_depth, max_depth), the odometry chain per fragment (odometry_poses), the
    pose-graph optimisation (global_optimization with reference_node 0, edge_prune_threshold 0.25, the consecutive edges certain;
    optimize=False skips it) and the TSDF fusion with the resulting camera-to-world poses (tsdf_fragments; tsdf_args are its
    keywords, depth_scale and depth_trunc also go to the pyramids; colors=True fuses the colour frames as well, through
    tsdf_fragments_colored, and needs [F,H,W,3] uint8 colour: a grey frame has no R, G, B to fuse).

    color, depth, intrinsic: as in rgbd_pyramids / tsdf_fragments; frame_offsets: G + 1 ints (None: one fragment).
    Returns what tsdf_fragments (colors=True: tsdf_fragments_colored) returns, then poses [F,4,4] float64 (camera to the
    fragment's first camera) and success [F - G'] bool over the consecutive pairs in order (G' fragments that hold a frame), on the device.  A fragment with a failed pair
    raises and names the pair (one host synchronisation, besides tsdf_fragments' own)."""
    what = "rgbd_fragments"
    unknown = set(tsdf_args) - {"voxel_length", "sdf_trunc", "depth_scale", "depth_trunc", "depth_sampling_stride", "max_units", "return_volume", "colors"}
    if unknown:
        fail(what, f"unknown argument {sorted(unknown)[0]!r}")
    tsdf_args = dict(tsdf_args)
    colors = tsdf_args.pop("colors", False)
    if not isinstance(colors, (bool, np.bool_)):
        fail(what, f"colors must be True or False (got {colors!r})")
    if colors and not (isinstance(color, torch.Tensor) and color.dtype == torch.uint8 and color.dim() == 4 and color.shape[-1] == 3):
        got = f"{tuple(color.shape)} {color.dtype}" if isinstance(color, torch.Tensor) else type(color).__name__
        fail(what, f"colors=True needs `color` as [F,H,W,3] uint8: a grey frame has no R, G, B to fuse (got {got})")
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
        fail(what, "`depth` must be a [F,H,W] torch tensor")
    F = depth.shape[0]
    if frame_offsets is None:
        off = [0, F]
    else:
        if isinstance(frame_offsets, torch.Tensor) and frame_offsets.is_cuda:
            fail(what, "frame_offsets must be G + 1 host integers (they size the call)")
        try:
            seq = frame_offsets.tolist() if isinstance(frame_offsets, (torch.Tensor, np.ndarray)) else list(frame_offsets)
            off = [int(o) for o in seq]
            if any(o != s for o, s in zip(off, seq)):
                raise ValueError
        except (TypeError, ValueError):
            fail(what, "frame_offsets must be G + 1 integers")
        if len(off) < 2 or off[0] != 0 or off[-1] != F or any(b < a for a, b in zip(off, off[1:])):
            fail(what, "frame_offsets must not decrease, start at 0 and end at F")
    p = float(preference_loop_closure) if isinstance(preference_loop_closure, (int, float, np.number)) else float("nan")
    if not (p > 0 and np.isfinite(p)):
        fail(what, f"preference_loop_closure must be finite and > 0 (got {preference_loop_closure!r})")
    K = _intrinsic(what, intrinsic)
    _depth_diff(what, max_depth_diff)
    src = [i for a, b in zip(off, off[1:]) for i in range(a, b - 1)]
    tgt = [i + 1 for i in src]
    pyramid_args = {k: tsdf_args[k] for k in ("depth_scale",) if k in tsdf_args}
    pyramid_args["depth_trunc"] = tsdf_args.get("depth_trunc", 3.0)
    tsdf_args.setdefault("depth_trunc", 3.0)
    try:
        if F == 0:
            if not isinstance(color, torch.Tensor):
                fail(what, "`color` must be a torch tensor")
            require_device(color, "color", what)
            require_device(depth, "depth", what)
            dev = depth.device
            success = torch.zeros(0, device=dev, dtype=torch.bool)
            poses = torch.zeros((0, 4, 4), device=dev, dtype=torch.float64)
        else:
            success, X, info = rgbd_odometry(color, depth, pair_source=src, pair_target=tgt, intrinsic=K, max_depth_diff=max_depth_diff,
                                             min_depth=min_depth, max_depth=max_depth, **pyramid_args)
            dev = X.device
            bad = torch.nonzero(~success).flatten().tolist() if len(src) else []
            if bad:
                e = bad[0]
                g = max(g for g in range(len(off) - 1) if off[g] <= src[e])
                fail(what, f"the odometry of frames {src[e]} -> {tgt[e]} (fragment {g}) failed: {len(bad)} of {len(src)} pairs did")
            parts, e0 = [], 0
            for a, b in zip(off, off[1:]):
                if b > a:
                    parts.append(odometry_poses(X[e0:e0 + b - a - 1]))
                    e0 += b - a - 1
            poses = torch.cat(parts)
            if optimize and len(src):
                # a fragment of one frame has no edge and nothing to optimise: its pose stays the identity
                graphs = [(a, b) for a, b in zip(off, off[1:]) if b - a >= 2]
                rows = torch.tensor([i for a, b in graphs for i in range(a, b)], device=dev)
                noff = [0] + list(np.cumsum([b - a for a, b in graphs]))
                eoff = [0] + list(np.cumsum([b - a - 1 for a, b in graphs]))
                es = [i for a, b in graphs for i in range(b - a - 1)]
                better = global_optimization(poses[rows], es, [i + 1 for i in es], X, info,
                                             torch.zeros(len(es), device=dev, dtype=torch.bool),
                                             node_offsets=[int(v) for v in noff], edge_offsets=[int(v) for v in eoff],
                                             edge_prune_threshold=0.25, preference_loop_closure=p, reference_node=0)[0]
                poses = poses.clone()
                poses[rows] = better
        if colors:
            out = tsdf_fragments_colored(color, depth, poses, K, frame_offsets=off, **tsdf_args)
        else:
            out = tsdf_fragments(depth, poses, K, frame_offsets=off, **tsdf_args)
    except RuntimeError as err:
        msg = str(err)
        for inner in ("rgbd_odometry", "rgbd_pyramids", "tsdf_fragments_colored", "tsdf_fragments", "global_optimization"):
            msg = msg.replace(f"gmf_amd.{inner}", f"gmf_amd.{what}", 1)
        raise RuntimeError(msg) from None
    return tuple(out) + (poses, success)
