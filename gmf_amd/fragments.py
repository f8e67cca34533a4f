"""Fragments on the device: TSDF fusion of posed depth frames to a cloud, as the reference makes them
(GMF_PointDSC/multiway/make_fragments.py:112-140 and GMF_DeepGlobalRegistration/*/util/integration.py:44-71: open3d's
ScalableTSDFVolume, integrate() per frame, extract_triangle_mesh(), of which make_fragments.py keeps the vertices).  Kernels:
csrc/tsdf_kernels.hip; C ABI: gmf_tsdf_allocate, gmf_tsdf_integrate, gmf_tsdf_extract.  tsdf_fragments_colored is the RGB8 volume
of the same scripts (color_type = RGB8, pcd.colors = mesh.vertex_colors): the same vertices and a colour for each, through
gmf_tsdf_integrate_color and gmf_tsdf_extract_color.

The contract is DESIGN.md section 4o, restated in numpy by tests/tsdf_reference.py and, for the colours (steps 3c and 4c),
tests/tsdf_color_reference.py; where it knowingly differs from open3d is listed there.  tsdf_fragment_meshes and
tsdf_extract_mesh give the mesh itself (steps 5 and 6, tests/tsdf_mesh_reference.py; gmf_tsdf_extract_mesh): the same vertices, the
triangles and, as mesh.compute_vertex_normals() does, a normal per vertex.  extract_point_cloud, grey volumes and file reading are
not here; the RGB-D odometry that gives the poses is gmf_amd/rgbd.py."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from ._args import check_offsets, device_offsets, fail, positive_finite, require_device, same_device
from ._util import handle_and_stream

MAX_FRAMES = 65535            # frames of one fragment, at most
MAX_FRAGMENTS = 65535         # fragments of one call, at most (kTsdfMaxFragments)
MAX_UNITS = 1 << 22           # the largest max_units the library takes


def _nothing(points_off, return_volume, colored=False, mesh=False):
    """The result of a call whose frames touch no unit."""
    dev = points_off.device
    if mesh:
        parts = _nothing(points_off, True, colored)
        meshes = TsdfMeshes(parts[0], points_off, torch.zeros((0, 3), device=dev, dtype=torch.int32), torch.zeros_like(points_off),
                            torch.zeros((0, 3), device=dev, dtype=torch.float32), parts[7] if colored else None)
        return (meshes, parts[2:7] + parts[8:]) if return_volume else meshes
    pts = torch.zeros((0, 3), device=dev, dtype=torch.float32)
    out = (pts, points_off)
    if return_volume:
        out += (torch.zeros((0, 3), device=dev, dtype=torch.int32), torch.zeros_like(points_off),
                torch.zeros(0, device=dev, dtype=torch.int32), torch.zeros((0, 16, 16, 16), device=dev),
                torch.zeros((0, 16, 16, 16), device=dev))
    if colored:
        out += (torch.zeros((0, 3), device=dev, dtype=torch.float32),)
        if return_volume:
            out += (torch.zeros((0, 16, 16, 16, 3), device=dev),)
    return out


def tsdf_fragments(depth, poses, intrinsic, frame_offsets=None, voxel_length=0.008, sdf_trunc=0.04, depth_scale=1000.0,
                   depth_trunc=4.5, depth_sampling_stride=4, max_units=1 << 18, return_volume=False):
    """G fragments from posed depth frames: per fragment a ScalableTSDFVolume(voxel_length, sdf_trunc) with 16^3-voxel units, every
    frame integrated in order, and the vertices of the marching-cubes mesh.

    depth [F,H,W] on the device: uint16 (sensor values, d = v / depth_scale) or float32 (metres; negative and non-finite are 0);
    d >= depth_trunc is 0, and 0 is no measurement.  poses [F,4,4] float64 camera-to-world, on the host (a device tensor is
    copied to the host first, which synchronises); they are inverted in fp64 on the host.  intrinsic (fx, fy, cx, cy): one camera
    per call.  frame_offsets: G + 1 ints, fragment g owns frames frame_offsets[g] .. frame_offsets[g+1] - 1 (possibly none);
    None: one fragment.  At most 65535 frames per fragment and 65535 fragments.
      allocation: every depth_sampling_stride-th pixel of every such row is back-projected (fp64) and the units within sdf_trunc
      of it exist; a unit's birth is the first frame of its fragment that touches it; units are listed per fragment in ascending
      (x, y, z) order;
      integration: a unit takes the frames from its birth on (open3d creates a unit when a frame first touches it), fp32,
      weight 1 per update;
      extraction: one vertex per sign-changing edge between observed voxels that lies in a fully observed 2x2x2 cube, ordered
      by fragment, unit, voxel, axis.
    Returns points [M,3] float32 and point_offsets [G+1] int32 (device); with return_volume also unit_keys [U,3] int32,
    unit_offsets [G+1] int32, birth [U] int32, tsdf [U,16,16,16] and weight [U,16,16,16] float32.
    A function of the inputs alone: the same bits on every run, and a fragment has the same bits alone and in any batch.
    Two host synchronisations per call (the unit count, the vertex count).  Raises when the frames touch more than max_units
    units (raise max_units) or a unit index leaves +-32767 (raise voxel_length)."""
    return _fragments("tsdf_fragments", None, depth, poses, intrinsic, frame_offsets, voxel_length, sdf_trunc, depth_scale, depth_trunc,
                      depth_sampling_stride, max_units, return_volume)


def tsdf_fragments_colored(color, depth, poses, intrinsic, frame_offsets=None, voxel_length=0.008, sdf_trunc=0.04, depth_scale=1000.0,
                           depth_trunc=4.5, depth_sampling_stride=4, max_units=1 << 18, return_volume=False):
    """tsdf_fragments with open3d's RGB8 volume: the same vertices, with the same bits, and a colour for each.

    color [F,H,W,3] uint8 on depth's device, channels R, G, B, the frames of `depth`; every other argument as in tsdf_fragments.
      integration: a voxel's colour starts at (0, 0, 0) and changes exactly when its tsdf does, from the same pixel:
      c = (c w + color[f,v,u]) / (w + 1) in fp32 with w the weight before the update; a pixel without a depth measurement is never
      read, and a voxel of weight 0 keeps colour 0;
      extraction: a vertex on the edge from voxel a to voxel b, ta = |tsdf_a|, tb = |tsdf_b|, has colour
      ((tb c_a + ta c_b) / (ta + tb)) / 255 in fp64, rounded once.
    Returns what tsdf_fragments returns, then colors [M,3] float32 in 0..1 (row i is the colour of points[i]); with return_volume
    also color_volume [U,16,16,16,3] float32 in 0..255 after that.  The same bits on every run, alone and in any batch; two host
    synchronisations per call."""
    return _fragments("tsdf_fragments_colored", color, depth, poses, intrinsic, frame_offsets, voxel_length, sdf_trunc, depth_scale,
                      depth_trunc, depth_sampling_stride, max_units, return_volume, colored=True)


TsdfMeshes = collections.namedtuple("TsdfMeshes", ("points", "point_offsets", "triangles", "triangle_offsets", "normals", "colors"))
TsdfMeshes.__doc__ = """The meshes of G fragments, on the device: points [M,3] float32, point_offsets [G+1] int32, triangles [K,3] int32
(each entry counts from its fragment's first vertex: fragment g's triangles index points[point_offsets[g]:point_offsets[g+1]]),
triangle_offsets [G+1] int32, normals [M,3] float32 (row i belongs to points[i]) and colors [M,3] float32 in 0..1, or None."""


def tsdf_fragment_meshes(depth, poses, intrinsic, frame_offsets=None, voxel_length=0.008, sdf_trunc=0.04, depth_scale=1000.0,
                         depth_trunc=4.5, depth_sampling_stride=4, max_units=1 << 18, color=None, return_volume=False):
    """tsdf_fragments, with the fragments as meshes: what the reference's make_fragments.py gets from
    volume.extract_triangle_mesh() and mesh.compute_vertex_normals().

    Every argument as in tsdf_fragments; with color [F,H,W,3] uint8 the volume is tsdf_fragments_colored's.  The vertices are those
    of tsdf_fragments (of tsdf_fragments_colored, with their colours), with the same bits and in the same order.
      triangles: every 2x2x2 cube of observed voxels whose corners do not all lie on one side of the surface yields the triangles
      of the classic marching-cubes table, between the vertices on its edges; ordered by fragment, unit, voxel of the cube's
      origin, table row; every vertex lies in at least one triangle;
      normals: per vertex the normalised sum, in fp64 and in ascending triangle order, of the cross products
      (p_j - p_i) x (p_l - p_i) of its triangles (i, j, l) over the returned float32 positions - area-weighted, pointing from
      negative to positive tsdf, which is towards the cameras; (0, 0, 1) where the sum has no finite positive length.
    Returns a TsdfMeshes; with return_volume the pair (TsdfMeshes, (unit_keys, unit_offsets, birth, tsdf, weight)), the volume
    followed by color_volume when there is `color`.  The same bits on every run, alone and in any batch; two host
    synchronisations per call (the unit count; the vertex and triangle counts, read back together).  `normals` is what
    icp_point_to_plane_batched takes as target normals."""
    what = "tsdf_fragment_meshes"
    return _fragments(what, color, depth, poses, intrinsic, frame_offsets, voxel_length, sdf_trunc, depth_scale, depth_trunc,
                      depth_sampling_stride, max_units, return_volume, colored=color is not None, mesh=True)


def tsdf_extract_mesh(unit_keys, unit_offsets, tsdf, weight, voxel_length, color_volume=None):
    """The meshes of a volume, as tsdf_fragments(..., return_volume=True) returns one - or any other: steps 4 to 6 of the contract.

    unit_keys [U,3] int32, tsdf and weight [U,16,16,16] float32 and, optionally, color_volume [U,16,16,16,3] float32 in 0..255, on
    one device; unit_offsets: G + 1 ints that ascend from 0 to U (fragment g owns units unit_offsets[g] .. unit_offsets[g+1] - 1),
    or an int32 tensor on that device, which is taken as it is.  voxel_length as the volume was built with.
    The volume is looked at only through weight > 0: a voxel with weight <= 0 (or NaN) is unobserved, whatever its tsdf, and no
    other property of the weights matters.  Within each fragment the keys must be ascending in (x, y, z) and distinct, each within
    +-32767, as tsdf_fragments lists them: the order of the output is defined by that listing, and it is not checked (the keys
    are on the device).
    Returns a TsdfMeshes (tsdf_fragment_meshes describes it); colors is None without a color_volume.  One host synchronisation
    (the vertex and triangle counts, read back together)."""
    what = "tsdf_extract_mesh"
    for name, x, dtype in (("unit_keys", unit_keys, torch.int32), ("tsdf", tsdf, torch.float32), ("weight", weight, torch.float32),
                           ("color_volume", color_volume, torch.float32)):
        if x is None and name == "color_volume":
            continue
        if not isinstance(x, torch.Tensor):
            fail(what, f"`{name}` must be a torch tensor")
        if x.dtype != dtype:
            fail(what, f"`{name}` must be {str(dtype).replace('torch.', '')} (got {x.dtype})")
    if unit_keys.dim() != 2 or unit_keys.shape[1] != 3:
        fail(what, f"`unit_keys` must be a [U,3] tensor (got {tuple(unit_keys.shape)})")
    U = unit_keys.shape[0]
    if U > MAX_UNITS:
        fail(what, f"a call holds at most {MAX_UNITS} units (got {U})")
    for name, x in (("tsdf", tsdf), ("weight", weight)):
        if tuple(x.shape) != (U, 16, 16, 16):
            fail(what, f"`{name}` must be [U,16,16,16] with unit_keys' U = {U} (got {tuple(x.shape)})")
    if color_volume is not None and tuple(color_volume.shape) != (U, 16, 16, 16, 3):
        fail(what, f"`color_volume` must be [U,16,16,16,3] with unit_keys' U = {U} (got {tuple(color_volume.shape)})")
    vl = positive_finite(what, "voxel_length", voxel_length, numeric=True)
    same_device(what, unit_keys=unit_keys, tsdf=tsdf, weight=weight, color_volume=color_volume)
    off = check_offsets(what, "unit_offsets", unit_offsets, U, allow_empty=True)
    G = (off.numel() if isinstance(off, torch.Tensor) else len(off)) - 1
    if G > MAX_FRAGMENTS:
        fail(what, f"a call holds at most {MAX_FRAGMENTS} fragments (got {G})")
    require_device(unit_keys, "unit_keys", what)
    dev = unit_keys.device
    dev_off, _ = device_offsets(off, U, dev, what, allow_empty=True, checked=True)
    h, st = handle_and_stream(tsdf)
    return _extract_mesh(h, st, unit_keys.contiguous(), dev_off, G, tsdf.contiguous(), weight.contiguous(),
                         None if color_volume is None else color_volume.contiguous(), vl)


def _extract_mesh(h, st, keys, unit_off, G, tsdf, weight, cvol, vl):
    """The counting and the emitting call of gmf_tsdf_extract_mesh on a checked, contiguous volume -> TsdfMeshes."""
    dev = tsdf.device
    U = keys.shape[0]
    point_off = torch.zeros(G + 1, device=dev, dtype=torch.int32)
    tri_off = torch.zeros(G + 1, device=dev, dtype=torch.int32)
    n, m = C.c_longlong(0), C.c_longlong(0)
    volume = (keys.data_ptr(), unit_off.data_ptr(), G, U, tsdf.data_ptr(), weight.data_ptr(), None if cvol is None else cvol.data_ptr(), vl)
    offsets = (point_off.data_ptr(), tri_off.data_ptr())
    if U:
        h.call("gmf_tsdf_extract_mesh", *volume, None, None, None, 0, None, 0, *offsets, C.byref(n), C.byref(m), st)
    M, K = int(n.value), int(m.value)
    pts = torch.empty((M, 3), device=dev, dtype=torch.float32)
    nrm = torch.empty((M, 3), device=dev, dtype=torch.float32)
    cols = None if cvol is None else torch.empty((M, 3), device=dev, dtype=torch.float32)
    tris = torch.empty((K, 3), device=dev, dtype=torch.int32)
    if M:
        h.call("gmf_tsdf_extract_mesh", *volume, pts.data_ptr(), nrm.data_ptr(), None if cols is None else cols.data_ptr(), M,
               tris.data_ptr(), K, *offsets, None, None, st)
    return TsdfMeshes(pts, point_off, tris, tri_off, nrm, cols)


def _fragments(what, color, depth, poses, intrinsic, frame_offsets, voxel_length, sdf_trunc, depth_scale, depth_trunc,
               depth_sampling_stride, max_units, return_volume, colored=False, mesh=False):
    """tsdf_fragments (colored False: `color` is not looked at), tsdf_fragments_colored and (mesh) tsdf_fragment_meshes: the
    argument checks, raised under the name `what`, and the calls."""
    if not isinstance(depth, torch.Tensor):
        fail(what, "`depth` must be a torch tensor")
    if depth.dtype not in (torch.uint16, torch.float32):
        fail(what, f"`depth` must be uint16 (sensor values) or float32 (metres) (got {depth.dtype})")
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        fail(what, f"`depth` must be a [F,H,W] tensor (got {tuple(depth.shape)})")
    F, H, W = depth.shape
    if F * H * W >= 2 ** 31:
        fail(what, f"`depth` must hold fewer than 2^31 pixels (got {F * H * W})")
    if colored:
        if not isinstance(color, torch.Tensor):
            fail(what, "`color` must be a torch tensor")
        if color.dtype != torch.uint8:
            fail(what, f"`color` must be uint8 (got {color.dtype})")
        if tuple(color.shape) != (F, H, W, 3):
            fail(what, f"`color` must be [F,H,W,3] (R, G, B) with depth's F, H, W = {F}, {H}, {W} (got {tuple(color.shape)})")
        if color.device != depth.device:
            fail(what, f"`color` must live on depth's device (got {color.device} and {depth.device})")
    if not isinstance(poses, torch.Tensor):
        fail(what, "`poses` must be a torch tensor")
    if poses.dtype != torch.float64:
        fail(what, f"`poses` must be float64 (got {poses.dtype})")
    if poses.dim() != 3 or tuple(poses.shape) != (F, 4, 4):
        fail(what, f"`poses` must be [F,4,4] with depth's F = {F} (got {tuple(poses.shape)})")
    try:
        fx, fy, cx, cy = (float(v) for v in intrinsic)
    except (TypeError, ValueError):
        fail(what, f"intrinsic must be four numbers (fx, fy, cx, cy) (got {intrinsic!r})")
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx > 0 and fy > 0):
        fail(what, f"intrinsic must be finite with fx, fy > 0 (got {intrinsic!r})")
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
    G = len(off) - 1
    if G > MAX_FRAGMENTS:
        fail(what, f"a call holds at most {MAX_FRAGMENTS} fragments (got {G})")
    if max(b - a for a, b in zip(off, off[1:])) > MAX_FRAMES:
        fail(what, f"a fragment holds at most {MAX_FRAMES} frames (got {max(b - a for a, b in zip(off, off[1:]))})")
    vl = positive_finite(what, "voxel_length", voxel_length, numeric=True)
    trunc = positive_finite(what, "sdf_trunc", sdf_trunc, numeric=True)
    scale = positive_finite(what, "depth_scale", depth_scale, numeric=True)
    far = positive_finite(what, "depth_trunc", depth_trunc, allow_inf=True, numeric=True)
    stride = int(depth_sampling_stride) if isinstance(depth_sampling_stride, (int, np.integer)) else 0
    if stride < 1:
        fail(what, f"depth_sampling_stride must be an integer >= 1 (got {depth_sampling_stride!r})")
    units_cap = int(max_units) if isinstance(max_units, (int, np.integer)) else 0
    if not 1 <= units_cap <= MAX_UNITS:
        fail(what, f"max_units must be an integer in 1..{MAX_UNITS} (got {max_units!r})")
    P = np.ascontiguousarray(poses.detach().cpu().numpy())
    if not np.isfinite(P).all():
        fail(what, "`poses` must be finite")
    try:
        Pinv = np.linalg.inv(P)
    except np.linalg.LinAlgError:
        fail(what, "`poses` must be invertible")
    require_device(depth, "depth", what)
    dev = depth.device

    points_off = torch.zeros(G + 1, device=dev, dtype=torch.int32)
    if F == 0:
        return _nothing(points_off, return_volume, colored, mesh)

    D = depth.contiguous()
    u16 = 1 if depth.dtype == torch.uint16 else 0
    both = torch.from_numpy(np.stack([P, Pinv])).pin_memory().to(dev, non_blocking=True)      # [2,F,4,4] fp64, no synchronisation
    dev_off, _ = device_offsets(off, F, dev, what, allow_empty=True, checked=True)
    h, st = handle_and_stream(D)
    shared = (D.data_ptr(), u16)
    camera = (G, F, H, W, fx, fy, cx, cy, vl, trunc, scale, far)

    keys = torch.empty((units_cap, 3), device=dev, dtype=torch.int32)
    birth = torch.empty(units_cap, device=dev, dtype=torch.int32)
    unit_off = torch.empty(G + 1, device=dev, dtype=torch.int32)
    n = C.c_longlong(0)
    h.call("gmf_tsdf_allocate", *shared, both[0].data_ptr(), dev_off.data_ptr(), *camera, stride, units_cap, keys.data_ptr(),
           birth.data_ptr(), unit_off.data_ptr(), C.byref(n), st)
    U = int(n.value)
    keys, birth = keys[:U].clone(), birth[:U].clone()
    if U == 0:
        return _nothing(points_off, return_volume, colored, mesh)
    tsdf = torch.empty((U, 16, 16, 16), device=dev, dtype=torch.float32)
    weight = torch.empty((U, 16, 16, 16), device=dev, dtype=torch.float32)
    units = (keys.data_ptr(), unit_off.data_ptr(), birth.data_ptr(), U, tsdf.data_ptr(), weight.data_ptr())
    volume = (keys.data_ptr(), unit_off.data_ptr(), G, U, tsdf.data_ptr(), weight.data_ptr())
    if not colored:
        h.call("gmf_tsdf_integrate", *shared, both[1].data_ptr(), dev_off.data_ptr(), *camera, *units, st)
        if mesh:
            meshes = _extract_mesh(h, st, keys, unit_off, G, tsdf, weight, None, vl)
            return (meshes, (keys, unit_off, birth, tsdf, weight)) if return_volume else meshes
        h.call("gmf_tsdf_extract", *volume, vl, None, 0, points_off.data_ptr(), C.byref(n), st)
        M = int(n.value)
        pts = torch.empty((M, 3), device=dev, dtype=torch.float32)
        if M:
            h.call("gmf_tsdf_extract", *volume, vl, pts.data_ptr(), M, points_off.data_ptr(), None, st)
        return (pts, points_off) + ((keys, unit_off, birth, tsdf, weight) if return_volume else ())
    Cf = color.contiguous()
    cvol = torch.empty((U, 16, 16, 16, 3), device=dev, dtype=torch.float32)
    h.call("gmf_tsdf_integrate_color", *shared, Cf.data_ptr(), both[1].data_ptr(), dev_off.data_ptr(), *camera, *units, cvol.data_ptr(), st)
    if mesh:
        meshes = _extract_mesh(h, st, keys, unit_off, G, tsdf, weight, cvol, vl)
        return (meshes, (keys, unit_off, birth, tsdf, weight, cvol)) if return_volume else meshes
    h.call("gmf_tsdf_extract_color", *volume, cvol.data_ptr(), vl, None, None, 0, points_off.data_ptr(), C.byref(n), st)
    M = int(n.value)
    pts = torch.empty((M, 3), device=dev, dtype=torch.float32)
    cols = torch.empty((M, 3), device=dev, dtype=torch.float32)
    if M:
        h.call("gmf_tsdf_extract_color", *volume, cvol.data_ptr(), vl, pts.data_ptr(), cols.data_ptr(), M, points_off.data_ptr(), None, st)
    return (pts, points_off) + ((keys, unit_off, birth, tsdf, weight) if return_volume else ()) + (cols,) + (
        (cvol,) if return_volume else ())
