"""FPFH descriptors on the device: the voxel grids, normals and FPFH features the reference computes with open3d (and
MinkowskiEngine's quantiser) on the CPU before matching (GMF_DeepGlobalRegistration/*/core/deep_global_registration.py:143-193;
GMF_PointDSC/misc/cal_fpfh.py:202-215, datasets/ThreeDMatch.py:104-117).  Kernels: csrc/pointcloud_kernels.hip.

Every stage is batched over ragged clouds given by `offsets` (B + 1 row offsets, a list or an int32 device tensor); a neighbour
never crosses a cloud boundary.  The search, normals and FPFH make no host synchronisation and can be captured into a graph for
a fixed row count; so do the colour gradients of coloured ICP (solvers.py).  The voxel grids read back one count per call (their output size).  Differences from open3d: INTEGRATION.md,
"Descriptors"."""
from __future__ import annotations

import ctypes

import torch

from ._args import check_offsets, check_rows, device_offsets, fail, int_in_range, positive_finite, require_device, same_device
from ._util import handle_and_stream

MAX_NN = 256      # the search keeps at most this many neighbours per row


def _check_cloud(points, offsets, what):
    check_rows(what, "points", points, 2, 3, non_empty=True)
    n = points.shape[0]
    return n, [0, n] if offsets is None else check_offsets(what, "offsets", offsets, n)


def _radius_and_nn(what, radius, max_nn):
    return positive_finite(what, "radius", radius, rule="> 0 and finite"), int_in_range(what, "max_nn", max_nn, 1, MAX_NN)


def _prepare(points, offsets, what):
    n, off = _check_cloud(points, offsets, what)
    require_device(points, "points", what)
    dev_off, _ = device_offsets(off, n, points.device, what, checked=True)
    return points.contiguous(), dev_off, dev_off.numel() - 1, n


def radius_knn_batched(points, offsets, radius, max_nn):
    """open3d's hybrid search over ragged clouds: for every row, up to `max_nn` rows of its cloud with d^2 < radius^2, itself
    included, the smallest by the key (d^2, row).  d^2 is fp64 from the fp32 coordinates, (dx dx + dy dy) + dz dz, every
    operation rounded on its own; a row at exactly `radius` is outside.

    points [sum N,3] float32 on the device, offsets B + 1 ints (or an int32 device tensor; None: one cloud).
    Returns idx [sum N, max_nn] int32 (row within the cloud, -1 padding), d2 [sum N, max_nn] float64 (0 padding) and
    count [sum N] int32, each row sorted by key."""
    what = "radius_knn_batched"
    r, m = _radius_and_nn(what, radius, max_nn)
    P, off, B, n = _prepare(points, offsets, what)
    dev = P.device
    idx = torch.empty((n, m), device=dev, dtype=torch.int32)
    d2 = torch.empty((n, m), device=dev, dtype=torch.float64)
    count = torch.empty(n, device=dev, dtype=torch.int32)
    h, st = handle_and_stream(P)
    h.call("gmf_radius_knn", P.data_ptr(), off.data_ptr(), B, n, r, m, idx.data_ptr(), d2.data_ptr(), count.data_ptr(), st)
    return idx, d2, count


def estimate_normals_batched(points, offsets, radius, max_nn=30):
    """open3d estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) without prior normals, over ragged clouds: over the
    neighbour set of radius_knn_batched, with >= 3 neighbours the eigenvector of the smallest eigenvalue of the fp64 covariance
    (open3d's FastEigen3x3, whose sign is kept: open3d does not orient these normals), else (0, 0, 1).  -> [sum N,3] float32."""
    what = "estimate_normals_batched"
    r, m = _radius_and_nn(what, radius, max_nn)
    P, off, B, n = _prepare(points, offsets, what)
    normals = torch.empty((n, 3), device=P.device, dtype=torch.float32)
    h, st = handle_and_stream(P)
    h.call("gmf_estimate_normals", P.data_ptr(), off.data_ptr(), B, n, r, m, normals.data_ptr(), st)
    return normals


def color_intensity(what, name, colors, rows_shape):
    """One float32 intensity per row from `colors`: float32 of shape rows_shape + (3,) (colours in 0..1, as
    `tsdf_fragments_colored` returns them) reduced elementwise to fp32(((r + g) + b) / 3) evaluated in fp64, or of shape
    rows_shape, taken as the intensity itself.  -> a flat contiguous tensor."""
    shape = tuple(rows_shape)
    if not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32 or tuple(colors.shape) not in (shape + (3,), shape):
        fail(what, f"{name} must be a float32 tensor of shape {shape + (3,)} (colours) or {shape} (intensities), one per row")
    if tuple(colors.shape) == shape:
        return colors.reshape(-1).contiguous()
    c = colors.reshape(-1, 3).double()
    return (((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0).float()


def color_gradients_batched(points, normals, colors, offsets, radius, max_nn=30):
    """open3d 0.9's InitializePointCloudForColoredICP(KDTreeSearchParamHybrid(radius, max_nn)) over ragged clouds: the colour
    gradient of every row in its tangent plane, over the neighbour list of radius_knn_batched.

    points [sum N,3], normals [sum N,3] (used as given: negating any of them changes no output bit), colors [sum N,3] in 0..1
    (reduced to the intensity fp32(((r + g) + b) / 3), evaluated in fp64) or [sum N] (the intensity itself), all float32.
    A row whose list holds fewer than 4 entries gets 0.  Otherwise the first entry is skipped, as open3d skips it (the row
    itself, unless an earlier row coincides with it), and over the others in list order, in fp64: e = v_a - v,
    d = e - (e . n) n, A = sum d d^T + (count - 1)^2 n n^T, b = sum d (I_a - I); A g = b by 3 x 3 LDL^T without pivoting, where
    a pivot d_k is accepted when it is finite and d_k > 2^-40 A_kk.  A rejected pivot or a non-finite component gives g = 0
    (open3d applies whatever ldlt() returns).  -> [sum N,3] float32.  No host synchronisation."""
    what = "color_gradients_batched"
    r, m = _radius_and_nn(what, radius, max_nn)
    n0, _ = _check_cloud(points, offsets, what)
    if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or tuple(normals.shape) != (n0, 3):
        fail(what, f"normals must be a float32 [{n0},3] tensor, one row per point")
    inten = color_intensity(what, "colors", colors, (n0,))
    P, off, B, n = _prepare(points, offsets, what)
    same_device(what, points=P, normals=normals, colors=inten)
    Nn = normals.contiguous()
    grad = torch.empty((n, 3), device=P.device, dtype=torch.float32)
    h, st = handle_and_stream(P)
    h.call("gmf_color_gradients", P.data_ptr(), Nn.data_ptr(), inten.data_ptr(), off.data_ptr(), B, n, r, m, grad.data_ptr(), st)
    return grad


def compute_fpfh_batched(points, normals, offsets, radius, max_nn=100):
    """open3d compute_fpfh_feature(KDTreeSearchParamHybrid(radius, max_nn)) over ragged clouds: the neighbour set of
    radius_knn_batched without the query row; SPFH from the fp64 pair features (phi, alpha, theta), 11 bins each; FPFH = the
    neighbours' SPFH weighted by 1 / d^2 (rows at d^2 = 0 skipped), each 11-bin block renormalised to 100, plus the row's own
    SPFH.  -> [sum N,33] float32, row-major (open3d's Feature.data is [33,N]).  Bitwise repeatable."""
    what = "compute_fpfh_batched"
    r, m = _radius_and_nn(what, radius, max_nn)
    n0, _ = _check_cloud(points, offsets, what)
    if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or tuple(normals.shape) != (n0, 3):
        fail(what, f"normals must be a float32 [{n0},3] tensor, one row per point")
    P, off, B, n = _prepare(points, offsets, what)
    require_device(normals, "normals", what)
    same_device(what, points=P, normals=normals)
    Nn = normals.contiguous()
    feats = torch.empty((n, 33), device=P.device, dtype=torch.float32)
    h, st = handle_and_stream(P)
    h.call("gmf_compute_fpfh", P.data_ptr(), Nn.data_ptr(), off.data_ptr(), B, n, r, m, feats.data_ptr(), st)
    return feats


def _voxel(points, offsets, voxel_size, what, mean):
    v = positive_finite(what, "voxel_size", voxel_size, rule="> 0 and finite")
    P, off, B, n = _prepare(points, offsets, what)
    dev = P.device
    out = torch.empty((n, 3) if mean else (n,), device=dev, dtype=torch.float32 if mean else torch.int32)
    out_off = torch.empty(B + 1, device=dev, dtype=torch.int32)
    num = ctypes.c_longlong(0)
    h, st = handle_and_stream(P)
    h.call("gmf_voxel_down_sample" if mean else "gmf_voxel_select", P.data_ptr(), off.data_ptr(), B, n, v, out.data_ptr(),
           out_off.data_ptr(), ctypes.byref(num), st)
    return out[:num.value], out_off, off


def voxel_down_sample_batched(points, offsets, voxel_size):
    """open3d voxel_down_sample over ragged clouds: per cloud the origin min(points) - voxel_size / 2, the voxel of a row
    floor((p - origin) / voxel_size), and the fp64 mean of each voxel's rows (in ascending row order) stored as float32.  The
    voxels of a cloud come in first-occurrence order (by their smallest row; open3d's order is that of a hash map).
    -> (points_down [M,3] float32, offsets_down [B+1] int32 device tensor).  One host synchronisation (M)."""
    pts, off, _ = _voxel(points, offsets, voxel_size, "voxel_down_sample_batched", True)
    return pts, off


def voxel_down_sample_colored_batched(points, colors, offsets, voxel_size):
    """`voxel_down_sample_batched` for clouds with colours: colors [sum N,3] float32.  The points, their order and the offsets
    are `voxel_down_sample_batched`'s, bit for bit; a voxel's colour is the fp64 mean of its rows' colours in ascending row
    order, stored as float32 (open3d's AccumulatedPoint).
    -> (points_down [M,3], colors_down [M,3], offsets_down [B+1] int32 device tensor).  One host synchronisation (M)."""
    what = "voxel_down_sample_colored_batched"
    v = positive_finite(what, "voxel_size", voxel_size, rule="> 0 and finite")
    n0, _ = _check_cloud(points, offsets, what)
    if not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32 or tuple(colors.shape) != (n0, 3):
        fail(what, f"colors must be a float32 [{n0},3] tensor, one row per point")
    same_device(what, points=points, colors=colors)
    P, off, B, n = _prepare(points, offsets, what)
    Cc = colors.contiguous()
    dev = P.device
    out = torch.empty((2, n, 3), device=dev, dtype=torch.float32)
    out_off = torch.empty(B + 1, device=dev, dtype=torch.int32)
    num = ctypes.c_longlong(0)
    h, st = handle_and_stream(P)
    h.call("gmf_voxel_down_sample_color", P.data_ptr(), Cc.data_ptr(), off.data_ptr(), B, n, v, out[0].data_ptr(),
           out[1].data_ptr(), out_off.data_ptr(), ctypes.byref(num), st)
    return out[0, :num.value], out[1, :num.value], out_off


def voxel_select_batched(points, offsets, voxel_size):
    """DGR's ME.utils.sparse_quantize(points / voxel_size, return_index=True) over ragged clouds: the voxel floor(p /
    voxel_size) with no offset, and of each voxel its smallest row.  -> (idx [M] int64, rows within their cloud, ascending per
    cloud; offsets_down [B+1] int32 device tensor).  One host synchronisation (M)."""
    idx, off, _ = _voxel(points, offsets, voxel_size, "voxel_select_batched", False)
    return idx.long(), off


def voxel_down_sample(points, voxel_size):
    """open3d PointCloud.voxel_down_sample for one cloud [N,3] -> [M,3] float32 (first-occurrence order)."""
    return voxel_down_sample_batched(points, None, voxel_size)[0]


def voxel_select(points, voxel_size):
    """ME.utils.sparse_quantize(points / voxel_size, return_index=True)[1] for one cloud [N,3] -> [M] int64, ascending."""
    return voxel_select_batched(points, None, voxel_size)[0]


def estimate_normals(points, radius, max_nn=30):
    """open3d estimate_normals(pcd, KDTreeSearchParamHybrid(radius, max_nn)) for one cloud [N,3] -> normals [N,3] float32."""
    return estimate_normals_batched(points, None, radius, max_nn)


def compute_fpfh_feature(points, normals, radius, max_nn=100):
    """open3d registration.compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)) for one cloud -> [N,33] float32
    (the transpose of open3d's Feature.data, as every reference call site uses it)."""
    return compute_fpfh_batched(points, normals, None, radius, max_nn)


def fpfh_descriptors(points, voxel_size, offsets=None, voxelize="mean"):
    """The reference's FPFH recipe: voxel grid -> normals (2 v, 30) -> FPFH (5 v, 100) -> nan_to_num -> f / (|f| + 1e-6).

    voxelize="mean": open3d voxel_down_sample (GMF_PointDSC/misc/cal_fpfh.py with the 3DMatch loader's normalisation);
    voxelize="select": DGR's preprocess, the smallest row of each voxel of floor(p / v) (deep_global_registration.py:143-193).
    points [N,3] float32 on the device -> (xyz_down [M,3], features [M,33]); with `offsets` (ragged clouds) ->
    (xyz_down, features, offsets_down).  The features feed nn_match / find_knn_gpu directly."""
    what = "fpfh_descriptors"
    if voxelize not in ("mean", "select"):
        fail(what, f"voxelize must be 'mean' or 'select' (got {voxelize!r})")
    v = positive_finite(what, "voxel_size", voxel_size, rule="> 0 and finite")
    n, off = _check_cloud(points, offsets, what)
    require_device(points, "points", what)
    if voxelize == "mean":
        xyz, off_d = voxel_down_sample_batched(points, off, v)
    else:
        idx, off_d, dev_off = _voxel(points, off, v, what, False)
        base = torch.repeat_interleave(dev_off[:-1].long(), (off_d[1:] - off_d[:-1]).long(), output_size=idx.shape[0])
        xyz = points[idx.long() + base]
    normals = estimate_normals_batched(xyz, off_d, 2 * v, 30)
    f = compute_fpfh_batched(xyz, normals, off_d, 5 * v, 100)
    f = torch.nan_to_num(f)
    f = f / (torch.linalg.norm(f, dim=1, keepdim=True) + 1e-6)
    return (xyz, f) if offsets is None else (xyz, f, off_d)
