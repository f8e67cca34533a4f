"""DGR's registration pipeline on the device (reference: GMF_DeepGlobalRegistration_fcgf/core/deep_global_registration.py:87-410,
model/__init__.py): `load_model` and `DeepGlobalRegistration` with its `register()`.

Every step runs on the device: voxel_select, FCGF (`gmf_amd.fcgf.ResUNetBN2C`, both clouds in one plan), find_knn_gpu, the 6-D
inlier network (`gmf_amd.ResUNetBN2C`), GlobalRegistration or the safeguard RANSAC, and ICP.

For training, the step between the data loader and the inlier network (core/trainer.py:616-699, core/correspondence.py:14-53,
util/pointcloud.py:83-96) over a collated batch: `matching_indices_batched` (the ground-truth pairs), `find_correct_correspondence`
(the labels) and `generate_inlier_input`.  Kernels: csrc/dgr_input_kernels.hip, csrc/match_kernels.hip.
"""
from __future__ import annotations

import ctypes
from collections.abc import Mapping

import numpy as np
import torch

from . import _lib, fcgf
from ._args import check_offsets, device_offsets, fail, positive_finite, require_device, same_device
from .features import voxel_select
from ._util import handle_and_stream
from .matching import _batch_offsets, _match_batched, find_knn_gpu
from .registration import GlobalRegistration
from .solvers import ransac_feature_matching_batched, registration_icp, registration_ransac_based_on_correspondence
from .sparse import ResUNetBN2C as InlierResUNetBN2C, inlier_coordinates

# model/__init__.py collects every class of simpleunet / resunet / pyramidnet; of those only FCGF's ResUNetBN2C is built
_BUILT = {"ResUNetBN2C": fcgf.ResUNetBN2C}


def load_model(name, corrs=False):
    """model/__init__.py:load_model: the class of a network by name; corrs=True returns the inlier network (the reference's
    resunet_new.ResUNetBN2C, `gmf_amd.ResUNetBN2C`) whatever the name.  A name that is not built raises NotImplementedError
    (the reference logs the options and returns None)."""
    if corrs:
        return InlierResUNetBN2C
    if name in _BUILT:
        return _BUILT[name]
    raise NotImplementedError(f"gmf_amd.dgr.load_model: {name!r} is not built; built: {', '.join(sorted(_BUILT))} (FCGF), and "
                              "with corrs=True the inlier network ResUNetBN2C")


_MISSING = object()


def _get(cfg, key, default=_MISSING):
    if isinstance(cfg, Mapping):
        v = cfg.get(key, _MISSING)
    else:
        v = getattr(cfg, key, _MISSING)
    if v is _MISSING:
        if default is _MISSING:
            raise KeyError(f"gmf_amd.dgr: the network config has no {key!r}")
        return default
    return v


def parse_network_config(cfg) -> dict:
    """The settings DeepGlobalRegistration reads from a checkpoint's `config` (:113-132), from a dict or an attribute object.
    The feat_* keys, or else the legacy model / model_n_out / conv1_kernel_size (:127-132)."""
    if _get(cfg, "feat_model", None) is not None:
        feat = (_get(cfg, "feat_model"), _get(cfg, "feat_model_n_out"), _get(cfg, "feat_conv1_kernel_size"))
    else:
        feat = (_get(cfg, "model"), _get(cfg, "model_n_out"), _get(cfg, "conv1_kernel_size"))
    return {"feat_model": feat[0], "feat_model_n_out": int(feat[1]), "feat_conv1_kernel_size": int(feat[2]),
            "bn_momentum": float(_get(cfg, "bn_momentum")), "normalize_feature": bool(_get(cfg, "normalize_feature")),
            "inlier_model": _get(cfg, "inlier_model"), "inlier_conv1_kernel_size": int(_get(cfg, "inlier_conv1_kernel_size")),
            "inlier_feature_type": _get(cfg, "inlier_feature_type"), "voxel_size": float(_get(cfg, "voxel_size")),
            "nn_max_n": int(_get(cfg, "nn_max_n"))}


def inlier_in_channels(feature_type: str, feat_n_out: int) -> int:
    """Input width of the inlier network per inlier_feature_type (:136, :236-243).  'feats' concatenates both clouds' FCGF
    features, 2 x feat_n_out wide; the reference builds that network with 1 input channel, which cannot run."""
    widths = {"ones": 1, "coords": 6, "feats": 2 * int(feat_n_out)}
    if feature_type not in widths:
        raise ValueError(f"gmf_amd.dgr: inlier_feature_type must be one of {sorted(widths)} (got {feature_type!r})")
    return widths[feature_type]


class DeepGlobalRegistration:
    """deep_global_registration.py:87-410 on the device.

    config: `weights` (the checkpoint path, read when `state` is None) and `clip_weight_thresh`.  state: the checkpoint mapping
    {'config', 'state_dict', 'state_dict_inlier'}; its `config` may be a dict or an attribute object (`parse_network_config`).
    inlier_pe: the inlier network's bottleneck position encoding (True in the fcgf tree's resunet_new.py:524).

    register(xyz0, xyz1) returns the 4 x 4 float64 pose T with T xyz0 ~ xyz1.  Deviations from the reference:
    - GlobalRegistration runs once; the reference runs the same deterministic call twice (:346, :372).
    - A non-finite pose from it falls back to the safeguard RANSAC; in the reference the second call overwrites the
      safeguard's pose with the same NaN.
    - Nothing is printed: `last_stats` holds wsum, its threshold, the branch taken ('global_registration' or 'safeguard'), the
      GlobalRegistration statistics (or None) and the correspondence count.
    - The images (or their tokens) go to the inlier network as given; inlier_thr is accepted and unused, as in the reference.
    - inlier_feature_type 'feats' gets a 2 x feat_model_n_out wide inlier network (`inlier_in_channels`).

    safeguard_method (:271-276): 'correspondence' (the default, as in the reference) or 'fcgf_feature_matching'; any other
    value makes the safeguard raise ValueError."""

    SAFEGUARD_METHODS = ("correspondence", "fcgf_feature_matching")

    def __init__(self, config, device=torch.device("cuda"), state=None, inlier_pe=True):
        self.config = config
        self.clip_weight_thresh = float(_get(config, "clip_weight_thresh"))
        self.device = torch.device(device)
        self.use_icp = True
        self.icp_search = "brute"            # registration_icp's `search`: "grid" returns the same pose (timings: DESIGN.md 4e)
        self.safeguard_method = "correspondence"
        if state is None:
            state = torch.load(_get(config, "weights"), map_location="cpu", weights_only=False)
        nc = parse_network_config(state["config"])
        self.network_config = nc
        self.voxel_size = nc["voxel_size"]
        self.inlier_feature_type = nc["inlier_feature_type"]
        FCGFModel = load_model(nc["feat_model"])
        self.fcgf_model = FCGFModel(1, nc["feat_model_n_out"], bn_momentum=nc["bn_momentum"],
                                    conv1_kernel_size=nc["feat_conv1_kernel_size"], normalize_feature=nc["normalize_feature"])
        self.fcgf_model.load_state_dict(state["state_dict"])
        self.fcgf_model = self.fcgf_model.to(self.device).eval()
        InlierModel = load_model(nc["inlier_model"], True)
        self.inlier_model = InlierModel(inlier_in_channels(self.inlier_feature_type, nc["feat_model_n_out"]), 1,
                                        bn_momentum=nc["bn_momentum"], conv1_kernel_size=nc["inlier_conv1_kernel_size"],
                                        normalize_feature=False, D=6, pe=inlier_pe)
        self.inlier_model.load_state_dict(state["state_dict_inlier"])
        self.inlier_model = self.inlier_model.to(self.device).eval()
        self.last_stats = None

    def _points(self, xyz):
        if isinstance(xyz, np.ndarray):
            xyz = torch.from_numpy(xyz)
        if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] != 3:
            raise RuntimeError("gmf_amd.DeepGlobalRegistration: a cloud must be an [N, 3] array or tensor")
        return xyz.to(self.device, torch.float32).contiguous()

    def preprocess(self, xyz):
        """:143-176: the cloud's points, one per voxel (ME.utils.sparse_quantize's pick), and their voxel coordinates
        floor(xyz / voxel_size) (computed in fp64, as the voxel selection) -> (xyz [M, 3] f32, coords [M, 3] int32)."""
        xyz = self._points(xyz)
        sel = voxel_select(xyz, self.voxel_size)
        xyz = xyz[sel]
        return xyz, torch.floor(xyz.double() / self.voxel_size).to(torch.int32)

    def features(self, c0, c1):
        """FCGF descriptors of both clouds in one call (batches 0 and 1 of one plan) -> (F0 [M0, n], F1 [M1, n])."""
        b = lambda n, v: torch.full((n, 1), v, dtype=torch.int32, device=self.device)      # noqa: E731
        coords = torch.cat([torch.cat([b(len(c0), 0), c0], 1), torch.cat([b(len(c1), 1), c1], 1)]).contiguous()
        F = self.fcgf_model(coords, torch.ones((len(coords), 1), device=self.device))
        return F[:len(c0)], F[len(c0):]

    def correspondences(self, F0, F1):
        """:194-207 -> (idx0, idx1) int64 on the device."""
        nns = find_knn_gpu(F0, F1, nn_max_n=self.network_config["nn_max_n"], knn=1, return_distance=False)
        idx1 = nns.reshape(-1).long()
        return torch.arange(len(idx1), device=self.device), idx1

    def inlier_features(self, xyz0, xyz1, F0, F1, idx0, idx1):
        """:209-245."""
        t = self.inlier_feature_type
        if t == "ones":
            return torch.ones((len(idx0), 1), device=self.device)
        if t == "feats":
            return torch.cat((F0[idx0], F1[idx1]), dim=1).contiguous()
        return torch.cat((torch.cos(xyz0[idx0]), torch.cos(xyz1[idx1])), dim=1).contiguous()

    def safeguard_registration(self, xyz0, xyz1, idx0, idx1):
        """:256-276.  'correspondence': RANSAC over the correspondences, ransac_n = 4, 80 000 hypotheses, threshold
        2 voxel_size.  'fcgf_feature_matching' (:26-54): feature-matching RANSAC, ransac_n = 4, the distance checker and the
        correspondence distance at 2 voxel_size, 80 000 proposals, 1000 validations.  idx1 is the feature-space nearest
        neighbour of every row of xyz0 (`correspondences`), so the descriptors are not needed and not matched again."""
        if self.safeguard_method not in self.SAFEGUARD_METHODS:
            raise ValueError(f"gmf_amd.DeepGlobalRegistration: safeguard_method must be one of {self.SAFEGUARD_METHODS} "
                             f"(got {self.safeguard_method!r})")
        tau = 2 * self.voxel_size
        if self.safeguard_method == "fcgf_feature_matching":
            T = ransac_feature_matching_batched(xyz0[None], xyz1[None], idx1[None], tau, ransac_n=4, checker_distance=tau,
                                                max_iteration=80000, max_validation=1000)[0]
            return T[0].double().cpu().numpy()
        res = registration_ransac_based_on_correspondence(xyz0, xyz1, torch.stack([idx0, idx1], 1), tau,
                                                          ransac_n=4, max_iteration=4000000, max_validation=80000)
        return res.transformation.double().cpu().numpy()

    def register(self, xyz0, xyz1, inlier_thr=0.0, p_image=None, q_image=None, use_corr=False, p_tokens=None, q_tokens=None):
        """:281-410.  xyz0, xyz1: [N, 3] numpy arrays or tensors.  The inlier network takes p_image / q_image [1, 3, H, W] or
        p_tokens / q_tokens [1, T, 128].  -> T [4, 4] float64 numpy (use_corr: T, xyz0[idx0], xyz1[idx1])."""
        if self.safeguard_method not in self.SAFEGUARD_METHODS:
            raise ValueError(f"gmf_amd.DeepGlobalRegistration: safeguard_method must be one of {self.SAFEGUARD_METHODS} "
                             f"(got {self.safeguard_method!r})")
        with torch.no_grad():
            xyz0, c0 = self.preprocess(xyz0)
            xyz1, c1 = self.preprocess(xyz1)
            F0, F1 = self.features(c0, c1)
            idx0, idx1 = self.correspondences(F0, F1)
            zeros = lambda c: torch.cat([torch.zeros((len(c), 1), dtype=torch.int32, device=self.device), c], 1)   # noqa: E731
            coords = inlier_coordinates(zeros(c0), zeros(c1), idx0, idx1)
            feats = self.inlier_features(xyz0, xyz1, F0, F1, idx0, idx1)
            logit = self.inlier_model(coords, feats, p_image=p_image, q_image=q_image, p_tokens=p_tokens, q_tokens=q_tokens)
            weights = logit.sigmoid()
            if self.clip_weight_thresh > 0:
                weights = torch.where(weights < self.clip_weight_thresh, torch.zeros_like(weights), weights)
            wsum = weights.sum().item()
        wsum_threshold = max(200, len(weights) * 0.05)
        stats = {"wsum": wsum, "wsum_threshold": wsum_threshold, "global_registration": None,
                 "num_correspondences": int(len(idx0))}
        T = None
        if wsum >= wsum_threshold:
            R, t, gr = GlobalRegistration(xyz0[idx0], xyz1[idx1], weights=weights.detach(), break_threshold_ratio=1e-4,
                                          quantization_size=2 * self.voxel_size, verbose=False)
            stats["global_registration"] = gr
            T = np.identity(4)
            T[0:3, 0:3] = R.double().cpu().numpy()
            T[0:3, 3] = t.double().cpu().numpy()
            if not np.isfinite(T).all():
                T = None
        stats["branch"] = "global_registration" if T is not None else "safeguard"
        if T is None:
            T = self.safeguard_registration(xyz0, xyz1, idx0, idx1)
        if self.use_icp:
            T = registration_icp(xyz0, xyz1, 2 * self.voxel_size, init=torch.as_tensor(T, dtype=torch.float32),
                                 search=self.icp_search).transformation.double().cpu().numpy()
        self.last_stats = stats
        if use_corr:
            return T, xyz0[idx0], xyz1[idx1]
        return T


def inlier_training_loss(logits, xyz0s, xyz1s, pred_pairs, is_correct, T_gt, *, clip_weight_thresh=0.05, trans_weight=1.0,
                         procrustes_loss_weight=1.0, inlier_direct_loss_weight=1.0, use_balanced_loss=False,
                         inlier_use_direct_loss=True, iter_size=1):
    """The loss of DGR's inlier-model training step (GMF_DeepGlobalRegistration_fcgf/core/trainer.py:229-270, core/loss.py,
    core/metrics.py) on the device.  logits [sum n_b] or [sum n_b, 1] (the inlier network's output, batches concatenated in
    order); xyz0s / xyz1s: per batch [N_b, 3] points; pred_pairs: per batch [n_b, 2] (index into xyz0, index into xyz1);
    is_correct [sum n_b] 0 / 1; T_gt [B, 4, 4].

    sigmoid, the clip (weights <= clip_weight_thresh -> 0, without an in-place write), one batched weighted Procrustes over the
    pairs of every batch (eps = fp32 eps, the gradient flows to the weights), rotation error acos(clamp((tr(R^T R_gt) - 1) / 2,
    -0.999, 0.999)) and translation error |t - t_gt|, the mean of rot + trans_weight trans over the batches with ws > 10 (ws the
    sum of a batch's clipped weights), plus inlier_direct_loss_weight x BCE-with-logits (UnbalancedLoss, or BalancedLoss: the
    mean over the two labels present) / iter_size.  Returns (loss, {"rot_error", "trans_error", "ws", "valid"}).  No batch valid:
    the loss is not finite (the reference then skips the step); nothing raises."""
    from .registration import weighted_procrustes_batched
    logits = logits.reshape(-1)
    weights = logits.sigmoid()
    if clip_weight_thresh > 0:
        weights = torch.where(weights > clip_weight_thresh, weights, torch.zeros_like(weights))
    lens = [int(p.shape[0]) for p in pred_pairs]
    if sum(lens) != logits.numel():
        raise RuntimeError(f"gmf_amd.inlier_training_loss: {logits.numel()} logits for {sum(lens)} pairs")
    X = torch.cat([x0[p[:, 0].long()] for x0, p in zip(xyz0s, pred_pairs)]).float()
    Y = torch.cat([x1[p[:, 1].long()] for x1, p in zip(xyz1s, pred_pairs)]).float()
    offsets = [0]
    for n in lens:
        offsets.append(offsets[-1] + n)
    R, t = weighted_procrustes_batched(X, Y, weights, offsets, float(np.finfo(np.float32).eps))
    seg = torch.repeat_interleave(torch.arange(len(lens), device=logits.device), torch.tensor(lens, device=logits.device))
    ws = torch.zeros(len(lens), device=logits.device, dtype=weights.dtype).index_add_(0, seg, weights.detach())
    T_gt = T_gt.to(logits.device).float()
    R_gt, t_gt = T_gt[:, :3, :3], T_gt[:, :3, 3]
    rot_error = torch.acos(torch.clamp(((R.reshape(-1, 9) * R_gt.reshape(-1, 9)).sum(1) - 1) / 2, min=-0.999, max=0.999))
    trans_error = torch.norm(t - t_gt, p=2, dim=1)
    individual = rot_error + trans_weight * trans_error
    valid = ws > 10
    # individual[valid].mean() without the host read of a boolean index: an empty selection gives 0 / 0 = NaN as mean() does
    loss = procrustes_loss_weight * torch.where(valid, individual, torch.zeros_like(individual)).sum() / valid.sum()
    if inlier_use_direct_loss:
        target = torch.as_tensor(is_correct, device=logits.device).reshape(-1).float()
        bce = torch.nn.functional.binary_cross_entropy_with_logits
        if use_balanced_loss:
            crit = logits.new_zeros(())
            for lab in (0, 1):
                mask = target == lab
                if bool(mask.any()):
                    crit = crit + bce(logits[mask], target[mask]) / 2
        else:
            crit = bce(logits, target)
        loss = loss + inlier_direct_loss_weight * crit / iter_size
    return loss, {"rot_error": rot_error, "trans_error": trans_error, "ws": ws, "valid": valid}


# ---- the batched input of the inlier network -----------------------------------------------------------------------------------

INLIER_FEATURE_TYPES = ("ones", "feats", "coords")      # gmf_inlier_input's feat_type 0, 1, 2


def matching_indices_batched(xyz0, off0, xyz1, off1, T, radius):
    """The ground-truth pairs of B registration problems on the device: get_matching_indices(source, target, trans,
    search_voxel_size, K=None) (util/pointcloud.py:83-96) for every pair of a batch, by brute force.

    xyz0 [sum N0, 3], xyz1 [sum N1, 3] float32 on the device; off0 / off1: B + 1 ascending row offsets (a sequence, or an int32
    device tensor); T [B, 4, 4] (used as float64) with T xyz0 ~ xyz1; radius > 0.
    Returns (pairs [K, 2] int64, pair_offsets [B + 1] int64), both on the device: pair b owns pairs[pair_offsets[b] :
    pair_offsets[b + 1]], rows (i, j) local to the pair.

    (i, j) is in when d2 < radius * radius (the product in float64; a pair at exactly `radius` is outside), with, in float64
    from the float32 coordinates and every operation rounded on its own,
        p  = ((T[b, r, 0] * x + T[b, r, 1] * y) + T[b, r, 2] * z) + T[b, r, 3]          for r = 0, 1, 2
        d2 = ((p0 - q0) * (p0 - q0) + (p1 - q1) * (p1 - q1)) + (p2 - q2) * (p2 - q2)
    Order: by i, then by j ascending.  open3d's search_radius_vector_3d orders each row's neighbours by distance; the labels only
    use set membership, so this order is a definition of this function, not parity.  One host read (K)."""
    what = "matching_indices_batched"
    for name, x in (("xyz0", xyz0), ("xyz1", xyz1)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3 or x.shape[0] == 0:
            fail(what, f"`{name}` must be a non-empty float32 [rows, 3] tensor")
    o0 = check_offsets(what, "off0", off0, xyz0.shape[0], allow_empty=True)
    o1 = check_offsets(what, "off1", off1, xyz1.shape[0], allow_empty=True)
    B = (o0.numel() if isinstance(o0, torch.Tensor) else len(o0)) - 1
    if (o1.numel() if isinstance(o1, torch.Tensor) else len(o1)) - 1 != B:
        fail(what, "off0 and off1 describe different numbers of pairs")
    T = torch.as_tensor(T)
    if tuple(T.shape) != (B, 4, 4):
        fail(what, f"T must be [{B}, 4, 4] (got {tuple(T.shape)})")
    r = positive_finite(what, "radius", radius, rule="> 0 and finite")
    require_device(xyz0, "xyz0", what)
    same_device(what, xyz0=xyz0, xyz1=xyz1)
    dev = xyz0.device
    xyz0, xyz1 = xyz0.contiguous(), xyz1.contiguous()
    d0 = device_offsets(o0, xyz0.shape[0], dev, what, allow_empty=True, checked=True)[0]
    d1 = device_offsets(o1, xyz1.shape[0], dev, what, allow_empty=True, checked=True)[0]
    Td = T.to(dev, torch.float64).contiguous()
    n0, n1 = xyz0.shape[0], xyz1.shape[0]
    row_start = torch.empty(n0 + 1, device=dev, dtype=torch.int64)
    pair_offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    num = ctypes.c_longlong(0)
    h, st = handle_and_stream(xyz0)
    h.call("gmf_matching_indices_count", xyz0.data_ptr(), d0.data_ptr(), xyz1.data_ptr(), d1.data_ptr(), B, n0, n1, Td.data_ptr(), r,
           row_start.data_ptr(), pair_offsets.data_ptr(), ctypes.byref(num), st)
    pairs = torch.empty((num.value, 2), device=dev, dtype=torch.int64)
    if num.value:
        h.call("gmf_matching_indices_fill", xyz0.data_ptr(), d0.data_ptr(), xyz1.data_ptr(), d1.data_ptr(), B, n0, n1, Td.data_ptr(),
               r, row_start.data_ptr(), pairs.data_ptr(), st)
    return pairs, pair_offsets


def _is_packed(pos_pairs):
    return (isinstance(pos_pairs, tuple) and len(pos_pairs) == 2 and isinstance(pos_pairs[0], torch.Tensor)
            and pos_pairs[0].dim() == 2 and isinstance(pos_pairs[1], torch.Tensor) and pos_pairs[1].dim() == 1)


def _num_pos(pos_pairs):
    return pos_pairs[1].numel() - 1 if _is_packed(pos_pairs) else len(pos_pairs)


def _label_seeds(n_pairs, hash_seed, len_batch, what):
    """The asserts of core/correspondence.py:30-32 as RuntimeError, and each pair's hash seed."""
    if hash_seed is None:
        if len_batch is None or len(len_batch) != n_pairs:
            fail(what, "without hash_seed, len_batch must have one (N0, N1) per pair")
        return [max(int(a), int(b)) for a, b in len_batch]
    return [int(hash_seed)] * n_pairs


def _positive_keys(pos_pairs, seeds, dev, what):
    """-> (keys [K] int64 sorted inside each pair's range, pos_off [B + 1] int64, seeds [B] int64), all on `dev`; no host read."""
    B = len(seeds)
    seeds_d = torch.tensor(seeds, dtype=torch.int64, device=dev)
    if _is_packed(pos_pairs):
        pos = pos_pairs[0].to(dev, torch.int64)
        pos_off = pos_pairs[1].to(dev, torch.int64).contiguous()
        seg = torch.searchsorted(pos_off[1:].contiguous(), torch.arange(pos.shape[0], device=dev), right=True)
    else:
        parts = []
        for p in pos_pairs:
            p = torch.as_tensor(p)
            if p.dtype.is_floating_point or p.dtype == torch.bool or (p.numel() and (p.dim() != 2 or p.shape[1] != 2)):
                fail(what, "every pos_pairs entry must be an integer [K, 2] tensor")
            parts.append(p.reshape(-1, 2).to(dev, torch.int64))
        counts = [int(p.shape[0]) for p in parts]
        pos = torch.cat(parts) if parts else torch.empty((0, 2), dtype=torch.int64, device=dev)
        pos_off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), device=dev)
        seg = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(counts, device=dev), output_size=pos.shape[0])
    if pos.dim() != 2 or pos.shape[1] != 2:
        fail(what, "the packed pos_pairs must be [K, 2]")
    keys = pos[:, 0] + pos[:, 1] * seeds_d[seg.clamp(max=B - 1)]          # core/correspondence.py:14-26, int64
    # sorted inside each pair's range: by key, then stably by pair (the ranges are contiguous already, so they keep their place)
    keys, order = torch.sort(keys, stable=True)
    keys = keys[torch.sort(seg[order], stable=True)[1]]
    return keys.contiguous(), pos_off, seeds_d


def find_correct_correspondence(pos_pairs, pred_pairs, hash_seed=None, len_batch=None):
    """DGR find_correct_correspondence (core/correspondence.py:29-53) on the device: for every predicted pair whether it is among
    its batch entry's positive pairs -> bool tensor [sum n_b] on the device (the reference returns a numpy array).

    pred_pairs: per batch entry an integer [n_b, 2] device tensor.  pos_pairs: per entry an integer [K_b, 2] tensor, on the CPU or
    the device, or the packed (pairs, pair_offsets) of `matching_indices_batched`.  The test is the reference's: membership of the
    key p[:, 0] + p[:, 1] * seed (int64) with seed = max(N0, N1) of the entry (len_batch) unless hash_seed is given - a seed that
    is too small collides exactly as the reference does.  Its asserts are RuntimeError here.  The positive keys are sorted with
    torch.sort and looked up by one kernel launch for the batch; no host read."""
    what = "find_correct_correspondence"
    B = len(pred_pairs)
    if _num_pos(pos_pairs) != B:
        fail(what, f"{_num_pos(pos_pairs)} pos_pairs entries for {B} pred_pairs entries")
    seeds = _label_seeds(B, hash_seed, len_batch, what)
    if B == 0:
        fail(what, "empty batch")
    for p in pred_pairs:
        if not isinstance(p, torch.Tensor) or p.dim() != 2 or p.shape[1] != 2 or p.dtype.is_floating_point:
            fail(what, "every pred_pairs entry must be an integer [n, 2] tensor")
        require_device(p, "pred_pairs", what)
    dev = pred_pairs[0].device
    pred = torch.cat([p.to(torch.int64) for p in pred_pairs]).contiguous()
    M = pred.shape[0]
    labels = torch.empty(M, device=dev, dtype=torch.uint8)
    if M == 0:
        return labels.bool()
    off = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in pred_pairs])])
    off_d = torch.tensor(off.astype(np.int32), device=dev)
    keys, pos_off, seeds_d = _positive_keys(pos_pairs, seeds, dev, what)
    h, st = handle_and_stream(pred)
    h.call("gmf_inlier_input", None, pred.data_ptr(), off_d.data_ptr(), None, B, M, None, None, None, None, 0, None, None, 0, None,
           keys.data_ptr(), pos_off.data_ptr(), seeds_d.data_ptr(), labels.data_ptr(), st)
    return labels.bool()


def _packed_points(xyz, n_rows, name, what):
    if isinstance(xyz, (list, tuple)):
        xyz = torch.cat([torch.as_tensor(x) for x in xyz], 0)
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] != n_rows:
        fail(what, f"`{name}` must hold {n_rows} points [*, 3] (a tensor, or a list with one tensor per pair)")
    return xyz


def generate_inlier_input(feat_model, xyz0, xyz1, iC0, iC1, iF0, iF1, len_batch, pos_pairs, *, inlier_feature_type, nn_max_n=-1,
                          knn=1):
    """WeightedProcrustesTrainer.generate_inlier_input (core/trainer.py:644-678) on the device.

    feat_model: the FCGF network (`gmf_amd.fcgf.ResUNetBN2C`, in eval mode); iC0 / iC1 [sum N, 4] integer rows (batch, x, y, z) of
    the B source / target clouds, iF0 / iF1 their input features; len_batch: B entries (N0, N1); xyz0 / xyz1: the points, one
    tensor per pair or packed (read for 'coords' only); pos_pairs as `find_correct_correspondence` takes them, or None.
    Returns (reg_coords [M, 7] int32, reg_feats [M, c] float32, pred_pairs, is_correct), all on the device: the inlier network's
    input rows cat(iC0[ind0], iC1[ind1, 1:]) and features over the predicted pairs of the batch (M = sum N0), the per-pair
    [N0, 2] int64 pairs of `find_pairs`, and the labels (None when pos_pairs is None) - what `train.resunet_train` and
    `inlier_training_loss` take.  inlier_feature_type: 'ones' (c = 1), 'feats' (both descriptors, c = 2 x the FCGF width) or
    'coords' (the cos of the two points, c = 6; evaluated in float64 and rounded to float32, within an ulp of torch.cos); 'counts'
    and anything else raise ValueError, as the reference does.  FCGF runs under no_grad, one call per side with all B clouds in
    one plan; then three launches match the batch and one writes rows, features, pairs and labels."""
    what = "generate_inlier_input"
    if inlier_feature_type not in INLIER_FEATURE_TYPES:
        raise ValueError("Inlier feature type not defined")
    if knn != 1:
        fail(what, "GMF-DGR only uses knn = 1 (deep_global_registration.py:300)", NotImplementedError)
    for name, c in (("iC0", iC0), ("iC1", iC1)):
        if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 4 or c.dtype.is_floating_point:
            fail(what, f"`{name}` must be an integer [N, 4] tensor (batch, x, y, z)")
    off0, off1 = _batch_offsets(len_batch, iC0.shape[0], iC1.shape[0], what)
    B = len(off0) - 1
    if pos_pairs is not None:
        if _num_pos(pos_pairs) != B:
            fail(what, f"{_num_pos(pos_pairs)} pos_pairs entries for {B} pairs")
        seeds = _label_seeds(B, None, len_batch, what)
    ftype = INLIER_FEATURE_TYPES.index(inlier_feature_type)
    if ftype == 2:
        xyz0 = _packed_points(xyz0, iC0.shape[0], "xyz0", what)
        xyz1 = _packed_points(xyz1, iC1.shape[0], "xyz1", what)
    dev = next(feat_model.parameters()).device
    require_device(dev, "feat_model", what)
    iC0 = iC0.to(dev, torch.int32).contiguous()
    iC1 = iC1.to(dev, torch.int32).contiguous()
    with torch.no_grad():
        oF0 = feat_model(iC0, iF0.to(dev))
        oF1 = feat_model(iC1, iF1.to(dev))
        idx32, _, _, _ = _match_batched(oF0, oF1, len_batch, 1 if nn_max_n > 1 else 2, False, what)
    M = off0[-1]
    a0 = a1 = None
    width = 1
    if ftype == 1:
        a0, a1, width = oF0.contiguous(), oF1.contiguous(), 2 * oF0.shape[1]
        if oF0.shape[1] > 64:
            fail(what, f"'feats' takes descriptors up to 64 wide (got {oF0.shape[1]})", NotImplementedError)
    elif ftype == 2:
        a0, a1, width = xyz0.to(dev, torch.float32).contiguous(), xyz1.to(dev, torch.float32).contiguous(), 6
    reg_coords = torch.empty((M, 7), device=dev, dtype=torch.int32)
    reg_feats = torch.empty((M, width), device=dev, dtype=torch.float32)
    pred = torch.empty((M, 2), device=dev, dtype=torch.int64)
    labels = keys = pos_off = seeds_d = None
    if pos_pairs is not None:
        labels = torch.empty(M, device=dev, dtype=torch.uint8)
        keys, pos_off, seeds_d = _positive_keys(pos_pairs, seeds, dev, what)
    if M:
        p = _lib.ptr
        d0 = device_offsets(off0, off0[-1], dev, what, allow_empty=True, checked=True)[0]
        d1 = device_offsets(off1, off1[-1], dev, what, allow_empty=True, checked=True)[0]
        h, st = handle_and_stream(idx32)
        h.call("gmf_inlier_input", idx32.data_ptr(), None, d0.data_ptr(), d1.data_ptr(), B, M, pred.data_ptr(), iC0.data_ptr(),
               iC1.data_ptr(), reg_coords.data_ptr(), ftype, p(a0), p(a1), oF0.shape[1] if ftype == 1 else 0, reg_feats.data_ptr(),
               p(keys), p(pos_off), p(seeds_d), p(labels), st)
    pred_pairs = [pred[a:b] for a, b in zip(off0, off0[1:])]
    return reg_coords, reg_feats, pred_pairs, None if labels is None else labels.bool()
