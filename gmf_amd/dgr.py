"""DGR's registration pipeline on the device (reference: GMF_DeepGlobalRegistration_fcgf/core/deep_global_registration.py:87-410,
model/__init__.py): `load_model` and `DeepGlobalRegistration` with its `register()`.

Every step runs on the device: voxel_select, FCGF (`gmf_amd.fcgf.ResUNetBN2C`, both clouds in one plan), find_knn_gpu, the 6-D
inlier network (`gmf_amd.ResUNetBN2C`), GlobalRegistration or the safeguard RANSAC, and ICP.
"""
from __future__ import annotations

from collections.abc import Mapping

import numpy as np
import torch

from . import fcgf
from .features import voxel_select
from .matching import find_knn_gpu
from .registration import GlobalRegistration
from .solvers import registration_icp, registration_ransac_based_on_correspondence
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
    - inlier_feature_type 'feats' gets a 2 x feat_model_n_out wide inlier network (`inlier_in_channels`)."""

    def __init__(self, config, device=torch.device("cuda"), state=None, inlier_pe=True):
        self.config = config
        self.clip_weight_thresh = float(_get(config, "clip_weight_thresh"))
        self.device = torch.device(device)
        self.use_icp = True
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
        """:256-272 with the correspondence safeguard: RANSAC over the correspondences, ransac_n = 4, 80 000 hypotheses,
        threshold 2 voxel_size."""
        res = registration_ransac_based_on_correspondence(xyz0, xyz1, torch.stack([idx0, idx1], 1), 2 * self.voxel_size,
                                                          ransac_n=4, max_iteration=4000000, max_validation=80000)
        return res.transformation.double().cpu().numpy()

    def register(self, xyz0, xyz1, inlier_thr=0.0, p_image=None, q_image=None, use_corr=False, p_tokens=None, q_tokens=None):
        """:281-410.  xyz0, xyz1: [N, 3] numpy arrays or tensors.  The inlier network takes p_image / q_image [1, 3, H, W] or
        p_tokens / q_tokens [1, T, 128].  -> T [4, 4] float64 numpy (use_corr: T, xyz0[idx0], xyz1[idx1])."""
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
            T = registration_icp(xyz0, xyz1, 2 * self.voxel_size, init=torch.as_tensor(T, dtype=torch.float32)
                                 ).transformation.double().cpu().numpy()
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
