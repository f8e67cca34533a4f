"""FCGF, the feature network of DGR (reference: GMF_DeepGlobalRegistration_fcgf/model/resunet.py:419-661, ResUNetBN2C),
eval-mode and forward-only, on the coordinate engine and sparse convolutions of `sparse.py`.

The same sparse U-Net as DGR's inlier network (`gmf_amd.ResUNetBN2C`, which stays the top-level name) without its image
fusion layers, with its own ends: conv1 (Cin = 1 in DGR, k^3 up to 7^3) runs on the narrow-input kernel
(`sparse_conv_narrow`), and conv1_tr, ReLU, final and the optional row normalisation run as one launch (`sparse_head_l2`).
Kernels: csrc/sparse_kernels.hip.  The state_dict keys and shapes are the reference's.
"""
from __future__ import annotations

import torch

from .sparse import CONV1_TR, FINAL, _ResUNet, _fail, _folded_conv, resunet_trunk, sparse_conv_narrow, sparse_head_l2

NARROW_MAX_CIN = 8
HEAD_MAX_C = 64


class ResUNetBN2C(_ResUNet):
    """FCGF's ResUNetBN2C (resunet.py:654-657 on ResUNet2, :419-651), eval-mode forward on the device.

    forward(coords [M, 1 + D] int32, feats [M, in_channels] float32) -> [M, out_channels], aligned with the input rows; several
    clouds go through one call as batches of one plan (column 0 of coords), each row's features independent of the others'
    batches.  With normalize_feature each row is divided by (its L2 norm + 1e-8).  `narrow_conv1` (default True) runs conv1 on
    the narrow-input kernel when in_channels <= 8; False runs it on the generic `sparse_conv` (for A/B runs)."""

    _MODULE = "fcgf."

    def __init__(self, in_channels=3, out_channels=32, bn_momentum=0.1, conv1_kernel_size=3, normalize_feature=False, D=3):
        super().__init__(in_channels, out_channels, conv1_kernel_size, normalize_feature, D)
        if not (1 <= int(out_channels) <= HEAD_MAX_C):
            _fail(self._what, f"the fused head takes out_channels in 1..{HEAD_MAX_C} (got {out_channels})", NotImplementedError)
        self.narrow_conv1 = True
        self._build_trunk(bn_momentum)

    def forward(self, coords, feats):
        if self.training:
            raise RuntimeError(f"gmf_amd.{self._what}: only the eval-mode forward is built - call eval()")
        feats = self._check_input(coords, feats)
        with torch.no_grad():
            return self._forward(coords, feats)

    def _forward(self, coords, feats):
        L = self._weights(coords.device)
        narrow = self.narrow_conv1 and self.in_channels <= NARROW_MAX_CIN
        plan, where = self._plan(coords, conv1_needs_pairs=narrow)

        def layer(i, xa, **kw):
            if i == 0 and narrow:
                W, sc, sh = L[0]
                return sparse_conv_narrow(plan, where[0][0], 0, xa, W, scale=sc, shift=sh)
            return _folded_conv(plan, where, L, i, xa, **kw)

        t1, s1 = resunet_trunk(layer, feats)
        # :641-648: conv1_tr on ME.cat(out_s1_tr, out_s1), MEF.relu, final (+ bias), the optional normalisation
        return sparse_head_l2(plan, 0, t1, L[CONV1_TR][0], L[FINAL][0], xb=s1, bias=L[FINAL][2],
                              normalize=self.normalize_feature)


class ResUNetBN2CX(ResUNetBN2C):
    """resunet.py:660-661: the hyper-cross kernel region.  Not built: constructing it raises NotImplementedError."""
    REGION_TYPE = "HYPER_CROSS"
