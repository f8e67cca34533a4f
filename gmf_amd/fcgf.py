"""FCGF, the feature network of DGR (reference: GMF_DeepGlobalRegistration_fcgf/model/resunet.py:419-661, ResUNetBN2C),
eval-mode and forward-only, on the coordinate engine and sparse convolutions of `sparse.py`.

The same sparse U-Net as DGR's inlier network (`gmf_amd.ResUNetBN2C`, which stays the top-level name) without its image
fusion layers, with its own ends: conv1 (Cin = 1 in DGR, k^3 up to 7^3) runs on the narrow-input kernel
(`sparse_conv_narrow`), and conv1_tr, ReLU, final and the optional row normalisation run as one launch (`sparse_head_l2`).
Kernels: csrc/sparse_kernels.hip.  The state_dict keys and shapes are the reference's.
"""
from __future__ import annotations

import torch
from torch import nn

from ._util import WeightWatcher
from .sparse import (MAX_D, MAX_KERNEL_VOLUME, SparsePlan, _NET_MAPS, _BasicBlockBN, _MinkowskiBatchNorm,
                     _MinkowskiConvolution, _f32_dev, check_coords, kernel_volume, layer_nsplit, pack_resunet, sparse_conv,
                     sparse_conv_narrow, sparse_head_l2)

NARROW_MAX_CIN = 8
HEAD_MAX_C = 64


class ResUNetBN2C(nn.Module):
    """FCGF's ResUNetBN2C (resunet.py:654-657 on ResUNet2, :419-651), eval-mode forward on the device.

    forward(coords [M, 1 + D] int32, feats [M, in_channels] float32) -> [M, out_channels], aligned with the input rows; several
    clouds go through one call as batches of one plan (column 0 of coords), each row's features independent of the others'
    batches.  With normalize_feature each row is divided by (its L2 norm + 1e-8).  `narrow_conv1` (default True) runs conv1 on
    the narrow-input kernel when in_channels <= 8; False runs it on the generic `sparse_conv` (for A/B runs)."""

    CHANNELS = [None, 32, 64, 128, 256]
    TR_CHANNELS = [None, 64, 64, 64, 128]
    REGION_TYPE = "HYPER_CUBE"

    def __init__(self, in_channels=3, out_channels=32, bn_momentum=0.1, conv1_kernel_size=3, normalize_feature=False, D=3):
        super().__init__()
        what = f"gmf_amd.fcgf.{type(self).__name__}"
        if self.REGION_TYPE != "HYPER_CUBE":
            raise NotImplementedError(f"{what}: only the hypercube kernel region is built (got {self.REGION_TYPE})")
        if not (1 <= int(D) <= MAX_D):
            raise ValueError(f"{what}: D must be in 1..{MAX_D} (got {D})")
        for k in (conv1_kernel_size, 3):
            if k % 2 == 0 or k < 1:
                raise ValueError(f"{what}: kernel size {k} must be odd")
            if kernel_volume(k, D) > MAX_KERNEL_VOLUME:
                raise NotImplementedError(f"{what}: kernel volume {k}^{D} exceeds {MAX_KERNEL_VOLUME}")
        if not (1 <= int(out_channels) <= HEAD_MAX_C):
            raise NotImplementedError(f"{what}: the fused head takes out_channels in 1..{HEAD_MAX_C} (got {out_channels})")
        CH, TR = self.CHANNELS, self.TR_CHANNELS
        self.D, self.conv1_kernel_size = int(D), int(conv1_kernel_size)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.normalize_feature = bool(normalize_feature)
        self.narrow_conv1 = True
        m = bn_momentum
        self.conv1 = _MinkowskiConvolution(in_channels, CH[1], conv1_kernel_size, D)
        self.norm1 = _MinkowskiBatchNorm(CH[1], m)
        self.block1 = _BasicBlockBN(CH[1], m, D)
        self.conv2 = _MinkowskiConvolution(CH[1], CH[2], 3, D)
        self.norm2 = _MinkowskiBatchNorm(CH[2], m)
        self.block2 = _BasicBlockBN(CH[2], m, D)
        self.conv3 = _MinkowskiConvolution(CH[2], CH[3], 3, D)
        self.norm3 = _MinkowskiBatchNorm(CH[3], m)
        self.block3 = _BasicBlockBN(CH[3], m, D)
        self.conv4 = _MinkowskiConvolution(CH[3], CH[4], 3, D)
        self.norm4 = _MinkowskiBatchNorm(CH[4], m)
        self.block4 = _BasicBlockBN(CH[4], m, D)
        self.conv4_tr = _MinkowskiConvolution(CH[4], TR[4], 3, D)
        self.norm4_tr = _MinkowskiBatchNorm(TR[4], m)
        self.block4_tr = _BasicBlockBN(TR[4], m, D)
        self.conv3_tr = _MinkowskiConvolution(CH[3] + TR[4], TR[3], 3, D)
        self.norm3_tr = _MinkowskiBatchNorm(TR[3], m)
        self.block3_tr = _BasicBlockBN(TR[3], m, D)
        self.conv2_tr = _MinkowskiConvolution(CH[2] + TR[3], TR[2], 3, D)
        self.norm2_tr = _MinkowskiBatchNorm(TR[2], m)
        self.block2_tr = _BasicBlockBN(TR[2], m, D)
        self.conv1_tr = _MinkowskiConvolution(CH[1] + TR[2], TR[1], 1, D)
        self.final = _MinkowskiConvolution(TR[1], out_channels, 1, D, bias=True)
        self._packed, self._packed_version = None, None
        self._watch = WeightWatcher(self)

    # -- weights --------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._watch.invalidate()
        self._packed = None
        return out

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        if hasattr(self, "_watch"):
            self._watch.invalidate()
        return out

    def _weights(self, device):
        """The 23 convolutions packed with their BatchNorms folded, rebuilt when a weight changes."""
        key = (self._watch.version(), torch.device(device))
        if self._packed is None or self._packed_version != key:
            self._packed, self._packed_version = pack_resunet(self.state_dict(), device), key
        return self._packed[1]

    # -- forward --------------------------------------------------------------------------------------------------------------
    def forward(self, coords, feats):
        what = f"fcgf.{type(self).__name__}"
        if self.training:
            raise RuntimeError(f"gmf_amd.{what}: only the eval-mode forward is built - call eval()")
        M, D = check_coords(coords, what)
        if D != self.D:
            raise RuntimeError(f"gmf_amd.{what}: coords have D = {D}, the network was built for D = {self.D}")
        feats = _f32_dev(feats, "feats", what)
        if feats.dim() != 2 or feats.shape != (M, self.in_channels):
            raise RuntimeError(f"gmf_amd.{what}: `feats` must be [{M}, {self.in_channels}] (got {tuple(feats.shape)})")
        with torch.no_grad():
            return self._forward(coords, feats)

    def _forward(self, coords, feats):
        L = self._weights(coords.device)
        maps = list(_NET_MAPS)
        c1 = self.conv1_kernel_size
        narrow = self.narrow_conv1 and self.in_channels <= NARROW_MAX_CIN
        if c1 == 3:
            c1_map = 0
        elif c1 == 1 and not narrow:
            c1_map = None                          # the generic kernel's identity map
        else:
            c1_map = len(maps)
            maps.append((c1, 0, 0))
        plan = SparsePlan(coords, 4, maps)

        def conv(i, m, lvl, xa, xb=None, residual=None, relu=False):
            W, sc, sh = L[i]
            return sparse_conv(plan, m, lvl, xa, W, xb=xb, scale=sc, shift=sh, residual=residual, relu=relu,
                               nsplit=layer_nsplit(W.shape[0], W.shape[1], W.shape[2]))

        def block(i, lvl, x):                      # residual_block.py: conv, norm, relu, conv, norm, + x, relu
            h = conv(i, lvl, lvl, x, relu=True)
            return conv(i + 1, lvl, lvl, h, residual=x, relu=True)

        if narrow:
            W, sc, sh = L[0]
            x1 = sparse_conv_narrow(plan, c1_map, 0, feats, W, scale=sc, shift=sh)
        else:
            x1 = conv(0, c1_map, 0, feats)
        # resunet.py:598-640; each block ends in a ReLU, so the MEF.relu after it is a no-op
        s1 = block(1, 0, x1)
        s2 = block(4, 1, conv(3, 4, 1, s1))
        s4 = block(7, 2, conv(6, 5, 2, s2))
        s8 = block(10, 3, conv(9, 6, 3, s4))
        t4 = block(13, 2, conv(12, 9, 2, s8))
        t2 = block(16, 1, conv(15, 8, 1, t4, xb=s4))                   # ME.cat(out_s4_tr, out_s4)
        t1 = block(19, 0, conv(18, 7, 0, t2, xb=s2))
        # :641-648: conv1_tr on ME.cat(out_s1_tr, out_s1), MEF.relu, final (+ bias), the optional normalisation
        return sparse_head_l2(plan, 0, t1, L[21][0], L[22][0], xb=s1, bias=L[22][2], normalize=self.normalize_feature)


class ResUNetBN2CX(ResUNetBN2C):
    """resunet.py:660-661: the hyper-cross kernel region.  Not built: constructing it raises NotImplementedError."""
    REGION_TYPE = "HYPER_CROSS"
