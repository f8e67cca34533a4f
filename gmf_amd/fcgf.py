"""FCGF, the feature network of DGR (reference: GMF_DeepGlobalRegistration_fcgf/model/resunet.py:419-661, ResUNetBN2C),
on the coordinate engine and sparse convolutions of `sparse.py`.  The module's forward is eval-mode and forward-only; the
differentiable train-mode forward is `gmf_amd.train.fcgf_train`, and `hardest_contrastive_loss` with
`sample_hardest_contrastive` below is the loss FCGF is trained with.

The same sparse U-Net as DGR's inlier network (`gmf_amd.ResUNetBN2C`, which stays the top-level name) without its image
fusion layers, with its own ends: conv1 (Cin = 1 in DGR, k^3 up to 7^3) runs on the narrow-input kernel
(`sparse_conv_narrow`), and conv1_tr, ReLU, final and the optional row normalisation run as one launch (`sparse_head_l2`).
Kernels: csrc/sparse_kernels.hip.  The state_dict keys and shapes are the reference's.
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import fail
from ._util import handle_and_stream
from .sparse import CONV1_TR, FINAL, _ResUNet, _folded_conv, resunet_trunk, sparse_conv_narrow, sparse_head_l2

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
            fail(self._what, f"the fused head takes out_channels in 1..{HEAD_MAX_C} (got {out_channels})", NotImplementedError)
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


# ---- training: FCGF's hardest-contrastive loss -----------------------------------------------------------------------------
# (Choy et al., "Fully Convolutional Geometric Features", ICCV 2019; the published trainer's HardestContrastiveLossTrainer.
# The reference tree freezes FCGF and holds no loss, so the definition below is this module's, with the trainer's random
# draws - the sampled positives and the candidate negatives - taken as arguments.)

LOSS_MAX_C = 64


def _index_arg(t, name, what, shape_tail=()):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
        fail(what, f"`{name}` must be an int64 tensor (got {getattr(t, 'dtype', type(t).__name__)})")
    if t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != tuple(shape_tail):
        fail(what, f"`{name}` must be [n{''.join(', ' + str(s) for s in shape_tail)}] (got {tuple(t.shape)})")
    return t


def _loss_args(F0, F1, positive_pairs, sel0, sel1, pos_sel, what):
    """Dtype and shape checks of the loss's arguments (no device needed), then the device checks."""
    for name, F in (("F0", F0), ("F1", F1)):
        if not isinstance(F, torch.Tensor) or F.dtype != torch.float32:
            fail(what, f"`{name}` must be a float32 tensor (got {getattr(F, 'dtype', type(F).__name__)})")
        if F.dim() != 2 or F.shape[0] == 0:
            fail(what, f"`{name}` must be a non-empty [N, C] tensor (got {tuple(F.shape)})")
    if F0.shape[1] != F1.shape[1]:
        fail(what, f"`F0` and `F1` must have the same width (got {F0.shape[1]} and {F1.shape[1]})")
    if not (1 <= F0.shape[1] <= LOSS_MAX_C):
        fail(what, f"the feature width must be in 1..{LOSS_MAX_C} (got {F0.shape[1]})", NotImplementedError)
    _index_arg(positive_pairs, "positive_pairs", what, (2,))
    _index_arg(sel0, "sel0", what)
    _index_arg(sel1, "sel1", what)
    if pos_sel is not None:
        _index_arg(pos_sel, "pos_sel", what)
    if sel0.shape[0] == 0 or sel1.shape[0] == 0:
        fail(what, "`sel0` and `sel1` must hold at least one candidate row each")
    for name, t in (("F0", F0), ("F1", F1), ("positive_pairs", positive_pairs), ("sel0", sel0), ("sel1", sel1), ("pos_sel", pos_sel)):
        if t is not None and not t.is_cuda:
            fail(what, f"`{name}` must live on a HIP device (got {t.device}); the HIP path is mandatory, there is no CPU fallback")


def _sum_by_dest(rows, dest, N):
    """[E, C] gradient rows with their destination rows [E] -> [N, C]: a CSR by destination from a stable sort (entries of one
    destination keep their order in `rows`), each destination's rows added in that order (`gmf_rows_sum_by_dest`)."""
    E, C = rows.shape
    sorted_dest, order = torch.sort(dest, stable=True)
    row_start = torch.searchsorted(sorted_dest, torch.arange(N + 1, device=dest.device, dtype=torch.int64))
    out = torch.empty((N, C), dtype=torch.float32, device=rows.device)
    h, st = handle_and_stream(rows)
    h.call("gmf_rows_sum_by_dest", rows.data_ptr(), E, order.data_ptr(), row_start.data_ptr(), N, C, out.data_ptr(), st)
    return out


class _HardestContrastive(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F0, F1, pairs, keys, pos_sel, sel0, sel1, pos_thresh, neg_thresh):
        F0, F1 = F0.detach().contiguous(), F1.detach().contiguous()
        dev = F0.device
        (N0, C), N1, K = F0.shape, F1.shape[0], pairs.shape[0]
        P = K if pos_sel is None else pos_sel.shape[0]
        h01 = torch.empty(P, dtype=torch.int64, device=dev)
        h10 = torch.empty(P, dtype=torch.int64, device=dev)
        keep0 = torch.empty(P, dtype=torch.uint8, device=dev)
        keep1 = torch.empty(P, dtype=torch.uint8, device=dev)
        D01 = torch.empty(P, dtype=torch.float32, device=dev)
        D10 = torch.empty(P, dtype=torch.float32, device=dev)
        terms = torch.empty(3 * P, dtype=torch.float32, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        h, st = handle_and_stream(F0)
        h.call("gmf_hardest_contrastive_forward", F0.data_ptr(), N0, F1.data_ptr(), N1, C, pairs.data_ptr(), K, keys.data_ptr(),
               _lib.ptr(pos_sel), P, sel0.data_ptr(), sel0.shape[0], sel1.data_ptr(), sel1.shape[0], float(pos_thresh),
               float(neg_thresh), h01.data_ptr(), h10.data_ptr(), keep0.data_ptr(), keep1.data_ptr(), D01.data_ptr(),
               D10.data_ptr(), terms.data_ptr(), out.data_ptr(), st)
        ctx.neg_thresh, ctx.has_sel = float(neg_thresh), pos_sel is not None
        ctx.save_for_backward(F0, F1, pairs, pos_sel if pos_sel is not None else pairs.new_empty(0), h01, h10, keep0, keep1, D01, D10,
                              terms, out)
        ctx.mark_non_differentiable(h01, h10, keep0, keep1, D01, D10)
        return out[0].clone(), out[1].clone(), h01, h10, keep0, keep1, D01, D10

    @staticmethod
    def backward(ctx, g_pos, g_neg, *_unused):
        F0, F1, pairs, pos_sel, h01, h10, keep0, keep1, D01, D10, terms, out = ctx.saved_tensors
        dev = F0.device
        (N0, C), N1, K, P = F0.shape, F1.shape[0], pairs.shape[0], h01.shape[0]
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        g_pos = zero if g_pos is None else g_pos.to(torch.float32).contiguous()
        g_neg = zero if g_neg is None else g_neg.to(torch.float32).contiguous()
        rows0 = torch.empty((3 * P, C), dtype=torch.float32, device=dev)
        rows1 = torch.empty((3 * P, C), dtype=torch.float32, device=dev)
        dest0 = torch.empty(3 * P, dtype=torch.int64, device=dev)
        dest1 = torch.empty(3 * P, dtype=torch.int64, device=dev)
        h, st = handle_and_stream(F0)
        h.call("gmf_hardest_contrastive_backward", F0.data_ptr(), N0, F1.data_ptr(), N1, C, pairs.data_ptr(), K,
               pos_sel.data_ptr() if ctx.has_sel else None, P, h01.data_ptr(), h10.data_ptr(), keep0.data_ptr(), keep1.data_ptr(),
               D01.data_ptr(), D10.data_ptr(), terms.data_ptr(), out.data_ptr(), ctx.neg_thresh, g_pos.data_ptr(), g_neg.data_ptr(),
               rows0.data_ptr(), dest0.data_ptr(), rows1.data_ptr(), dest1.data_ptr(), st)
        dF0 = _sum_by_dest(rows0, dest0, N0) if ctx.needs_input_grad[0] else None
        dF1 = _sum_by_dest(rows1, dest1, N1) if ctx.needs_input_grad[1] else None
        return dF0, dF1, None, None, None, None, None, None, None


def hardest_contrastive_loss(F0, F1, positive_pairs, sel0, sel1, pos_sel=None, pos_thresh=0.1, neg_thresh=1.4):
    """FCGF's hardest-contrastive loss on the device, differentiable in F0 and F1, with the trainer's random draws as arguments
    (`sample_hardest_contrastive` draws them).  -> (pos_loss, neg_loss, aux); the trainer's loss is pos_loss + neg_loss.

    F0 [N0, C], F1 [N1, C] float32 (C <= 64): the features of the batch (negatives may come from any cloud of it);
    positive_pairs [K, 2] int64 rows (i, j) into F0 / F1 (`matching_indices_batched`'s pairs with the batch offsets added);
    sel0 [H0], sel1 [H1] int64 candidate-negative rows of F0 / F1; pos_sel [P] int64 indices into positive_pairs (None: all).
    With (i_k, j_k) = positive_pairs[pos_sel[k]] and d(a, b) = sqrt(sum_c (a_c - b_c)^2 + 1e-7):
      h01_k = the row s of sel1 nearest to F0[i_k] (smallest float32 sum of squared differences; equal sums: the first position in
              sel1), D01_k = d(F0[i_k], F1[h01_k]); h10_k / D10_k likewise over sel0 against F1[j_k];
      keep0_k = (i_k, h01_k) is not among the K positive pairs, keep1_k = (h10_k, j_k) is not (keys i + j max(N0, N1), sorted,
              then binary search);
      pos_loss = mean_k relu(sum_c (F0[i_k] - F1[j_k])^2 - pos_thresh)
      neg_loss = (mean over keep0 of relu(neg_thresh - D01_k)^2 + mean over keep1 of relu(neg_thresh - D10_k)^2) / 2.
    A mean over no rows is 0 with a zero gradient (the published trainer gives NaN there: a deliberate departure), and so is a loss
    over no positive pairs.  aux: h01, h10 (int64 [P]), keep0, keep1 (bool [P]), D01, D10 (float32 [P]), all detached.

    The backward writes, for every k, the gradient rows of its three terms and adds them per row of F0 / F1 in a fixed order (a
    CSR by destination from a stable sort): no float atomics, bitwise-repeatable gradients for rows that several pairs share.  No
    host read in forward or backward; an index outside its tensor raises at the next `gmf_amd.check_status()`."""
    what = "fcgf.hardest_contrastive_loss"
    _loss_args(F0, F1, positive_pairs, sel0, sel1, pos_sel, what)
    pairs = positive_pairs.contiguous()
    P = pairs.shape[0] if pos_sel is None else pos_sel.shape[0]
    if P == 0:
        zero = (F0.sum() + F1.sum()) * 0.0
        e = torch.empty(0, device=F0.device)
        return zero, zero.clone(), {"h01": e.long(), "h10": e.long(), "keep0": e.bool(), "keep1": e.bool(), "D01": e, "D10": e}
    keys = torch.sort(pairs[:, 0] + pairs[:, 1] * max(F0.shape[0], F1.shape[0])).values
    pos, neg, h01, h10, keep0, keep1, D01, D10 = _HardestContrastive.apply(
        F0, F1, pairs, keys, None if pos_sel is None else pos_sel.contiguous(), sel0.contiguous(), sel1.contiguous(), pos_thresh,
        neg_thresh)
    return pos, neg, {"h01": h01, "h10": h10, "keep0": keep0.bool(), "keep1": keep1.bool(), "D01": D01, "D10": D10}


def sample_hardest_contrastive(N0, N1, K, num_pos=1024, num_hn_samples=256, generator=None):
    """The random draws of the hardest-contrastive loss, as the published trainer takes them: (sel0 [min(N0, num_hn_samples)],
    sel1 [min(N1, num_hn_samples)], pos_sel [min(K, num_pos)]) int64 on the device, each the head of a `torch.randperm`.
    `generator`: a torch.Generator of the device (its device is where the draws live); without one, the current HIP device and
    its global generator."""
    device = generator.device if generator is not None else torch.device("cuda", torch.cuda.current_device())
    draw = lambda n, m: torch.randperm(int(n), generator=generator, device=device)[:min(int(n), int(m))]   # noqa: E731
    return draw(N0, num_hn_samples), draw(N1, num_hn_samples), draw(K, num_pos)


class ResUNetBN2CX(ResUNetBN2C):
    """resunet.py:660-661: the hyper-cross kernel region.  Not built: constructing it raises NotImplementedError."""
    REGION_TYPE = "HYPER_CROSS"
