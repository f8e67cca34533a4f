"""Training path, second backward slice: forward + backward of one FusionLayer /
PerceiverIO (reference: GMF_PointDSC/models/fusion_layer.py:32-128,172-201; DGR twin model/perceiver_io.py) as a
``torch.autograd.Function`` over the training primitives of the C ABI (``gmf_gemm_f32``, ``gmf_lcpe``,
``gmf_layernorm_*``, ``gmf_softmax_rows``, ``gmf_geglu``, ``gmf_colsum`` - gmf_amd/csrc/train_kernels.hip).

Every tensor stays on the device, every kernel is HIP; torch only owns the memory and the autograd graph.  The
function is NOT the fused inference kernel: it saves its activations (x', LN statistics, q, k|v, P, the 1024-wide
hidden layer ...) for the backward, as the reference's autograd does.  Gradients equal the reference's own
(golden F18).
"""
from __future__ import annotations

import torch

from ._util import handle_and_stream, require_cuda_f32


def _p(t, off=0):
    return t.data_ptr() + 4 * off


def _call(name, on, *args):
    """C function `name` on the handle and current stream of tensor `on`: a tensor goes as its data_ptr(), None as NULL, a bool
    as 0 / 1, anything else (numbers, raw pointers such as `_p(...)`) as it is; the stream goes last."""
    h, st = handle_and_stream(on)
    h.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else int(a) if isinstance(a, bool) else a for a in args], st)


SIGMA_ON_DEVICE = object()       # [r5] marker in place of sigma's host value: the kernels read the parameter's device memory


class sigma_device:
    """`with sigma_device(handle, sigma_tensor):` - the C calls inside read PointDSC's learnable sigma (PointDSC.py:164) from the
    tensor's device memory (gmf_set_sigma_device) instead of a by-value float; None = the by-value form.  Host-side state only:
    inside a graph capture the calls between enter and exit are what gets captured."""

    def __init__(self, h, sigma):
        self.h, self.sigma = h, sigma

    def __enter__(self):
        if self.sigma is not None:
            self.h.call("gmf_set_sigma_device", self.sigma.data_ptr())

    def __exit__(self, *exc):
        if self.sigma is not None:
            self.h.call("gmf_set_sigma_device", None)
        return False


def gemm(a, b, ta=False, tb=False, bias=None, residual=None, alpha=1.0, out=None, m=None, n=None, k=None, lda=None, ldb=None,
         ldc=None, a_off=0, b_off=0, c_off=0, batch=1, sa=0, sb=0, sc=0, relu=False):
    """out = alpha * op(a) op(b) (+ bias) (+ residual) through gmf_gemm_f32.  With the keyword geometry left out, `a` and `b`
    are dense 2-D row-major matrices; with it, any sub-matrix / batch of a larger buffer (offsets and strides in floats)."""
    if m is None:
        m, k = (a.shape[1], a.shape[0]) if ta else (a.shape[0], a.shape[1])
        n = b.shape[0] if tb else b.shape[1]
        lda, ldb = a.shape[1], b.shape[1]
    if out is None:
        out = torch.empty((batch, m, n) if batch > 1 else (m, n), device=a.device, dtype=torch.float32)
        ldc, sc = n, m * n
    _call("gmf_gemm_f32", a, bool(ta), bool(tb), _p(a, a_off), _p(b, b_off), _p(out, c_off), bias,
          None if residual is None else _p(residual, c_off), m, n, k, lda, ldb, ldc, sa, sb, sc, batch, float(alpha), bool(relu))
    return out


def colsum(x, y=None, mean=None, rstd=None, shift=0, L=None, dual=False, relu_y=None):
    """[rows, C] -> [C]: sum_r x[r] * y'[r + shift] (see gmf_colsum).  dual: ([C] that sum, [C] the plain column sums of x)
    from ONE pass; relu_y: x is masked by the saved output of a ReLU first."""
    rows, C = x.shape
    out = torch.empty(2 * C if dual else C, device=x.device, dtype=torch.float32)
    _call("gmf_colsum", x, x, y, mean, rstd, None, None, 0, int(shift), int(L if L is not None else rows), rows, C, relu_y, bool(dual),
          out)
    return (out[:C], out[C:]) if dual else out


def layernorm_fwd(x, gamma, beta):
    rows, C = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    _call("gmf_layernorm_forward", x, x, gamma, beta, y, mean, rstd, rows, C)
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dx_add=None):
    rows, C = x.shape
    dx = torch.empty_like(x)
    _call("gmf_layernorm_backward", x, dy, x, gamma, mean, rstd, dx_add, dx, rows, C)
    return dx


def lcpe_fwd(x2d, w, b, L):
    y = torch.empty_like(x2d)
    _call("gmf_lcpe", x2d, 0, x2d, w, b, y, x2d.shape[0], L, x2d.shape[1])
    return y


def lcpe_bwd(dy2d, w, L):
    dx = torch.empty_like(dy2d)
    _call("gmf_lcpe", dy2d, 1, dy2d, w, None, dx, dy2d.shape[0], L, dy2d.shape[1])
    return dx


def softmax_rows(S2d, scale, mul=None):
    P = torch.empty_like(S2d)
    _call("gmf_softmax_rows", S2d, 0, S2d, None, mul, P, S2d.shape[0], S2d.shape[1], float(scale))
    return P


def softmax_rows_bwd(P2d, dP2d, scale, mul=None):
    dS = torch.empty_like(P2d)
    _call("gmf_softmax_rows", P2d, 1, P2d, dP2d, mul, dS, P2d.shape[0], P2d.shape[1], float(scale))
    return dS


def geglu_fwd(hdn):
    rows, H2 = hdn.shape
    g = torch.empty((rows, H2 // 2), device=hdn.device, dtype=torch.float32)
    _call("gmf_geglu", hdn, 0, hdn, None, g, rows, H2 // 2)
    return g


def geglu_bwd(hdn, dg):
    dh = torch.empty_like(hdn)
    _call("gmf_geglu", hdn, 1, hdn, dg, dh, hdn.shape[0], hdn.shape[1] // 2)
    return dh


def relu_backward(dy, y):
    """dy masked by the saved output y of a ReLU: y > 0 ? dy : 0 (gmf_relu_backward)."""
    g = torch.empty_like(dy)
    _call("gmf_relu_backward", dy, dy, y, g, dy.numel())
    return g


class _FusionLayerTrain(torch.autograd.Function):
    """forward(data [B,T,dim], x [B,N,lat], pe, *params) -> [B,N,lat] with params in the order of `_param_list`."""

    @staticmethod
    def forward(ctx, data, x, pe, *params):
        data = require_cuda_f32(data, "data").contiguous()
        x = require_cuda_f32(x, "queries_encoder").contiguous()
        params = [p.detach().contiguous() for p in params]
        if pe:
            wq_t, bq_t, wc_t, bc_t = params[:4]
            rest = params[4:]
        else:
            rest = params
        g1, b1n, gc, bcn, Wq, Wkv, Wo, bo, g2, b2n, W1, bf1, W2, bf2 = rest
        B, N, lat = x.shape
        T, dim = data.shape[1], data.shape[2]
        dh = Wq.shape[0]
        scale = dh ** -0.5
        x2, c2 = x.reshape(B * N, lat), data.reshape(B * T, dim)
        xp = lcpe_fwd(x2, wq_t, bq_t, N) if pe else x2
        cp = lcpe_fwd(c2, wc_t, bc_t, T) if pe else c2
        xn, mu1, rs1 = layernorm_fwd(xp, g1, b1n)
        cn, muc, rsc = layernorm_fwd(cp, gc, bcn)
        q = gemm(xn, Wq, tb=True)                                   # [BN, dh]
        kv = gemm(cn, Wkv, tb=True)                                 # [BT, 2 dh] = k | v
        S = torch.empty((B, N, T), device=x.device, dtype=torch.float32)
        gemm(q, kv, tb=True, out=S, m=N, n=T, k=dh, lda=dh, ldb=2 * dh, ldc=T, batch=B, sa=N * dh, sb=T * 2 * dh, sc=N * T)
        P = softmax_rows(S.reshape(B * N, T), scale)
        a = torch.empty((B * N, dh), device=x.device, dtype=torch.float32)
        gemm(P, kv, out=a, m=N, n=dh, k=T, lda=T, ldb=2 * dh, ldc=dh, b_off=dh, batch=B, sa=N * T, sb=T * 2 * dh, sc=N * dh)
        x1 = gemm(a, Wo, tb=True, bias=bo, residual=xp)             # [BN, lat]
        xn2, mu2, rs2 = layernorm_fwd(x1, g2, b2n)
        hdn = gemm(xn2, W1, tb=True, bias=bf1)                      # [BN, 2 H]
        g = geglu_fwd(hdn)
        out = gemm(g, W2, tb=True, bias=bf2, residual=x1)
        ctx.pe, ctx.dims, ctx.scale = pe, (B, N, T, lat, dim, dh), scale
        ctx.save_for_backward(x2, c2, xp, cp, mu1, rs1, muc, rsc, xn, cn, q, kv, P, a, x1, mu2, rs2, xn2, hdn, g, *params)
        return out.reshape(B, N, lat)

    @staticmethod
    def backward(ctx, dout):
        (x2, c2, xp, cp, mu1, rs1, muc, rsc, xn, cn, q, kv, P, a, x1, mu2, rs2, xn2, hdn, g, *params) = ctx.saved_tensors
        pe, scale = ctx.pe, ctx.scale
        B, N, T, lat, dim, dh = ctx.dims
        if pe:
            wq_t, bq_t, wc_t, bc_t = params[:4]
            rest = params[4:]
        else:
            rest = params
        g1, b1n, gc, bcn, Wq, Wkv, Wo, bo, g2, b2n, W1, bf1, W2, bf2 = rest
        dev = dout.device
        d2 = require_cuda_f32(dout, "grad").contiguous().reshape(B * N, lat)
        # ---- feed-forward (fusion_layer.py:54-69,191) ----
        dW2 = gemm(d2, g, ta=True)                                  # [lat, H]
        db2 = colsum(d2)
        dg = gemm(d2, W2)                                           # [BN, H]
        dhd = geglu_bwd(hdn, dg)                                    # [BN, 2 H]
        dW1 = gemm(dhd, xn2, ta=True)                               # [2 H, lat]
        db1 = colsum(dhd)
        dxn2 = gemm(dhd, W1)                                        # [BN, lat]
        dg2, dbn2 = colsum(dxn2, y=x1, mean=mu2, rstd=rs2, dual=True)
        dx1 = layernorm_bwd(dxn2, x1, g2, mu2, rs2, dx_add=d2)
        # ---- cross-attention (fusion_layer.py:71-94,190) ----
        dWo = gemm(dx1, a, ta=True)                                 # [lat, dh]
        dbo = colsum(dx1)
        da = gemm(dx1, Wo)                                          # [BN, dh]
        dP = torch.empty((B * N, T), device=dev, dtype=torch.float32)
        gemm(da, kv, tb=True, out=dP, m=N, n=T, k=dh, lda=dh, ldb=2 * dh, ldc=T, b_off=dh, batch=B, sa=N * dh, sb=T * 2 * dh, sc=N * T)
        dkv = torch.empty((B * T, 2 * dh), device=dev, dtype=torch.float32)
        gemm(P, da, ta=True, out=dkv, m=T, n=dh, k=N, lda=T, ldb=dh, ldc=2 * dh, c_off=dh, batch=B, sa=N * T, sb=N * dh, sc=T * 2 * dh)   # dv
        dS = softmax_rows_bwd(P, dP, scale)
        dq = torch.empty((B * N, dh), device=dev, dtype=torch.float32)
        gemm(dS, kv, out=dq, m=N, n=dh, k=T, lda=T, ldb=2 * dh, ldc=dh, batch=B, sa=N * T, sb=T * 2 * dh, sc=N * dh)
        gemm(dS, q, ta=True, out=dkv, m=T, n=dh, k=N, lda=T, ldb=dh, ldc=2 * dh, batch=B, sa=N * T, sb=N * dh, sc=T * 2 * dh)            # dk
        dWq = gemm(dq, xn, ta=True)                                 # [dh, lat]
        dxn = gemm(dq, Wq)                                          # [BN, lat]
        dWkv = gemm(dkv, cn, ta=True)                               # [2 dh, dim]
        dcn = gemm(dkv, Wkv)                                        # [BT, dim]
        dg1, dbn1 = colsum(dxn, y=xp, mean=mu1, rstd=rs1, dual=True)
        dxp = layernorm_bwd(dxn, xp, g1, mu1, rs1, dx_add=dx1)
        dgc, dbnc = colsum(dcn, y=cp, mean=muc, rstd=rsc, dual=True)
        dcp = layernorm_bwd(dcn, cp, gc, muc, rsc)
        grads = []
        if pe:
            # ---- LCPE (fusion_layer.py:118-128) ----
            dx = lcpe_bwd(dxp, wq_t, N)
            dc = lcpe_bwd(dcp, wc_t, T)
            tq0, dbq = colsum(dxp, y=x2, shift=0, L=N, dual=True)        # the centre tap and the bias from one pass
            tc0, dbc = colsum(dcp, y=c2, shift=0, L=T, dual=True)
            dwq = torch.stack([colsum(dxp, y=x2, shift=-1, L=N), tq0, colsum(dxp, y=x2, shift=1, L=N)], dim=1).reshape(wq_t.shape)
            dwc = torch.stack([colsum(dcp, y=c2, shift=-1, L=T), tc0, colsum(dcp, y=c2, shift=1, L=T)], dim=1).reshape(wc_t.shape)
            grads += [dwq, dbq, dwc, dbc]
        else:
            dx, dc = dxp, dcp
        grads += [dg1, dbn1, dgc, dbnc, dWq, dWkv, dWo, dbo, dg2, dbn2, dW1, db1, dW2, db2]
        return (dc.reshape(B, T, dim), dx.reshape(B, N, lat), None, *grads)


def _param_list(layer):
    attn, ff = layer.cross_attend_blocks
    ps = []
    if layer.pe:
        ps += [layer.cpe.proj_q.weight, layer.cpe.proj_q.bias, layer.cpe.proj_content.weight, layer.cpe.proj_content.bias]
    ps += [attn.norm.weight, attn.norm.bias, attn.norm_context.weight, attn.norm_context.bias,
           attn.fn.to_q.weight, attn.fn.to_kv.weight, attn.fn.to_out.weight, attn.fn.to_out.bias,
           ff.norm.weight, ff.norm.bias, ff.fn.net[0].weight, ff.fn.net[0].bias, ff.fn.net[2].weight, ff.fn.net[2].bias]
    return ps


def fusion_layer_train(layer, data, queries):
    """Differentiable FusionLayer / PerceiverIO forward (depth = 0, one cross head): gradients flow to `data`, `queries`
    and every parameter of `layer`."""
    if getattr(layer, "depth", 0) != 0 or getattr(layer, "cross_heads", 1) != 1:
        raise NotImplementedError("gmf_amd.FusionLayer: the differentiable path covers what GMF trains (depth 0, one cross-attention head: "
                                  "PointDSC.py:29-38,92-100); latent self-attention layers / several heads are forward-only (eval())")
    return _FusionLayerTrain.apply(data, queries, bool(layer.pe), *_param_list(layer))


# =====================================================================================================================
# The rest of the encoder in training mode (PointDSC.py:10-74,77-143,175-181 with TRAIN-mode BatchNorm) and the two losses
# the reference trains with by default (libs/loss.py:67-140; config_3DMatch.py:50-52: weight_transformation = 0).
# Activations are token-major [B * N, C] rows (the reference's [B, C, N] transposed; BatchNorm1d over (B, N) per channel =
# per column over all rows).
# =====================================================================================================================
class _Linear(torch.autograd.Function):
    """y = relu?(x W^T + b (+ residual)); x [rows, in], W [out, in] (a Conv1d k = 1 weight squeezed), residual [rows, out]."""

    @staticmethod
    def forward(ctx, x, W, b, residual, relu):
        x = x.contiguous()
        W2 = W.detach().reshape(W.shape[0], -1).contiguous()
        y = gemm(x, W2, tb=True, bias=None if b is None else b.detach(), residual=None if residual is None else residual.contiguous(),
                 relu=relu)
        ctx.relu, ctx.has_b, ctx.has_r, ctx.wshape = relu, b is not None, residual is not None, W.shape
        ctx.save_for_backward(x, W2, y if relu else x.new_empty(0))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W2, y = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.relu:
            dy = relu_backward(dy, y)
        dW = gemm(dy, x, ta=True).reshape(ctx.wshape)
        db = colsum(dy) if ctx.has_b else None
        dx = gemm(dy, W2)
        return dx, dW, db, (dy if ctx.has_r else None), None


def linear(x, W, b=None, residual=None, relu=False):
    return _Linear.apply(x, W, b, residual, relu)


class _BatchNormTrain(torch.autograd.Function):
    """relu?(bn(x) (+ residual)) with nn.BatchNorm1d / 2d in training mode on rows [rows, C] (the residual: a BasicBlock's identity
    branch, resnet.py:59-75); updates running_mean / running_var in place.  The residual's gradient is dy masked by the ReLU."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, running_mean, running_var, eps, momentum, relu):
        x = x.contiguous()
        rows, C = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(C, device=x.device, dtype=torch.float32)
        rstd = torch.empty(C, device=x.device, dtype=torch.float32)
        tail = (gamma, beta, y, mean, rstd, running_mean, running_var, rows, C, float(eps), float(momentum), bool(relu))
        if residual is None:
            _call("gmf_batchnorm_train_forward", x, x, *tail)
        else:
            _call("gmf_batchnorm_residual_forward", x, x, residual.contiguous(), *tail)
        ctx.relu = relu
        ctx.save_for_backward(x, gamma.detach(), mean, rstd, y if relu else x.new_empty(0))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd, y = ctx.saved_tensors
        dy = dy.contiguous()
        rows, C = x.shape
        dx = torch.empty_like(x)
        dg = torch.empty(C, device=x.device, dtype=torch.float32)
        db = torch.empty(C, device=x.device, dtype=torch.float32)
        _call("gmf_batchnorm_train_backward", x, dy, x, y if ctx.relu else None, mean, rstd, gamma, dx, dg, db, rows, C)
        dres = None
        if ctx.needs_input_grad[1]:
            dres = relu_backward(dy, y) if ctx.relu else dy
        return dx, dres, dg, db, None, None, None, None, None


def _bn_tracked(bn, who, apply):
    """torch's train-mode bookkeeping around `apply(running_mean, running_var)` ((None, None) when `bn` tracks none):
    num_batches_tracked advances after the call.  Shared by the dense and the masked form."""
    if bn.momentum is None:
        raise NotImplementedError(f"gmf_amd.train: BatchNorm with cumulative moving average (momentum=None) is not used by {who}")
    track = bn.track_running_stats
    y = apply(*((bn.running_mean, bn.running_var) if track else (None, None)))
    if track and bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1
    return y


def batchnorm_train(x, bn, relu=False, residual=None):
    """relu?(bn(x) (+ residual)); `bn`: an nn.BatchNorm1d / 2d whose parameters and running statistics are used / updated
    exactly as torch would in train()."""
    return _bn_tracked(bn, "GMF", lambda rm, rv: _BatchNormTrain.apply(x, residual, bn.weight, bn.bias, rm, rv, bn.eps, bn.momentum,
                                                                      bool(relu)))


class _SCAttention(torch.autograd.Function):
    """message = softmax_j(compat_ij * <q_i, k_j> / sqrt(C)) V per pair (PointDSC.py:56-64).  qkv [B, N, 3C] token-major holds
    Q | K | V side by side (ONE projection GEMM produces them, one GEMM each takes their gradients back: the products below
    address the three column blocks through leading dimensions and offsets); compat [B, N, N] has no gradient (the reference
    computes it under no_grad, PointDSC.py:216-221)."""

    @staticmethod
    def forward(ctx, qkv, compat):
        qkv, compat = qkv.contiguous(), compat.contiguous()
        B, N, C3 = qkv.shape
        Cc = C3 // 3
        scale = 1.0 / (Cc ** 0.5)
        S = torch.empty((B, N, N), device=qkv.device, dtype=torch.float32)
        gemm(qkv, qkv, tb=True, out=S, m=N, n=N, k=Cc, lda=C3, ldb=C3, ldc=N, b_off=Cc, batch=B, sa=N * C3, sb=N * C3, sc=N * N)
        P = softmax_rows(S.reshape(B * N, N), scale, mul=compat.reshape(B * N, N))
        msg = torch.empty((B, N, Cc), device=qkv.device, dtype=torch.float32)
        gemm(P, qkv, out=msg, m=N, n=Cc, k=N, lda=N, ldb=C3, ldc=Cc, b_off=2 * Cc, batch=B, sa=N * N, sb=N * C3, sc=N * Cc)
        ctx.scale = scale
        ctx.save_for_backward(qkv, compat, P)
        return msg

    @staticmethod
    def backward(ctx, dmsg):
        qkv, compat, P = ctx.saved_tensors
        dmsg = dmsg.contiguous()
        B, N, C3 = qkv.shape
        Cc = C3 // 3
        dev = qkv.device
        dqkv = torch.empty_like(qkv)
        dP = torch.empty((B * N, N), device=dev, dtype=torch.float32)
        gemm(dmsg, qkv, tb=True, out=dP, m=N, n=N, k=Cc, lda=Cc, ldb=C3, ldc=N, b_off=2 * Cc, batch=B, sa=N * Cc, sb=N * C3, sc=N * N)
        gemm(P, dmsg, ta=True, out=dqkv, m=N, n=Cc, k=N, lda=N, ldb=Cc, ldc=C3, c_off=2 * Cc, batch=B, sa=N * N, sb=N * Cc,
             sc=N * C3)                                                                              # dV
        dS = softmax_rows_bwd(P, dP, ctx.scale, mul=compat.reshape(B * N, N))
        gemm(dS, qkv, out=dqkv, m=N, n=Cc, k=N, lda=N, ldb=C3, ldc=C3, b_off=Cc, batch=B, sa=N * N, sb=N * C3, sc=N * C3)     # dQ = dS K
        gemm(dS, qkv, ta=True, out=dqkv, m=N, n=Cc, k=N, lda=N, ldb=C3, ldc=C3, c_off=Cc, batch=B, sa=N * N, sb=N * C3,
             sc=N * C3)                                                                              # dK = dS^T Q
        return dqkv, None


def sc_attention(qkv, compat):
    return _SCAttention.apply(qkv, compat)


def nonlocal_block_train(block, feat, compat, image_feat, B, N):
    """NonLocalBlock.forward (PointDSC.py:40-74) on token-major rows feat [B * N, C]; returns [B * N, C]."""
    C = feat.shape[1]
    # Q | K | V from ONE product (the concatenation is a view-free torch.cat of three small parameters; autograd hands each its
    # slice of the joint gradient)
    Wqkv = torch.cat([block.projection_q.weight, block.projection_k.weight, block.projection_v.weight], dim=0)
    bqkv = torch.cat([block.projection_q.bias, block.projection_k.bias, block.projection_v.bias], dim=0)
    qkv = linear(feat, Wqkv, bqkv)
    msg = sc_attention(qkv.reshape(B, N, 3 * C), compat).reshape(B * N, C)
    fm = block.fc_message
    m1 = batchnorm_train(linear(msg, fm[0].weight, fm[0].bias), fm[1], relu=True)
    m2 = batchnorm_train(linear(m1, fm[3].weight, fm[3].bias), fm[4], relu=True)
    fused = fusion_layer_train(block.fusion_layer_2, image_feat, feat.reshape(B, N, C)).reshape(B * N, C)
    return linear(m2, fm[6].weight, fm[6].bias, residual=fused)           # message + image_feat (PointDSC.py:73)


def encoder_train(net, corr_pos, compat, p_tokens, q_tokens):
    """NonLocalNet.forward (PointDSC.py:114-143) from image TOKENS; returns corr_features [B, N, C] (= the reference's
    encoder output permuted to token-major, PointDSC.py:223-228)."""
    B, N, D = corr_pos.shape
    image_feat = fusion_layer_train(net.fusion_layer_1, p_tokens, q_tokens)            # PointDSC.py:137
    feat = linear(corr_pos.reshape(B * N, D).contiguous(), net.layer0.weight, net.layer0.bias)
    for i in range(net.num_layers):
        pc = net.blocks[f"PointCN_layer_{i}"]
        feat = batchnorm_train(linear(feat, pc[0].weight, pc[0].bias), pc[1], relu=True)
        feat = nonlocal_block_train(net.blocks[f"NonLocal_layer_{i}"], feat, compat, image_feat, B, N)
    return feat.reshape(B, N, -1)


def classifier_train(cls, feat):
    """PointDSC.classification (PointDSC.py:175-181,241): [B, N, C] -> logits [B, N]."""
    B, N, C = feat.shape
    h1 = linear(feat.reshape(B * N, C), cls[0].weight, cls[0].bias, relu=True)
    h2 = linear(h1, cls[2].weight, cls[2].bias, relu=True)
    return linear(h2, cls[4].weight, cls[4].bias).reshape(B, N)


class _Normalize(torch.autograd.Function):
    """F.normalize(x, p=2, dim=-1) (PointDSC.py:229) on rows [rows, C]: LayerNorm-free row scaling, done with the primitives:
    y = x / max(||x||, 1e-12); dx = (dy - y <dy, y>) / ||x||."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        nrm = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
        y = torch.empty_like(x)
        _call("gmf_normalize_rows", x, 0, x, None, nrm, y, x.shape[0], x.shape[1])
        ctx.save_for_backward(y, nrm)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, nrm = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        _call("gmf_normalize_rows", y, 1, y, dy, nrm, dx, y.shape[0], y.shape[1])
        return dx


def normalize_rows(x):
    return _Normalize.apply(x)


class _SimilarityMatrix(torch.autograd.Function):
    """M = clamp(1 - (1 - Fn Fn^T) / sigma^2, 0, 1), zero diagonal (PointDSC.py:231-234), dense [B, N, N], differentiable with
    respect to Fn and sigma for any upstream gradient (gmf_similarity_backward)."""

    @staticmethod
    def forward(ctx, feat_n, sigma, sigma_value):
        f = feat_n.contiguous()
        B, N, _ = f.shape
        on_dev = sigma_value is SIGMA_ON_DEVICE          # [r5] no host read: the kernels take sigma from the parameter's own memory
        sig = 1.0 if on_dev else (float(sigma) if sigma_value is None else float(sigma_value))     # (a caller that already read the scalar passes it)
        M = torch.empty((B, N, N), device=f.device, dtype=torch.float32)
        h, _ = handle_and_stream(f)
        with sigma_device(h, sigma if on_dev else None):
            _call("gmf_similarity_matrix", f, f, B, N, sig, M, N)
        ctx.sig, ctx.sigma_is_tensor, ctx.sigma_dev = sig, torch.is_tensor(sigma), (sigma if on_dev else None)
        ctx.save_for_backward(f)
        return M

    @staticmethod
    def backward(ctx, dM):
        (f,) = ctx.saved_tensors
        B, N, _ = f.shape
        dM = dM.contiguous()
        dF = torch.empty_like(f)
        dsig = torch.empty(1, device=f.device, dtype=torch.float32)
        h, _ = handle_and_stream(f)
        with sigma_device(h, ctx.sigma_dev):
            _call("gmf_similarity_backward", f, f, dM, B, N, ctx.sig, dF, dsig)
        return dF, dsig if ctx.sigma_is_tensor else None, None


def similarity_matrix_train(feat_n, sigma, sigma_value=None):
    return _SimilarityMatrix.apply(feat_n, sigma, sigma_value)


class _ClassificationLossFn(torch.autograd.Function):
    """The loss value of ClassificationLoss (libs/loss.py:67-93) with its gradient with respect to the logits."""

    @staticmethod
    def forward(ctx, pred, gt, weight, balanced):
        pred = pred.contiguous()
        out = torch.empty(6, device=pred.device, dtype=torch.float32)
        _call("gmf_classification_loss", pred, pred, gt, weight, pred.shape[0], pred.shape[1], bool(balanced), out)
        ctx.balanced = balanced
        ctx.save_for_backward(pred, gt, weight if weight is not None else pred.new_empty(0))
        ctx.has_w = weight is not None
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, dloss, _dstats):
        pred, gt, weight = ctx.saved_tensors
        d = torch.empty_like(pred)
        _call("gmf_classification_backward", pred, pred, gt, weight if ctx.has_w else None, pred.shape[0], pred.shape[1],
              bool(ctx.balanced), d)
        return dloss * d, None, None, None


def classification_loss_train(pred, gt, weight, balanced):
    return _ClassificationLossFn.apply(pred, gt, weight, balanced)


class _SpectralMatchingDense(torch.autograd.Function):
    """SpectralMatchingLoss(M, gt) (libs/loss.py:116-140) on a dense M with its gradient dL/dM."""

    @staticmethod
    def forward(ctx, M, gt, balanced):
        N = M.shape[1]
        if not (M.stride(2) == 1 and M.stride(1) >= N and M.stride(0) == N * M.stride(1)):
            M = M.contiguous()
        out = torch.empty(1, device=M.device, dtype=torch.float32)
        _call("gmf_spectral_matching_loss", M, M, M.stride(1), gt, M.shape[0], N, bool(balanced), out)
        ctx.balanced = balanced
        ctx.save_for_backward(M, gt)
        return out[0].clone()

    @staticmethod
    def backward(ctx, dloss):
        M, gt = ctx.saved_tensors
        B, N = M.shape[0], M.shape[1]
        dM = torch.empty((B, N, N), device=M.device, dtype=torch.float32)
        _call("gmf_spectral_matching_dense_backward", M, M, M.stride(1), gt, B, N, bool(ctx.balanced), dM)
        return dloss * dM, None, None


def spectral_matching_loss_train(M, gt, balanced):
    return _SpectralMatchingDense.apply(M, gt, balanced)


def compat_dense(src, tgt, sigma_d):
    """[B, N, N] spatial-consistency matrix of PointDSC.py:216-221 (no gradient, as in the reference)."""
    B, N, _ = src.shape
    out = torch.empty((B, N, N), device=src.device, dtype=torch.float32)
    _call("gmf_compat_dense", src, src, tgt, B, N, float(sigma_d), out)
    return out


class _PoseHeadTrain(torch.autograd.Function):
    """final_trans of the non-test forward (PointDSC.py:246-252,304-425): top-S seeds by confidence, kNN in feature space,
    compatibility matrix + power iteration + weighted Kabsch per seed, the hypothesis with most inliers.  Forward =
    gmf_pose_head; backward = gmf_pose_head_backward (only the best seed of each pair carries gradient: to the k neighbour
    rows of the unit features and to sigma)."""

    @staticmethod
    def forward(ctx, feat_n, sigma, model, src, tgt, logits, sigmas):
        f = feat_n.contiguous()
        on_dev = sigmas is not None and sigmas[0] is SIGMA_ON_DEVICE
        if on_dev:
            sigmas = (1.0, sigmas[1])                    # (placeholder: the kernels read sigma from the parameter's memory)
        h, _ = handle_and_stream(f)
        with sigma_device(h, sigma if on_dev else None):
            final_T, _, aux = model.pose_head(f, src, tgt, logits, False, return_aux=True, sigmas=sigmas)
        ctx.model, ctx.sigmas, ctx.sigma_is_tensor, ctx.sigma_dev = model, sigmas, torch.is_tensor(sigma), (sigma if on_dev else None)
        ctx.save_for_backward(f, src, tgt, aux["knn_idx"], aux["fitness"])
        return final_T

    @staticmethod
    def backward(ctx, dT):
        f, src, tgt, knn_idx, fitness = ctx.saved_tensors
        B, N, _ = f.shape
        pp, _, _ = ctx.model._pose_params(N, False, ctx.sigmas)
        dT = dT.contiguous()
        dF = torch.empty_like(f)
        dsig = torch.empty(B, device=f.device, dtype=torch.float32)
        h, _ = handle_and_stream(f)
        with sigma_device(h, ctx.sigma_dev):
            _call("gmf_pose_head_backward", f, pp, f, src, tgt, knn_idx, fitness, dT, B, N, dF, dsig)
        return dF, (dsig.sum().reshape(1) if ctx.sigma_is_tensor else None), None, None, None, None, None


def pose_head_train(model, feat_n, sigma, src, tgt, logits, sigmas):
    return _PoseHeadTrain.apply(feat_n, sigma, model, src, tgt, logits, sigmas)


class GraphedTrainingStep:
    """One training step of `model` (a gmf_amd.PointDSC in train() mode) - forward, loss, backward, optimizer step - captured ONCE as a
    HIP graph and replayed (libs/trainer.py:131-166 is the loop this stands in for).  An eager step is ~1 900 kernel launches from
    ~320 C calls; the replay is one launch from Python.  It is NOT shorter than a well-fed eager step: the kernels are dependent and
    sum to ~24 ms at 16 x 1000 - the graph removes the host from the loop, not time from the device.

    What makes the step capturable: `model.sigma_on_device = True` (the learnable sigma is read by the kernels from the parameter's
    own memory, gmf_set_sigma_device - the eager step reads it to the host once per step), a `loss_fn(result, batch) -> 0-dim device
    tensor` that makes no host read (`ClassificationLoss(host_stats=False)`), and an optimizer whose step is capturable
    (`torch.optim.Adam(..., capturable=True, fused=True)` - fused: torch's multi-tensor Adam under capture issues three broadcast
    divisions per parameter, ~950 launches and 4 ms of a 27 ms step at 16 x 1000).  `warmup` eager steps run first, on a side stream: they size the library's workspace
    and the allocator's pools, and they are real optimizer steps.  Shapes are fixed by the example batch; `__call__(batch)` copies
    the tensors of `batch` into the captured inputs and replays."""

    def __init__(self, model, optimizer, loss_fn, batch, warmup: int = 3):
        self.model, self.optimizer, self.loss_fn = model, optimizer, loss_fn
        model.sigma_on_device = True
        self.static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}

        def step():
            optimizer.zero_grad(set_to_none=True)
            loss = loss_fn(model(self.static), self.static)
            loss.backward()
            optimizer.step()
            return loss
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        with torch.cuda.graph(self.graph):
            self.loss = step()

    def __call__(self, batch=None):
        if batch is not None:
            for k, v in batch.items():
                if torch.is_tensor(v):
                    self.static[k].copy_(v)
        self.graph.replay()
        return self.loss


# =====================================================================================================================
# DGR's inlier network ResUNetBN2C in training mode (resunet_new.py:627-706 with batch-statistics BatchNorm; the loop of
# GMF_DeepGlobalRegistration_fcgf/core/trainer.py:159-305).  Activations are the plan's [M, C] level buffers: counts[l] valid rows
# first, the rest written as 0 by every BatchNorm and every data gradient.


# Not merged with the dense `_BatchNormTrain`: k_bnm_* chunk differently, take 1 / sqrtf for rsqrtf, write zero rows - other bits.
class _BatchNormMasked(torch.autograd.Function):
    """MinkowskiBatchNorm in training mode over the counts[level] valid rows of x [M, C] (`gmf_batchnorm_masked_forward`), + an
    optional residual, + an optional ReLU; rows past the count are 0 in y and dx; the residual's gradient is the masked upstream
    gradient g.  Updates running_mean / running_var in place."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, running_mean, running_var, n_ptr, eps, momentum, relu):
        x = x.detach().contiguous()
        cap, C = x.shape
        res = None if residual is None else residual.detach().contiguous()
        y = torch.empty_like(x)
        mean = torch.empty(C, device=x.device, dtype=torch.float32)
        rstd = torch.empty(C, device=x.device, dtype=torch.float32)
        _call("gmf_batchnorm_masked_forward", x, x, res, gamma, beta, n_ptr, cap, C, float(eps), float(momentum), bool(relu), y, mean,
              rstd, running_mean, running_var)
        ctx.relu, ctx.n_ptr, ctx.has_res = relu, n_ptr, residual is not None
        ctx.save_for_backward(x, gamma.detach(), mean, rstd, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd, y = ctx.saved_tensors
        dy = require_cuda_f32(dy, "grad").contiguous()
        cap, C = x.shape
        g = torch.empty_like(x)
        dx = torch.empty_like(x)
        dg = torch.empty(C, device=x.device, dtype=torch.float32)
        db = torch.empty(C, device=x.device, dtype=torch.float32)
        _call("gmf_batchnorm_masked_backward", x, dy, x, y if ctx.relu else None, mean, rstd, gamma, ctx.n_ptr, cap, C, g, dx, dg, db)
        return dx, (g if ctx.has_res else None), dg, db, None, None, None, None, None, None


def batchnorm_masked(x, bn, plan, level: int, residual=None, relu: bool = False):
    """`bn` (an nn.BatchNorm1d) in train() mode over the valid rows of level `level` of `plan`: relu?(bn(x) + residual), rows past
    counts[level] written as 0.  Parameters and running statistics are used / updated exactly as torch would."""
    return _bn_tracked(bn, "DGR", lambda rm, rv: _BatchNormMasked.apply(x, residual, bn.weight, bn.bias, rm, rv, plan.count_ptr(level),
                                                                       bn.eps, bn.momentum, bool(relu)))


def resunet_train(model, coords, feats, p_image=None, q_image=None, p_tokens=None, q_tokens=None):
    """The differentiable train-mode forward of a gmf_amd.ResUNetBN2C (resunet_new.py:627-706, batch-statistics BatchNorm):
    logits [M, out_channels], aligned with the input rows.  Gradients reach the 23 kernels, final.bias, the 21 BatchNorms, both
    fusion layers, the image encoder (`image_encoder_train`, HIP kernels) when images are given, and p_tokens / q_tokens when tokens
    are given; every running statistic is updated as torch does.  The eval path's conventions hold: one image pair, the
    bottleneck's queries all stride-8 rows in ascending (batch, coordinates) order, zero rows past the level count (the position
    encoding's zero padding for pe=True).  Reads the four level counts to the host once, to raise as torch's BatchNorm does on
    a level of fewer than 2 rows."""
    from .sparse import TRUNK, check_coords, resunet_trunk, sparse_conv_train
    if not model.training:
        raise RuntimeError("gmf_amd.train.resunet_train: the model is in eval() mode - call train(), or use forward() for inference")
    if not torch.is_grad_enabled():
        raise RuntimeError("gmf_amd.train.resunet_train: autograd is disabled (torch.no_grad()); the eval forward is model.forward")
    model._check_images(p_image, q_image, p_tokens, q_tokens)
    M, D = check_coords(coords, "resunet_train")
    if D != model.D:
        raise RuntimeError(f"gmf_amd.train.resunet_train: coords have D = {D}, the network was built for D = {model.D}")
    feats = require_cuda_f32(feats, "feats").contiguous()
    if feats.shape != (M, model.in_channels):
        raise RuntimeError(f"gmf_amd.train.resunet_train: `feats` must be [{M}, {model.in_channels}] (got {tuple(feats.shape)})")
    p_tok, q_tok = model._tokens(p_image, q_image, p_tokens, q_tokens)
    plan, where = model._plan(coords)
    counts = plan.counts.tolist()
    if min(counts) < 2:
        raise RuntimeError(f"gmf_amd.train.resunet_train: a level has fewer than 2 rows (counts {counts}); BatchNorm in training "
                           "mode needs more than 1 value per channel")

    def layer(i, xa, xb=None, residual=None, relu=False):
        conv, norm = TRUNK[i][:2]
        m, lvl = where[i]
        y = sparse_conv_train(plan, m, lvl, xa, model.get_submodule(conv).kernel, xb=xb)
        return batchnorm_masked(y, model.get_submodule(norm).bn, plan, lvl, residual=residual, relu=relu)

    image_feat = fusion_layer_train(model.image_fusion, p_tok, q_tok)                  # resunet_new.py:636

    def fuse(s8):                                # resunet_new.py:694-704; rows of s8 past counts[3] are 0
        return fusion_layer_train(model.perceiver_io, image_feat, s8.unsqueeze(0))[0]

    t1, s1 = resunet_trunk(layer, feats, bottleneck=fuse)
    o = sparse_conv_train(plan, None, 0, t1, model.conv1_tr.kernel, xb=s1, relu=True)      # MEF.relu(conv1_tr(ME.cat(...)))
    return sparse_conv_train(plan, None, 0, o, model.final.kernel, bias=model.final.bias)


# =====================================================================================================================
# FCGF's ResUNetBN2C in training mode (GMF_DeepGlobalRegistration_fcgf/model/resunet.py:598-650 with batch-statistics BatchNorm):
# the trunk above without a bottleneck, conv1 on the narrow-input kernels, and the head composed of two 1x1 convolutions and the
# row normalisation (the eval forward's one-launch head, `sparse_head_l2`, has no backward and stays eval-only).


# Not `_Normalize`: that is F.normalize's x / max(||x||, 1e-12); this is FCGF's x / (||x|| + 1e-8) - other bits, another kernel.
class _RowNormEps(torch.autograd.Function):
    """y = x / (||x||_2 + 1e-8) per row of x [rows, C] (resunet.py:647-648; `gmf_rownorm_eps`): dx = dy / s - x <x, dy> / (||x|| s^2)
    with s = ||x|| + 1e-8.  A zero row gives a zero row and a zero gradient."""

    @staticmethod
    def forward(ctx, x):
        x = x.detach().contiguous()
        nrm = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
        y = torch.empty_like(x)
        _call("gmf_rownorm_eps", x, 0, x, None, nrm, y, x.shape[0], x.shape[1])
        ctx.save_for_backward(x, nrm)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, nrm = ctx.saved_tensors
        dy = require_cuda_f32(dy, "grad").contiguous()
        dx = torch.empty_like(x)
        _call("gmf_rownorm_eps", x, 1, x, dy, nrm, dx, x.shape[0], x.shape[1])
        return dx


def normalize_rows_eps(x):
    """FCGF's feature normalisation x / (||x||_2 + 1e-8) on the rows of x [rows, C] (float32, on the device), differentiable."""
    x = require_cuda_f32(x, "x")
    if x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise RuntimeError(f"gmf_amd.train.normalize_rows_eps: `x` must be a non-empty [rows, C] tensor (got {tuple(x.shape)})")
    return _RowNormEps.apply(x)


def fcgf_train(model, coords, feats):
    """The differentiable train-mode forward of a gmf_amd.fcgf.ResUNetBN2C (resunet.py:598-650, batch-statistics BatchNorm):
    features [M, out_channels], aligned with the input rows; several clouds go through as batches of one plan (column 0 of
    coords), as in the eval forward - the BatchNorm statistics then span the whole batch, as MinkowskiEngine's do.  Gradients
    reach the 23 kernels, final.bias and the 21 BatchNorms; every running statistic is updated as torch does.  conv1 runs on the
    narrow-input kernels (`sparse_conv_narrow`, weight gradient `sparse_conv_narrow_wgrad`) when model.narrow_conv1 is set and
    in_channels <= 8, else on the generic ones; `feats` gets no gradient on the narrow path.  The head is conv1_tr (+ ReLU), final
    (+ bias) and, with normalize_feature, y / (||y|| + 1e-8), each its own differentiable call.  Reads the four level counts to the
    host once, to raise as torch's BatchNorm does on a level of fewer than 2 rows."""
    from . import sparse as SP
    from .fcgf import NARROW_MAX_CIN
    from .fcgf import ResUNetBN2C as _FCGF
    what = "gmf_amd.train.fcgf_train"
    if not isinstance(model, _FCGF):
        raise RuntimeError(f"{what}: `model` must be a gmf_amd.fcgf.ResUNetBN2C (got {type(model).__name__})")
    if not model.training:
        raise RuntimeError(f"{what}: the model is in eval() mode - call train(), or use forward() for inference")
    if not torch.is_grad_enabled():
        raise RuntimeError(f"{what}: autograd is disabled (torch.no_grad()); the eval forward is model.forward")
    M, D = SP.check_coords(coords, "fcgf_train")
    if D != model.D:
        raise RuntimeError(f"{what}: coords have D = {D}, the network was built for D = {model.D}")
    feats = require_cuda_f32(feats, "feats").contiguous()
    if feats.shape != (M, model.in_channels):
        raise RuntimeError(f"{what}: `feats` must be [{M}, {model.in_channels}] (got {tuple(feats.shape)})")
    narrow = bool(model.narrow_conv1) and model.in_channels <= NARROW_MAX_CIN and not feats.requires_grad
    plan, where = model._plan(coords, conv1_needs_pairs=narrow)
    counts = plan.counts.tolist()
    if min(counts) < 2:
        raise RuntimeError(f"{what}: a level has fewer than 2 rows (counts {counts}); BatchNorm in training mode needs more than "
                           "1 value per channel")

    def layer(i, xa, xb=None, residual=None, relu=False):
        conv, norm = SP.TRUNK[i][:2]
        m, lvl = where[i]
        W = model.get_submodule(conv).kernel
        if i == 0 and narrow:
            y = SP.sparse_conv_narrow_train(plan, m, lvl, xa, W)
        else:
            y = SP.sparse_conv_train(plan, m, lvl, xa, W, xb=xb)
        return batchnorm_masked(y, model.get_submodule(norm).bn, plan, lvl, residual=residual, relu=relu)

    t1, s1 = SP.resunet_trunk(layer, feats)
    o = SP.sparse_conv_train(plan, None, 0, t1, model.conv1_tr.kernel, xb=s1, relu=True)     # :641-643 MEF.relu(conv1_tr(ME.cat(..)))
    y = SP.sparse_conv_train(plan, None, 0, o, model.final.kernel, bias=model.final.bias)    # :644 final (+ bias)
    return _RowNormEps.apply(y) if model.normalize_feature else y                            # :647-648


# =====================================================================================================================
# The image encoder in train() mode (ResNet-34 -> layer2, GMF_PointDSC/models/resnet.py:36-75,195-216; trained by both
# plugins, PointDSC.py:129-135): every operation a HIP kernel of this library (gmf_amd/csrc/image_train_kernels.hip and the
# BatchNorm / ReLU / column-sum primitives above).  Activations travel as dense NHWC fp32, i.e. as [B * H * W, C] row
# matrices with their (B, H, W) beside them; weights are the nn.Conv2d parameters themselves.
# =====================================================================================================================
_CONV2D_SHAPES = ((3, 64, 7, 2), (64, 64, 3, 1), (128, 128, 3, 1), (64, 128, 3, 2), (64, 128, 1, 2))


def conv2d_out_size(H, W, ks, stride):
    pad = ks // 2
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


class _Conv2dTrain(torch.autograd.Function):
    """y [B*Ho*Wo, cout] = conv2d(x, W) without bias, pad = ks // 2.  x: rows [B*H*W, cin] of a dense NHWC activation with
    geom = (B, H, W), or (the stem) the image itself [B, 3, H, W] in any layout - read through its strides, no gradient."""

    @staticmethod
    def forward(ctx, x, W, geom, stride):
        B, H, Wd = geom
        cout, cin, ks, _ = W.shape
        image = x.dim() == 4
        if not image:
            x = x.contiguous()
        Wc = W.detach().contiguous()
        strides = tuple(x.stride()) if image else (H * Wd * cin, 1, Wd * cin, cin)          # (sb, sc, sh, sw) in elements
        Ho, Wo = conv2d_out_size(H, Wd, ks, stride)
        y = torch.empty((B * Ho * Wo, cout), device=x.device, dtype=torch.float32)
        _call("gmf_conv2d_forward_f32", x, x, *strides, Wc, y, B, H, Wd, cin, cout, ks, stride)
        ctx.geom, ctx.stride, ctx.strides, ctx.image = (B, H, Wd, cin, cout, ks), stride, strides, image
        ctx.save_for_backward(x, Wc)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, Wc = ctx.saved_tensors
        B, H, Wd, cin, cout, ks = ctx.geom
        dy = dy.contiguous()
        dW = torch.empty_like(Wc)
        _call("gmf_conv2d_wgrad", dy, x, *ctx.strides, dy, dW, B, H, Wd, cin, cout, ks, ctx.stride)
        dx = None
        if not ctx.image and ctx.needs_input_grad[0]:
            dx = torch.empty((B * H * Wd, cin), device=dy.device, dtype=torch.float32)
            _call("gmf_conv2d_dgrad", dy, dy, Wc, None, dx, B, H, Wd, cin, cout, ks, ctx.stride)
        return dx, dW, None, None


def conv2d_train(x, conv, geom):
    """`conv`: a bias-free nn.Conv2d of one of the encoder's five shapes -> (rows [B*Ho*Wo, cout], (B, Ho, Wo))."""
    cout, cin, ks, _ = conv.weight.shape
    stride = conv.stride[0]
    if (cin, cout, ks, stride) not in _CONV2D_SHAPES or conv.bias is not None or conv.padding[0] != ks // 2:
        raise NotImplementedError(f"gmf_amd.train: convolution (cin, cout, ks, stride) = {(cin, cout, ks, stride)} is not one of the "
                                  f"image encoder's shapes {_CONV2D_SHAPES} (bias-free, pad = ks // 2)")
    B, H, W = geom
    return _Conv2dTrain.apply(x, conv.weight, geom, stride), (B, *conv2d_out_size(H, W, ks, stride))


class _MaxPoolTrain(torch.autograd.Function):
    """nn.MaxPool2d(3, 2, 1) on rows [B*H*W, C] of an NHWC activation; the backward recomputes each window's argmax from x."""

    @staticmethod
    def forward(ctx, x, geom):
        x = x.contiguous()
        B, H, W = geom
        C = x.shape[1]
        Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((B * Hp * Wp, C), device=x.device, dtype=torch.float32)
        _call("gmf_maxpool3x3s2_forward", x, x, y, B, H, W, C)
        ctx.geom = geom
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        B, H, W = ctx.geom
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        _call("gmf_maxpool3x3s2_backward", x, x, dy, dx, B, H, W, x.shape[1])
        return dx, None


def maxpool_train(x, geom):
    B, H, W = geom
    return _MaxPoolTrain.apply(x, geom), (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1)


def image_encoder_train(enc, image):
    """The differentiable train-mode pass of a gmf_amd ImageEncoder: image [B, 3, H, W] fp32 on a HIP device (any layout, no
    gradient) -> [B, 128, H', W'] (a channels-last view of the NHWC result), the same function as `enc.backbone(image)` in
    train(): batch statistics, running statistics and num_batches_tracked updated per BatchNorm per call, gradients for all 48
    trained tensors.  Walks enc.backbone's own modules and parameters; no host read, capturable after a warm-up."""
    bb = enc.backbone
    require_cuda_f32(image, "image")
    if image.dim() != 4 or image.shape[1] != 3:
        raise ValueError(f"gmf_amd.train: image must be [B, 3, H, W], got {tuple(image.shape)}")
    B, _, H, W = image.shape
    Hc, Wc = conv2d_out_size(H, W, 7, 2) if H > 0 and W > 0 else (0, 0)
    Hf, Wf = (((Hc - 1) // 2 + 1) - 1) // 2 + 1, (((Wc - 1) // 2 + 1) - 1) // 2 + 1      # max-pool, then layer2's stride
    if B < 1 or H < 1 or W < 1 or B * Hf * Wf < 2:
        # torch's BatchNorm raises the same way ("Expected more than 1 value per channel when training"); nothing is launched
        raise ValueError(f"gmf_amd.train: image {tuple(image.shape)} leaves the encoder's last BatchNorms {B * max(Hf, 0) * max(Wf, 0)} "
                         f"row(s) ([{B}, 128, {Hf}, {Wf}]); training-mode batch statistics need more than one")
    x, g = conv2d_train(image.detach(), bb.conv1, (B, H, W))
    x = batchnorm_train(x, bb.bn1, relu=True)
    x, g = maxpool_train(x, g)
    for layer in (bb.layer1, bb.layer2):
        for blk in layer:
            if blk.downsample is None:
                idt = x
            else:
                idt, _ = conv2d_train(x, blk.downsample[0], g)
                idt = batchnorm_train(idt, blk.downsample[1])
            out, g2 = conv2d_train(x, blk.conv1, g)
            out = batchnorm_train(out, blk.bn1, relu=True)
            out, g2 = conv2d_train(out, blk.conv2, g2)
            x, g = batchnorm_train(out, blk.bn2, relu=True, residual=idt), g2          # resnet.py:59-75
    Bo, Ho, Wo = g
    return x.view(Bo, Ho, Wo, x.shape[1]).permute(0, 3, 1, 2)
