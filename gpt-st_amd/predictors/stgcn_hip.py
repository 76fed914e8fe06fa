"""The STGCN predictor on HIP (csrc/stgcn.hip), forward and backward: what ``STGCN(..., backend="hip")`` runs on CUDA fp32 input.

Channels-last throughout: the embedding arrives as (B, T, N, C), every activation is (B*T*N rows, C), a temporal tap is a row offset of
+-N rows, the LayerNorm weight [N, C] matches a (b, t) slab of rows as stored — no permute is materialised.  The module's parameters stay in
the reference's layout (so checkpoints load unchanged); each forward repacks the few KB of weights into the kernels' GEMM form with plain
tensor ops, which also carries the packed gradients back to the parameters.

    temporal conv   one launch (ops.stgcn_tapgemm): the kt taps and the 1x1 align as K-blocks of one GEMM, GLU / relu / sigmoid and the
                    residual in the epilogue.  Backward: dPre (stgcn_gate_bwd), dW / db / align gradients (stgcn_wgrad: row-split partials),
                    dX = the mirrored tap GEMM of dPre with the transposed weights.
    graph conv      Z = [L_k X]_k (stgcn_nodemix), Y = relu(Z Theta + b + X) (stgcn_tapgemm).  Backward: dTheta = Z^T dPre (stgcn_wgrad),
                    G = dPre Theta^T, dX = sum_k L_k^T G_k + dPre (stgcn_nodemix, reduce).
    LayerNorm       stgcn_ln_fwd / stgcn_ln_bwd over (N, C) per (b, t).
    fc              c -> dim_out (33 MFLOP): a torch matmul on the (rows, c) view.

Kept for the backward: every layer's input (it is the previous layer's output), the GLU's sigmoid(Q) and P + res, the graph convolution's Z,
the LayerNorm's mean and rstd.  Without a backward to serve (no_grad, eval mode: the module passes keep = False) nothing is kept or written for one, and the same launches run.
"""
import torch

from .. import _C, ops
from ..ops import ACT_GLU, ACT_NONE, ACT_RELU, ACT_SIGMOID
from .rows_hip import LNFn, TapFn, is_hip_input, padded_graph, widths_ok

_ACT = {"GLU": ACT_GLU, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID}


class _SConvFn(torch.autograd.Function):
    """y = relu(sum_k (L_k x) theta_k + b + x);  Theta (c, ks * c) with column k c + i = theta[i, :, k]"""

    @staticmethod
    def forward(ctx, x, Theta, b, Lp, LpT, T, N, keep):
        keep = keep and any(ctx.needs_input_grad)
        c = x.shape[1]
        Z = ops.stgcn_nodemix(Lp, x, N, c, reduce=False)
        y = ops.stgcn_tapgemm(Z, Theta, b, (0,), ACT_RELU, T, N, res=x, res_w=c)
        if keep:
            ctx.cfg = (T, N)
            ctx.save_for_backward(Z, y, Theta, LpT)
        return y

    @staticmethod
    def backward(ctx, dy):
        Z, y, Theta, LpT = ctx.saved_tensors
        T, N = ctx.cfg
        c = y.shape[1]
        dPre = ops.stgcn_gate_bwd(dy.contiguous(), ACT_RELU, out=y)
        dTheta = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dTheta, db = ops.stgcn_wgrad(dPre, Z, (0,), T, N)
        if ctx.needs_input_grad[0]:
            G = ops.stgcn_tapgemm(dPre, Theta.t().contiguous(), None, (0,), ACT_NONE, T, N)               # (rows, ks c): G_k = dPre theta_k^T
            dx = ops.stgcn_nodemix(LpT, G, N, c, reduce=True, res=dPre)
        return dx, dTheta, db, None, None, None, None, None


def _tconv(m, x, T, N, keep=True):
    """predictors.stgcn._TConv on rows: the conv's taps (and the 1x1 align as one more centre tap) packed tap-major into one GEMM weight"""
    w = m.conv.weight                                                   # (cw, ci, kt, 1)
    cw, ci, kt = w.shape[0], w.shape[1], w.shape[2]
    W = w[..., 0].permute(0, 2, 1).reshape(cw, kt * ci)
    b = m.conv.bias
    taps = tuple(j - (kt - 1) // 2 for j in range(kt))
    res_w = min(ci, m.c_out)
    if ci > m.c_out:                                                    # 1x1 down: its rows feed the P half only
        wa, ba = m.align.conv1x1.weight.view(m.c_out, ci), m.align.conv1x1.bias
        if cw > m.c_out:
            wa, ba = torch.cat([wa, wa.new_zeros(cw - m.c_out, ci)]), torch.cat([ba, ba.new_zeros(cw - m.c_out)])
        W, b, taps, res_w = torch.cat([W, wa], 1), b + ba, taps + (0,), 0
    return TapFn.apply(x, W.contiguous(), b.contiguous(), None, taps, _ACT[m.act], res_w, T, N, keep)


def _sconv(m, x, T, N, keep=True):
    c_in, c_out, ks = m.theta.shape
    Theta = m.theta.permute(1, 2, 0).reshape(c_out, ks * c_in).contiguous()
    lp, lpt = padded_graph(m, m.Lk, "_lp_cache", True)
    return _SConvFn.apply(x, Theta, m.b.reshape(c_out).contiguous(), lp, lpt, T, N, keep)


def _ln(ln, x, units, keep=True):
    return LNFn.apply(x, ln.weight.contiguous(), ln.bias.contiguous(), units, ln.eps, keep)


def supported(model, x):
    """the HIP path serves: CUDA fp32 input, channel widths that are multiples of 16 up to 128, Kt and outputl_ks of 1 or 3, Ks <= 3, and
    inactive dropout (drop_prob == 0 or eval mode)"""
    if not is_hip_input(x):
        return False
    blocks = (model.st_conv1, model.st_conv2)
    widths = [x.shape[-1]]
    for blk in blocks:
        widths += [blk.tconv1.c_out, blk.tconv2.c_out]
        if blk.dropout.p != 0 and model.training:
            return False
        if blk.tconv1.conv.kernel_size[0] not in (1, 3) or blk.tconv2.conv.kernel_size[0] not in (1, 3) or blk.sconv.theta.shape[2] > 3:
            return False
        if blk.sconv.theta.shape[0] != blk.sconv.theta.shape[1] or blk.sconv.Lk.shape[1] != x.shape[2]:
            return False
    if model.output.tconv1.conv.kernel_size[0] not in (1, 3) or x.shape[-1] != model.st_conv1.tconv1.conv.in_channels:
        return False
    return widths_ok(widths)


def forward(model, x, keep=True):
    """predictors.stgcn.STGCN.forward on the kernels: x (B, T, N, dim_in) -> (B, T, N, dim_out).  keep = False (no_grad, eval mode): no launch writes
    anything for a backward and nothing is saved"""
    _C.lib()
    B, T, N, C = x.shape
    h = x.contiguous().view(B * T * N, C)
    for blk in (model.st_conv1, model.st_conv2):
        h = _tconv(blk.tconv1, h, T, N, keep)
        h = _sconv(blk.sconv, h, T, N, keep)
        h = _tconv(blk.tconv2, h, T, N, keep)
        h = _ln(blk.ln, h, B * T, keep)
    head = model.output
    h = _tconv(head.tconv1, h, T, N, keep)
    h = _ln(head.ln, h, B * T, keep)
    h = _tconv(head.tconv2, h, T, N, keep)
    fc = head.fc.conv
    y = torch.addmm(fc.bias, h, fc.weight.view(fc.out_channels, -1).t())
    return y.view(B, T, N, fc.out_channels)
