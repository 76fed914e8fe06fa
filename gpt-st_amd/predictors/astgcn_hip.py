"""The ASTGCN predictor on HIP (csrc/astgcn.hip, csrc/stgcn.hip), forward and backward: what ``ASTGCN(..., backend="hip")`` runs on CUDA fp32 input.

Channels-last as for the other predictors: the embedding arrives as (B, T, N, C), every activation is (B*T*N rows, C) with row (b T + t) N + n, a
temporal tap is a row offset of +-N rows — no permute is materialised.  The module's parameters stay in the reference's layout (so checkpoints
load unchanged); each forward repacks the few KB of weights into the kernels' GEMM form with plain tensor ops, which also carries the packed
gradients back to the parameters.

    masked mix      Z[(b,t,n), k c + ch] = sum_m T_k[m,n] S[b,m,n] x[(b,t,m), ch] (ops.astgcn_attmix: every sample mixes with ITS graph, formed
                    in LDS), then relu(Z Theta) with Theta = [theta_k]_k stacked (ops.stgcn_tapgemm).  Backward: dTheta = dPre^T Z (stgcn_wgrad),
                    G = dPre Theta, dx = the reduce form of the mix on G, dS = ops.astgcn_attgrad(x, G).
    time conv       relu(sum over the taps (-1, 0, 1) of g W_j + b + R) with R = the 1x1 residual conv of x: two ops.stgcn_tapgemm launches, the
                    second takes R as ``res=``.  Backward: stgcn_gate_bwd, stgcn_wgrad and the mirrored tap GEMM.
    LayerNorm       over the c values of each row: ops.astgcn_rowln_*.
    kept in torch   the two attention score chains (x_TAt is not materialised: the spatial attention needs only a[b,n,f] = sum_t x (E W1)[t] and
                    rhs[b,t',n] = sum_t E[t,t'] (x W3)[b,t,n]), Vs sigmoid(.), the column softmax, and final_conv (as one matmul over (T, F)).  The score product is N^3 per
                    sample (0.6 GFLOP per block against 8.5 for the mix).  S enters the autograd function below as an input with a gradient.

Kept for the backward: the block input, Z, the relu outputs, the LayerNorm's mean and rstd.  Without a backward to serve (no_grad, eval mode: the
module passes keep = False) nothing is kept.
"""
import torch
import torch.nn.functional as F

from .. import _C, ops
from ..ops import ACT_NONE, ACT_RELU
from . import rows_hip
from .rows_hip import TapFn, is_hip_input, widths_ok


class _MixFn(torch.autograd.Function):
    """y = relu(sum_k ((T_k * S_b)^T x) theta_k);  Theta (co, ks c) with column k c + i = theta_k[i, :]"""

    @staticmethod
    def forward(ctx, x, S, Theta, Tp, T, N, keep):
        keep = keep and any(ctx.needs_input_grad)
        c = x.shape[1]
        S = S.contiguous()
        Z = ops.astgcn_attmix(Tp, S, x, T, c, reduce=False)
        y = ops.stgcn_tapgemm(Z, Theta, None, (0,), ACT_RELU, T, N)
        if keep:
            ctx.cfg = (T, N)
            ctx.save_for_backward(x, S, Z, y, Theta, Tp)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, S, Z, y, Theta, Tp = ctx.saved_tensors
        T, N = ctx.cfg
        c = x.shape[1]
        dPre = ops.stgcn_gate_bwd(dy.contiguous(), ACT_RELU, out=y)
        dx = dS = dTheta = None
        if ctx.needs_input_grad[2]:
            dTheta, _ = ops.stgcn_wgrad(dPre, Z, (0,), T, N, want_bias=False)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            G = ops.stgcn_tapgemm(dPre, Theta.t().contiguous(), None, (0,), ACT_NONE, T, N)               # (rows, ks c): G_k = dPre theta_k^T
            if ctx.needs_input_grad[0]:
                dx = ops.astgcn_attmix(Tp, S, G, T, c, reduce=True)
            if ctx.needs_input_grad[1]:
                dS = ops.astgcn_attgrad(Tp, x, G, S.shape[0], T, N)
        return dx, dS, dTheta, None, None, None, None


class _RowLNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, keep):
        keep = keep and any(ctx.needs_input_grad)
        y, mean, rstd = ops.astgcn_rowln_fwd(x, gamma, beta, eps, keep=keep)
        if keep:
            ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        dx = ops.astgcn_rowln_bwd(dy, x, gamma, mean, rstd) if ctx.needs_input_grad[0] else None
        dg = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dg, db = ops.astgcn_rowln_bwd_param(dy, x, mean, rstd)
        return dx, dg, db, None, None


def padded_graph(model):
    """the polynomials zero-padded to 16-node tiles"""
    return rows_hip.padded_graph(model, model.cheb, "_tp_cache", False)


def attention(blk, x4):
    """S (B, N, N) of a block from x4 (B, T, N, F), in torch: the reference's two score chains without x_TAt.  With E the temporal attention,
    x_TAt[b,n,f,t'] = sum_t x[b,t,n,f] E[b,t,t'], and the spatial scores need only (x_TAt W1) = sum_t x (E W1)[t] and (W3 x_TAt) = E^T (x W3)."""
    ta, sa = blk.TAt, blk.SAt
    lhs = torch.einsum("btnf,n->btf", x4, ta.U1) @ ta.U2                       # (B, T, N)
    xu3 = x4 @ ta.U3                                                           # (B, T, N)
    E = F.softmax(torch.matmul(ta.Ve, torch.sigmoid(lhs @ xu3.transpose(1, 2) + ta.be)), dim=1)      # (B, T, T)
    a = torch.einsum("btnf,bt->bnf", x4, E @ sa.W1)                            # (B, N, F)
    rhs = E.transpose(1, 2) @ (x4 @ sa.W3)                                     # (B, T', N)
    return F.softmax(torch.matmul(sa.Vs, torch.sigmoid((a @ sa.W2) @ rhs + sa.bs)), dim=1)


def pack_theta(blk):
    """[theta_k]_k as the tap GEMM's weight (co, ks c): column k c + i = theta_k[i, :]"""
    return torch.cat([th.t() for th in blk.cheb_conv_SAt.Theta], dim=1).contiguous()


def pack_time_conv(blk):
    """(co, ci, 1, 3) -> (co, 3 ci), tap-major columns: the taps (-1, 0, 1)"""
    w = blk.time_conv.weight
    return w[:, :, 0, :].permute(0, 2, 1).reshape(w.shape[0], 3 * w.shape[1]).contiguous()


def head(model, h):
    """final_conv on h (B, T, N, F) as one contraction over (T, F) — the convolution library's default algorithms are not bit-repeatable on this
    GPU, a matmul is — then the reference's reshape and transpose (ASTGCN.py:309-311)"""
    fc = model.final_conv
    y = torch.einsum("btnf,otf->bon", h, fc.weight[:, :, 0, :]) + fc.bias[None, :, None]
    return y.reshape(h.shape[0], model.num_for_predict, model.dim_out, -1).transpose(-1, -2)


def supported(model, x):
    """the HIP path serves: CUDA fp32 input, channel widths that are multiples of 16 up to 128, K <= 3, time_strides == 1, and a node count whose
    masked tiles and slab fit the LDS of a CU (N <= 320)"""
    if not is_hip_input(x):
        return False
    blk0 = model.BlockList[0]
    ks, n = model.cheb.shape[0], model.cheb.shape[1]
    if model.time_strides != 1 or ks > 3 or x.shape[2] != n or x.shape[-1] != blk0.residual_conv.in_channels:
        return False
    if x.shape[1] != model.final_conv.in_channels or x.shape[1] < 2:
        return False
    if n > 320:                                                            # the masked tiles and the slab of gptst_astgcn_attmix: 160 KB of LDS
        return False
    widths = [x.shape[-1]]
    for blk in model.BlockList:
        widths += [blk.time_conv.in_channels, blk.time_conv.out_channels]
    return widths_ok(widths)


def forward(model, x, keep=True):
    """predictors.astgcn.ASTGCN.forward on the kernels: x (B, T, N, dim_in) -> (B, num_for_predict, N, dim_out).  keep = False (no_grad, eval
    mode): nothing is saved for a backward"""
    _C.lib()
    B, T, N, _ = x.shape
    tp = padded_graph(model)
    h = x.contiguous()
    for blk in model.BlockList:
        rows = h.view(B * T * N, h.shape[-1])
        S = attention(blk, h)
        g = _MixFn.apply(rows, S, pack_theta(blk), tp, T, N, keep)
        rc = blk.residual_conv
        R = TapFn.apply(rows, rc.weight.view(rc.out_channels, rc.in_channels).contiguous(), rc.bias.contiguous(), None, (0,), ACT_NONE, 0, T, N, keep)
        y = TapFn.apply(g, pack_time_conv(blk), blk.time_conv.bias.contiguous(), R, (-1, 0, 1), ACT_RELU, R.shape[1], T, N, keep)
        y = _RowLNFn.apply(y, blk.ln.weight.contiguous(), blk.ln.bias.contiguous(), blk.ln.eps, keep)
        h = y.view(B, T, N, y.shape[-1])
    return head(model, h)
