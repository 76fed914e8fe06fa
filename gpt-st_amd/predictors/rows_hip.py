"""The row layer the HIP predictors share (stgcn_hip.py, tgcn_hip.py, mtgnn_hip.py, astgcn_hip.py): what two or more of them run on the
kernels of csrc/stgcn.hip, in the channels-last layout they all use — an activation is (B*T*N rows, C) with row (b T + t) N + n, a temporal
tap is a row offset of +-N rows.

    TapFn           the tap GEMM with its epilogue, and its backward: dPre (stgcn_gate_bwd), dW / db (stgcn_wgrad: row-split partials),
                    dX = the mirrored tap GEMM of dPre with the transposed weights (``mirror``)
    LNFn            LayerNorm over each unit's values: stgcn_ln_fwd / stgcn_ln_bwd / stgcn_ln_bwd_param
    padded_graph    a graph zero-padded to 16-node tiles, cached on the module that owns it
    the checks every ``supported`` makes: is_hip_input, widths_ok, and nodemix_fits where the node mix's slab bounds N

Every launch goes through the ``ops`` module's attribute at call time, so a test that replaces ``ops.stgcn_tapgemm`` sees it.
"""
import torch

from .. import ops
from ..ops import ACT_GLU, ACT_NONE

LDS_MAX = 160 * 1024


def pad16(n):
    return 16 * ((n + 15) // 16)


def nodemix_fits(N):
    """the node mix keeps a (Np, 36) slab of the unit in LDS"""
    return pad16(N) * 36 * 4 <= LDS_MAX


def is_hip_input(x):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4


def widths_ok(widths):
    """every channel width a multiple of 16 in 16 .. 128"""
    return all(w % 16 == 0 and 16 <= w <= 128 for w in widths)


def mirror(W, ntap):
    """W (cw, ntap * ci) -> (ci, ntap * cw) with block j = W_j^T: the weight of the data backward"""
    cw = W.shape[0]
    return W.view(cw, ntap, -1).permute(2, 1, 0).reshape(-1, ntap * cw).contiguous()


def padded_graph(owner, graph, cache_attr, transposed):
    """``graph`` (ks, N, N) or (N, N) zero-padded to 16-node tiles, (ks | 1, Np, Np) — with its transpose when ``transposed``: built when
    the owner's graph is another tensor than last time, or was written to"""
    c = getattr(owner, cache_attr, None)
    if c is None or c[0] is not graph or c[1] != graph._version:
        g3 = graph if graph.dim() == 3 else graph[None]
        n = g3.shape[1]
        lp = graph.new_zeros(g3.shape[0], pad16(n), pad16(n))
        lp[:, :n, :n] = g3
        c = (graph, graph._version, lp, lp.transpose(1, 2).contiguous() if transposed else None)
        setattr(owner, cache_attr, c)
    return (c[2], c[3]) if transposed else c[2]


class TapFn(torch.autograd.Function):
    """y = act(sum_j x[t + taps[j]] W_j + b + residual);  W (co | 2 co (GLU), len(taps) * ci).  The residual is ``res`` (rows, res_w), which
    takes dPre as its gradient, or with res = None and res_w > 0 the input's own first res_w columns, whose gradient rides in the epilogue
    of the mirrored GEMM."""

    @staticmethod
    def forward(ctx, x, W, b, res, taps, act, res_w, T, N, keep):
        keep = keep and any(ctx.needs_input_grad)
        own = res is None and res_w > 0
        r = x if own else res
        S = A = None
        if act == ACT_GLU and keep:
            y, S, A = ops.stgcn_tapgemm(x, W, b, taps, act, T, N, res=r, res_w=res_w, keep=True)
        else:
            y = ops.stgcn_tapgemm(x, W, b, taps, act, T, N, res=r, res_w=res_w)
        if keep:
            ctx.cfg = (taps, act, res_w if own else 0, T, N)
            ctx.save_for_backward(x, W, S, A, None if act in (ACT_GLU, ACT_NONE) else y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W, S, A, y = ctx.saved_tensors
        taps, act, own_w, T, N = ctx.cfg
        dPre = dy.contiguous() if act == ACT_NONE else ops.stgcn_gate_bwd(dy.contiguous(), act, out=y, S=S, A=A)
        dW = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dW, db = ops.stgcn_wgrad(dPre, x, taps, T, N)
        if ctx.needs_input_grad[0]:
            dx = ops.stgcn_tapgemm(dPre, mirror(W, len(taps)), None, tuple(-t for t in taps), ACT_NONE, T, N, res=dPre if own_w > 0 else None,
                                   res_w=own_w)
        return dx, dW, db, (dPre if ctx.needs_input_grad[3] else None), None, None, None, None, None, None


class LNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, units, eps, keep):
        keep = keep and any(ctx.needs_input_grad)
        y, mean, rstd = ops.stgcn_ln_fwd(x, gamma, beta, units, eps, keep=keep)
        if keep:
            ctx.units = units
            ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        dx = ops.stgcn_ln_bwd(dy, x, gamma, mean, rstd, ctx.units) if ctx.needs_input_grad[0] else None
        dg = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dg, db = (g.view_as(gamma) for g in ops.stgcn_ln_bwd_param(dy, x, mean, rstd, ctx.units))
        return dx, dg, db, None, None, None
