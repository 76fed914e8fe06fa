"""The STGODE predictor on HIP (csrc/stgode.hip), forward and backward: what ``STGODE(..., backend="hip")`` runs on CUDA fp32 input.

Channels-last as for the other predictors: the embedding arrives as (B, T, N, C), every activation is rows (b, t, n) x C, nothing is permuted.
A block is BN_nodes(relu(step(relu(X)))) — its temporal convolutions never run (predictors/stgode.py) — and the whole trunk, all 2 n_layers
branches of two blocks and the max over them, is ONE autograd function, because the branches share the running max and its winner index.

    step            z = relu(3 alpha_n (A t)[n] + 6 t W + 6 sum_k W2[k, tau] t[k] - 11 t), t = relu(X): one launch over the batch and all frames
                    (ops.stgode_step: relu on load, node product on the LDS slab, channel product, time mix, row scale and relu in the epilogue).
                    alpha = sigmoid(alpha), W = (w clamp(d)) w^T and W2 are torch's (ODEFunc.mats): tiny tensors, and autograd carries their
                    gradients back to alpha, w, d, w2, d2 through the sigmoid and the clamp.
    batch norm      the node is the channel.  Training: ops.stgode_bn_stats (per-split mean and squared deviations, two passes) then
                    ops.stgode_bn_apply, which folds the splits (Chan, double, fixed order), normalises, updates the running statistics as torch
                    does, and — for the last block of a branch — folds the result into the running max (strictly greater replaces: exact ties
                    stay with the lowest branch) instead of writing it.  Eval: the apply alone, on the running statistics.
    backward        per block, last to first: the batch norm's two per-node sums and then g = dz [z > 0] (ops.stgode_bn_bwd, two launches; the
                    last block of a branch reads its upstream gradient as dBest [which == branch]); dW = 6 t^T g (ops.stgode_wgrad), dW2 and
                    dalpha (ops.stgode_reduce); dX = the SAME step kernel with A^T, W^T, W2 for W2^T, alpha on the source rows, the coefficient
                    -17 in place of -11 (x0 is detached in the reference: the backward is not the derivative of the forward) and the mask
                    [X > 0].  The branches' input gradients are summed by torch in branch order.
    kept in torch   the small-parameter chains above and the heads (STGODE.head).

Project launches per block: 3 forward (step, stats, apply; 2 outside training mode) + 5 backward (two of the batch norm, weight gradient,
reductions, step) = 8 in a training step, whatever B, T and N; a branch's first block skips its backward step when the input needs no gradient.

Kept for the backward, per block: its input X (the previous block's output, or x), z, the node product A t (for dalpha: recomputing it would
cost a second node product, the dominant part of the step; see DESIGN.md for the memory this takes) and the batch statistics; per model the
winner index.  Without a backward to serve (no_grad, eval mode: keep = False) nothing is kept and no product is written.
"""
import torch

from .. import _C, ops
from . import rows_hip
from .rows_hip import is_hip_input, pad16, widths_ok

MAX_NODES = 448            # the step keeps a (Np, 36) slab of a frame in the 64 KB of LDS a launch gets by default
MAX_T = 32                 # a row of the time-mix matrix in LDS (csrc/stgode.hip ST_MAX_T)
FWD = (3.0, 6.0, 6.0, -11.0)        # node, channel, time, self: z = x + 6 f with x0 = x
BWD = (3.0, 6.0, 6.0, -17.0)        # ... with x0 detached


class _TrunkFn(torch.autograd.Function):
    """best (B T N, C) = max over the branches of their two blocks; x (B T N, C); cfg = (B, T, N, [(Lp, Lpt, [batch_norm, ...])] per branch,
    keep); params = (alpha, W, W2, gamma, beta) per block in branch order"""

    @staticmethod
    def forward(ctx, x, cfg, *params):
        B, T, N, branches, keep = cfg
        keep = keep and any(ctx.needs_input_grad)
        best = torch.empty_like(x)
        which = torch.empty(x.shape, device=x.device, dtype=torch.int32) if keep else None
        saved, k = [], 0
        for bi, (Lp, _, bns) in enumerate(branches):
            h = x
            for j, bn in enumerate(bns):
                alpha, W, W2, gamma, beta = (p.contiguous() for p in params[5 * k:5 * k + 5])
                out = ops.stgode_step(Lp, h, W, W2.t().contiguous(), B, T, N, FWD, oscale=alpha, relu_in=True, relu_out=True, keep_at=keep)
                z, AT = out if keep else (out, None)
                last = j == len(bns) - 1
                part = ops.stgode_bn_stats(z, B, T, N) if bn.training else None
                y, mean, rstd = ops.stgode_bn_apply(z, part, gamma, beta, bn.running_mean, bn.running_var, bn.training, bn.momentum, bn.eps, B, T, N,
                                                    keep=keep, best=best if last else None, which=which if last else None, idx=bi, want_y=not last)
                if bn.training:
                    bn.num_batches_tracked.add_(1)
                if keep:
                    saved += [h, z, AT, mean, rstd, alpha, W, W2, gamma]
                h, k = y, k + 1
        if keep:
            ctx.cfg = cfg
            ctx.save_for_backward(which, *saved)
        return best

    @staticmethod
    def backward(ctx, dBest):
        B, T, N, branches, _ = ctx.cfg
        which, saved = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        dBest = dBest.contiguous()
        nblk = len(saved) // 9
        grads, dx, k = [None] * (5 * nblk), None, 0
        for bi, (_, Lpt, bns) in enumerate(branches):
            up = None
            for j in range(len(bns) - 1, -1, -1):
                X, z, AT, mean, rstd, alpha, W, W2, gamma = saved[9 * (k + j):9 * (k + j) + 9]
                if up is None:
                    g, dgam, dbet = ops.stgode_bn_bwd(None, z, gamma, mean, rstd, B, T, N, dBest=dBest, which=which, idx=bi)
                else:
                    g, dgam, dbet = ops.stgode_bn_bwd(up, z, gamma, mean, rstd, B, T, N)
                d2, da = ops.stgode_reduce(g, X, AT, B, T, N)
                grads[5 * (k + j):5 * (k + j) + 5] = [3.0 * da, 6.0 * ops.stgode_wgrad(g, X), 6.0 * d2, dgam, dbet]
                if j > 0 or ctx.needs_input_grad[0]:
                    up = ops.stgode_step(Lpt, g, W.t().contiguous(), W2, B, T, N, BWD, sscale=alpha, mask=X)
            if ctx.needs_input_grad[0]:
                dx = up if dx is None else dx + up
            k += len(bns)
        return (dx, None) + tuple(grads)


def padded_graphs(model):
    """[(A, A^T)] zero-padded to 16-node tiles: the spatial pair, the semantic pair"""
    sp, spt = rows_hip.padded_graph(model, model.A_sp, "_go_cache_sp", True)
    se, set_ = rows_hip.padded_graph(model, model.A_se, "_go_cache_se", True)
    return (sp[0], spt[0]), (se[0], set_[0])


def supported(model, x):
    """the HIP path serves: CUDA fp32 4-D input of the module's window, node count and block width; every temporal net of the module in its
    identity form (no downsample: dim_in equal to out_channels[-1] — the ``-mode ori`` sizes run the convolutions and fall back); a width that
    is a multiple of 16 up to 128; T <= 32; a node count whose slab fits the default LDS of a launch (N <= 448); batch norms with their
    affine, their running statistics and a momentum"""
    C = model.out_channels[-1]
    if not is_hip_input(x) or x.shape[1] != model.window or x.shape[2] != model.num_nodes or x.shape[3] != C:
        return False
    if model.window > MAX_T or pad16(model.num_nodes) > MAX_NODES or not widths_ok([C]):
        return False
    for seq, _ in model.branches():
        for blk in seq:
            bn, f = blk.batch_norm, blk.odeg.odeblock.odefunc
            if not blk.identity_form() or not bn.affine or not bn.track_running_stats or bn.momentum is None:
                return False
            if tuple(f.w.shape) != (C, C) or tuple(f.w2.shape) != (model.window, model.window) or f.alpha.shape[0] != model.num_nodes:
                return False
    return True


def trunk(model, x, keep=True):
    """x (B, T, N, C) -> best (B T N, C): every branch's two blocks and the max over the branches"""
    _C.lib()
    B, T, N, C = x.shape
    (sp, spt), (se, set_) = padded_graphs(model)
    branches, params = [], []
    for seq, A in model.branches():
        g = (sp, spt) if A is model.A_sp else (se, set_)
        branches.append((g[0], g[1], [blk.batch_norm for blk in seq]))
        for blk in seq:
            params += [*blk.odeg.odeblock.odefunc.mats(), blk.batch_norm.weight, blk.batch_norm.bias]
    return _TrunkFn.apply(x.contiguous().view(B * T * N, C), (B, T, N, branches, keep), *params)


def forward(model, x, keep=True):
    """predictors.stgode.STGODE.forward on the kernels: x (B, T, N, C) -> (B, horizon, N, dim_out).  keep = False (no_grad, eval mode): nothing is
    saved for a backward"""
    return model.head(trunk(model, x, keep).view(x.shape))
