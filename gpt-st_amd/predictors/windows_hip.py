"""What the two window predictors on HIP share (stsgcn_hip.py: windows of three frames, stfgnn_hip.py: of four): the layer function over the
kernels of csrc/stsgcn.hip and the mix of either predictor, the checks both ``supported`` make, and the gathering of a layer's stacked weights.

A layer over T frames has W = T - span + 1 windows of ``span`` frames.  Inside it activations are window-expanded, rows (b, w, k, n) in groups of
R = span N with block (w, k) standing for frame w + k; the last operation's output and the running max are rows (b, w, n).  The two predictors
differ in the span and in the mix: which ``ops`` entry it is and how many graphs it takes (``Mix`` below).

Every launch goes through the ``ops`` module's attribute at call time (rows_hip), so a test that replaces ``ops.stsgcn_wingemm`` sees it; a
``Mix.call`` looks its entry up the same way.
"""
from typing import Callable, NamedTuple

import torch

from .. import ops
from ..ops import ACT_GLU, ACT_NONE
from .rows_hip import is_hip_input, widths_ok

MAX_NODES = 448            # the mix keeps a (Np, 36) slab of a block in the 64 KB of LDS a launch gets by default


class Mix(NamedTuple):
    """call(graphs, X, mode, B, T, N) -> the mixed rows; fwd: the graph operands of the forward, adj: their transposes, for the adjoints"""
    call: Callable
    fwd: tuple
    adj: tuple


class LayerFn(torch.autograd.Function):
    """best (B W N, co) = max over the J operations of a layer; H (B T N, ci) with the embeddings added; wb = W_0, b_0, W_1, b_1, ...: the stacked
    weights (W | 1, 2 co, ci) and biases"""

    @staticmethod
    def forward(ctx, H, mix, span, B, T, N, keep, *wb):
        keep = keep and any(ctx.needs_input_grad)
        W, J = T - span + 1, len(wb) // 2
        co = wb[0].shape[1] // 2
        best = H.new_empty(B * W * N, co)
        which = torch.empty(B * W * N, co, device=H.device, dtype=torch.int32) if keep else None
        cur, saved = H, []
        for j in range(J):
            last = j == J - 1
            Z = mix.call(mix.fwd, cur, ops.MIX_F2E if j == 0 else ops.MIX_E2M if last else ops.MIX_E2E, B, T, N)            # (J >= 2: supported())
            R = N if last else span * N
            out = ops.stsgcn_wingemm(Z, wb[2 * j], wb[2 * j + 1], ACT_GLU, B, W, R, N, keep=keep, best=best, which=which, opj=j)
            if keep:
                cur, S, A = out
                saved += [Z, S, A]
            else:
                cur = out
        if keep:
            ctx.cfg = (mix, span, B, T, N, J, len(ctx.needs_input_grad) - len(wb))      # the last: where wb starts among forward's arguments
            ctx.save_for_backward(which, *wb[0::2], *saved)
        return best

    @staticmethod
    def backward(ctx, dBest):
        mix, span, B, T, N, J, wb0 = ctx.cfg
        which = ctx.saved_tensors[0]
        Ws, saved = ctx.saved_tensors[1:1 + J], ctx.saved_tensors[1 + J:]
        W = T - span + 1
        dBest = dBest.contiguous()
        grads, up = [None] * (2 * J), None
        for j in range(J - 1, -1, -1):
            Z, S, A = saved[3 * j:3 * j + 3]
            R = N if j == J - 1 else span * N
            dPre = ops.stsgcn_gate_bwd(up, dBest, which, j, S, A, B, W, R, N)
            if ctx.needs_input_grad[wb0 + 2 * j] or ctx.needs_input_grad[wb0 + 2 * j + 1]:
                dW, db = ops.stsgcn_winwgrad(dPre, Z, B, W, R)
                if Ws[j].shape[0] == 1 and W > 1:                       # one weight for all windows (STSGCN "sharing"): the windows' gradients add up, in order
                    dW, db = dW.sum(0, keepdim=True), db.sum(0, keepdim=True)
                grads[2 * j], grads[2 * j + 1] = dW, db
            if j == 0 and not ctx.needs_input_grad[0]:
                up = None
                break
            dZ = ops.stsgcn_wingemm(dPre, Ws[j].transpose(1, 2).contiguous(), None, ACT_NONE, B, W, R, N)
            up = mix.call(mix.adj, dZ, ops.MIX_E2F if j == 0 else ops.MIX_M2E if j == J - 1 else ops.MIX_E2E, B, T, N)
        return (up,) + (None,) * (wb0 - 1) + tuple(grads)


def stacked_weights(lay, J):
    """W_0, b_0, W_1, b_1, ... of a layer's J operations, as LayerFn takes them"""
    wb = []
    for j in range(J):
        wb += lay.stacked(j)
    return wb


def supported(model, x, fe, window, filters):
    """the checks the two predictors share: CUDA fp32 4-D input of ``window`` frames, the module's node count and the first embedding's (``fe``)
    input width; GLU, no mask; per layer (``filters``: its operations' widths) at least two operations of equal widths; channel widths that are
    multiples of 16 up to 128; a node count whose slab fits the default LDS of a launch (N <= 448)"""
    if not is_hip_input(x) or model.activation != "GLU" or model.use_mask:
        return False
    if x.shape[1] != window or x.shape[2] != model.num_nodes or x.shape[3] != fe.in_features or model.num_nodes > MAX_NODES:
        return False
    widths = [fe.in_features, fe.out_features]
    for f in filters:
        if len(f) < 2 or len(set(f)) != 1:
            return False
        widths += f
    return widths_ok(widths)
