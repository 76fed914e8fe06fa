"""The STFGNN predictor on HIP (csrc/stfgnn.hip, csrc/stsgcn.hip, csrc/mtgnn.hip, csrc/stgcn.hip), forward and backward: what
``STFGNN(..., backend="hip")`` runs on CUDA fp32 input.

Channels-last as for the other predictors: the embedding arrives as (B, T, N, C), every activation is rows x C, nothing is permuted.  A layer over
T frames has W = T - 3 windows of four frames; inside it activations are window-expanded, rows (b, w, k, n) with block (w, k) standing for frame
w + k, and the last operation's output, the running max and the gated branch are rows (b, w, n) — already the next layer's (b, t, n).

    operation j     Z_j = mix(source) with the (4N, 4N) fusion graph as its blocks S^ and D (graph.stfgnn_blocks),
                        mix(X)_0 = mix(X)_3 = D (X_0 + X_3) + X_1 + X_2,    mix(X)_k = S^ X_k + the other three blocks, k = 1, 2
                    (ops.stfgnn_mix; the matrix is never formed: the first operation reads the frames directly, the last one forms block 1 only and
                    does not touch D), then GLU(Z_j W_j[w] + b_j[w]) with the weight of the row's window (ops.stsgcn_wingemm on groups of 4N rows),
                    whose epilogue keeps the running max over the operations and the index of the winner.  Two launches per operation, all
                    windows and the whole batch in each.
    gated branch    tanh(conv2) sigmoid(conv1), each conv two taps at frames t and t + 3: ONE gated tap GEMM (ops.mtgnn_tapgemm, offsets (0, 3),
                    T -> T - 3 frames) over the weight [conv2; conv1] stacked tap-major — the kernel's gate is tanh(P) sigmoid(Q), so tanh takes
                    conv2.  The stacking is torch's, which carries the gradient of the stacked weight back onto conv1 and conv2 in their
                    (Cout, C, 1, 2) shape.  The sum of the two branches is a torch add.
    backward        windows (windows_hip.LayerFn, the layer function stsgcn_hip.py runs too), per operation, last to first: dPre
                    (ops.stsgcn_gate_bwd: the upstream gradient plus dOut where this operation won), dW and db per window (ops.stsgcn_winwgrad), dZ = dPre W (the grouped GEMM with the mirrored weights), then the
                    adjoint mix with S^T and D^T: middle -> expanded, expanded -> expanded, and for the first operation expanded -> frames.
                    Gate: dPre (ops.mtgnn_gate_bwd), dW and db (ops.mtgnn_wgrad), dX = the mirrored tap GEMM with offsets (0, -3).
    kept in torch   the position-embedding add (a broadcast add: autograd gives its gradients), the sum of the branches and the heads, stacked:
                    one addmm over the concatenated FC1 weights, one baddbmm for FC2 (STFGNN.head).  The first embedding is rows_hip.TapFn.

Kept for the backward, per operation: Z_j, sigma(Q) and P + b; per layer the winner index, and the gate's input, tanh and sigmoid.  Without a
backward to serve (no_grad, eval mode: keep = False) nothing is kept.
"""
import torch

from .. import _C, ops
from ..ops import ACT_RELU
from . import rows_hip, windows_hip
from .rows_hip import TapFn, mirror
from .windows_hip import MAX_NODES, LayerFn, Mix            # noqa: F401  (MAX_NODES: the bound of the mix's slab, under this module's name too)

SPAN = 4                   # frames of a window
GATE_OFFS = (0, 3)         # the two taps of conv1 / conv2: dilation 3 along T


def _mix(graphs, X, mode, B, T, N):
    return ops.stfgnn_mix(*graphs, X, mode, B, T, N)


class _GateFn(torch.autograd.Function):
    """g (B (T - 3) N, co) = tanh(P) sigmoid(Q), [P | Q] = H[t] Wg_0 + H[t + 3] Wg_1 + bg; Wg (2 co, 2 ci) tap-major"""

    @staticmethod
    def forward(ctx, H, Wg, bg, B, T, N, keep):
        keep = keep and any(ctx.needs_input_grad)
        if not keep:
            return ops.mtgnn_tapgemm(H, Wg, bg, GATE_OFFS, B, T, T - 3, N, gated=True)
        g, tn, s = ops.mtgnn_tapgemm(H, Wg, bg, GATE_OFFS, B, T, T - 3, N, gated=True, keep=True)
        ctx.cfg = (B, T, N)
        ctx.save_for_backward(H, Wg, tn, s)
        return g

    @staticmethod
    def backward(ctx, dg):
        H, Wg, tn, s = ctx.saved_tensors
        B, T, N = ctx.cfg
        dPre = ops.mtgnn_gate_bwd(dg.contiguous(), tn, s)
        dH = dW = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dW, db = ops.mtgnn_wgrad(dPre, H, GATE_OFFS, B, T, T - 3, N)
        if ctx.needs_input_grad[0]:
            dH = ops.mtgnn_tapgemm(dPre, mirror(Wg, 2), None, tuple(-o for o in GATE_OFFS), B, T - 3, T, N)
        return dH, dW, db, None, None, None, None


def gate_weight(lay):
    """(W (2 co, 2 ci) tap-major, b (2 co)) of the gated branch as one tap GEMM: conv2's rows (tanh), then conv1's (sigmoid)"""
    w = torch.cat([lay.conv2.weight, lay.conv1.weight])[:, :, 0, :].permute(0, 2, 1)
    return w.reshape(w.shape[0], -1).contiguous(), torch.cat([lay.conv2.bias, lay.conv1.bias])


def padded_graphs(model):
    """(S^, D, S^^T, D^T) zero-padded to 16-node tiles"""
    sp, spt = rows_hip.padded_graph(model, model.s_hat, "_sf_cache_s", True)
    dp, dpt = rows_hip.padded_graph(model, model.d_hat, "_sf_cache_d", True)
    return sp[0], dp[0], spt[0], dpt[0]


def supported(model, x):
    """the HIP path serves: CUDA fp32 4-D input of the module's window and node count, GLU, no mask, an adjacency that graph.stfgnn_blocks
    recognises as a fusion graph, at least two operations per layer of equal widths, channel widths that are multiples of 16 up to 128, and a
    node count whose slab fits the default LDS of a launch (N <= 448)"""
    if model.s_hat is None or model.d_hat is None:
        return False
    return windows_hip.supported(model, x, model.First_FC, model.window, model.hidden_dims)


def forward(model, x, keep=True):
    """predictors.stfgnn.STFGNN.forward on the kernels: x (B, T, N, dim_in) -> (B, horizon, N, output_dim).  keep = False (no_grad, eval mode):
    nothing is saved for a backward"""
    _C.lib()
    B, T, N, _ = x.shape
    sp, dp, spt, dpt = padded_graphs(model)
    mix = Mix(_mix, (sp, dp), (spt, dpt))
    fe = model.First_FC
    h = TapFn.apply(x.contiguous().view(B * T * N, -1), fe.weight.contiguous(), fe.bias.contiguous(), None, (0,), ACT_RELU, 0, T, N, keep)
    for lay in model.STSGCLS:
        H = lay.embed(h.view(B, T, N, -1)).reshape(B * T * N, -1)
        Wg, bg = gate_weight(lay)
        h = LayerFn.apply(H, mix, SPAN, B, T, N, keep, *windows_hip.stacked_weights(lay, len(lay.out_dims))) + _GateFn.apply(H, Wg, bg, B, T, N, keep)
        T -= SPAN - 1
    return model.head(h.view(B, T, N, -1))
