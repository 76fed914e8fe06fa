"""The STSGCN predictor on HIP (csrc/stsgcn.hip, csrc/stgcn.hip), forward and backward: what ``STSGCN(..., backend="hip")`` runs on CUDA fp32 input.

Channels-last as for the other predictors: the embedding arrives as (B, T, N, C), every activation is rows x C, nothing is permuted.  A layer over
T frames has W = T - 2 windows; inside it activations are window-expanded, rows (b, w, k, n) with block (w, k) standing for frame w + k, and the
last operation's output and the running max are rows (b, w, n) — already the next layer's (b, t, n).

    operation j     Z_j = mix(source) with the localized adjacency as blocks, mix(S)_k = A^ S_k + [k >= 1] S_{k-1} + [k <= 1] S_{k+1}
                    (ops.stsgcn_mix; the (3N, 3N) matrix is never formed: the first operation reads the frames directly, the last one forms the
                    middle block only), then GLU(Z_j W_j[w] + b_j[w]) with the weight of the row's window (ops.stsgcn_wingemm), whose epilogue
                    keeps the running max over the operations and the index of the winner.  Two launches per operation, all windows and the
                    whole batch in each.
    backward        per operation, last to first: dPre (ops.stsgcn_gate_bwd: the upstream gradient plus dOut where this operation won), dW and db
                    per window (ops.stsgcn_winwgrad), dZ = dPre W (the grouped GEMM with the mirrored weights), then the adjoint mix with A^T:
                    middle -> expanded, expanded -> expanded, and for the first operation expanded -> frames, a gather in a fixed order.
    kept in torch   the position-embedding add (a broadcast add: autograd gives its gradients) and the heads, stacked: one addmm over the
                    concatenated hidden weights, one baddbmm for the output layers (STSGCN.head).  The first embedding is rows_hip.TapFn.

Kept for the backward, per operation: Z_j (the GEMM's input, for the weight gradient — kept, not rebuilt: rebuilding it is another mix launch per
operation), sigma(Q) and P + b; per layer the winner index.  Without a backward to serve (no_grad, eval mode: keep = False) nothing is kept.
"""
import torch

from .. import _C, ops
from ..ops import ACT_GLU, ACT_NONE, ACT_RELU
from . import rows_hip
from .rows_hip import TapFn, is_hip_input, widths_ok

MAX_NODES = 448            # the mix keeps a (Np, 36) slab of a block in the 64 KB of LDS a launch gets by default


class _LayerFn(torch.autograd.Function):
    """best (B W N, co) = max over the J operations of a layer; H (B T N, ci) with the embeddings added; wb = W_0, b_0, W_1, b_1, ...: the stacked
    weights (W | 1, 2 co, ci) and biases"""

    @staticmethod
    def forward(ctx, H, lp, lpt, B, T, N, keep, *wb):
        keep = keep and any(ctx.needs_input_grad)
        W, J = T - 2, len(wb) // 2
        co = wb[0].shape[1] // 2
        best = torch.empty(B * W * N, co, device=H.device, dtype=torch.float32)
        which = torch.empty(B * W * N, co, device=H.device, dtype=torch.int32) if keep else None
        cur, saved = H, []
        for j in range(J):
            last = j == J - 1
            Z = ops.stsgcn_mix(lp, cur, ops.MIX_F2E if j == 0 else ops.MIX_E2M if last else ops.MIX_E2E, B, T, N)          # (J >= 2: supported())
            R = N if last else 3 * N
            out = ops.stsgcn_wingemm(Z, wb[2 * j], wb[2 * j + 1], ACT_GLU, B, W, R, N, keep=keep, best=best, which=which, opj=j)
            if keep:
                cur, S, A = out
                saved += [Z, S, A]
            else:
                cur = out
        if keep:
            ctx.cfg = (B, T, N, J)
            ctx.save_for_backward(lpt, which, *wb[0::2], *saved)
        return best

    @staticmethod
    def backward(ctx, dBest):
        B, T, N, J = ctx.cfg
        lpt, which = ctx.saved_tensors[:2]
        Ws, saved = ctx.saved_tensors[2:2 + J], ctx.saved_tensors[2 + J:]
        W = T - 2
        dBest = dBest.contiguous()
        grads, up = [None] * (2 * J), None
        for j in range(J - 1, -1, -1):
            Z, S, A = saved[3 * j:3 * j + 3]
            R = N if j == J - 1 else 3 * N
            dPre = ops.stsgcn_gate_bwd(up, dBest, which, j, S, A, B, W, R, N)
            if ctx.needs_input_grad[7 + 2 * j] or ctx.needs_input_grad[8 + 2 * j]:
                dW, db = ops.stsgcn_winwgrad(dPre, Z, B, W, R)
                if Ws[j].shape[0] == 1 and W > 1:                       # one weight for all windows: the windows' gradients add up, in order
                    dW, db = dW.sum(0, keepdim=True), db.sum(0, keepdim=True)
                grads[2 * j], grads[2 * j + 1] = dW, db
            if j == 0 and not ctx.needs_input_grad[0]:
                up = None
                break
            dZ = ops.stsgcn_wingemm(dPre, Ws[j].transpose(1, 2).contiguous(), None, ACT_NONE, B, W, R, N)
            up = ops.stsgcn_mix(lpt, dZ, ops.MIX_E2F if j == 0 else ops.MIX_M2E if j == J - 1 else ops.MIX_E2E, B, T, N)
        return (up, None, None, None, None, None, None) + tuple(grads)


def padded_graph(model):
    """(A^, A^T) zero-padded to 16-node tiles"""
    lp, lpt = rows_hip.padded_graph(model, model.a_hat, "_ss_cache", True)
    return lp[0], lpt[0]


def supported(model, x):
    """the HIP path serves: CUDA fp32 input of the module's input_window frames, GLU, at least two operations per layer of equal widths, channel
    widths that are multiples of 16 up to 128, no mask, and a node count whose slab fits the default LDS of a launch (N <= 448)"""
    if not is_hip_input(x) or model.activation != "GLU" or model.use_mask or model.first_layer_embedding is None:
        return False
    fe = model.first_layer_embedding
    if x.shape[1] != model.input_window or x.shape[2] != model.num_nodes or x.shape[3] != fe.in_features or model.num_nodes > MAX_NODES:
        return False
    widths = [fe.in_features, fe.out_features]
    for lay in model.stsgcl_layers:
        f = lay.layer.filters
        if len(f) < 2 or len(set(f)) != 1:
            return False
        widths += f
    return widths_ok(widths)


def forward(model, x, keep=True):
    """predictors.stsgcn.STSGCN.forward on the kernels: x (B, T, N, dim_in) -> (B, output_window, N, dim_out).  keep = False (no_grad, eval
    mode): nothing is saved for a backward"""
    _C.lib()
    B, T, N, _ = x.shape
    lp, lpt = padded_graph(model)
    fe = model.first_layer_embedding
    h = TapFn.apply(x.contiguous().view(B * T * N, -1), fe.weight.contiguous(), fe.bias.contiguous(), None, (0,), ACT_RELU, 0, T, N, keep)
    for lay in model.stsgcl_layers:
        lay = lay.layer
        H = lay.position_embedding(h.view(B, T, N, -1)).reshape(B * T * N, -1)
        wb = []
        for j in range(len(lay.filters)):
            wb += lay.stacked(j)
        h = _LayerFn.apply(H, lp, lpt, B, T, N, keep, *wb)
        T -= 2
    return model.head(h.view(B, T, N, -1))
