"""The STSGCN predictor on HIP (csrc/stsgcn.hip, csrc/stgcn.hip), forward and backward: what ``STSGCN(..., backend="hip")`` runs on CUDA fp32 input.

Channels-last as for the other predictors: the embedding arrives as (B, T, N, C), every activation is rows x C, nothing is permuted.  A layer over
T frames has W = T - 2 windows; inside it activations are window-expanded, rows (b, w, k, n) with block (w, k) standing for frame w + k, and the
last operation's output and the running max are rows (b, w, n) — already the next layer's (b, t, n).

    operation j     Z_j = mix(source) with the localized adjacency as blocks, mix(S)_k = A^ S_k + [k >= 1] S_{k-1} + [k <= 1] S_{k+1}
                    (ops.stsgcn_mix; the (3N, 3N) matrix is never formed: the first operation reads the frames directly, the last one forms the
                    middle block only), then GLU(Z_j W_j[w] + b_j[w]) with the weight of the row's window (ops.stsgcn_wingemm), whose epilogue
                    keeps the running max over the operations and the index of the winner.  Two launches per operation, all windows and the
                    whole batch in each.
    backward        (windows_hip.LayerFn, the layer function stfgnn_hip.py runs too) per operation, last to first: dPre
                    (ops.stsgcn_gate_bwd: the upstream gradient plus dOut where this operation won), dW and db
                    per window (ops.stsgcn_winwgrad), dZ = dPre W (the grouped GEMM with the mirrored weights), then the adjoint mix with A^T:
                    middle -> expanded, expanded -> expanded, and for the first operation expanded -> frames, a gather in a fixed order.
    kept in torch   the position-embedding add (a broadcast add: autograd gives its gradients) and the heads, stacked: one addmm over the
                    concatenated hidden weights, one baddbmm for the output layers (STSGCN.head).  The first embedding is rows_hip.TapFn.

Kept for the backward, per operation: Z_j (the GEMM's input, for the weight gradient — kept, not rebuilt: rebuilding it is another mix launch per
operation), sigma(Q) and P + b; per layer the winner index.  Without a backward to serve (no_grad, eval mode: keep = False) nothing is kept.
"""
from .. import _C, ops
from ..ops import ACT_RELU
from . import rows_hip, windows_hip
from .rows_hip import TapFn
from .windows_hip import MAX_NODES, LayerFn, Mix            # noqa: F401  (MAX_NODES: the bound of the mix's slab, under this module's name too)

SPAN = 3                   # frames of a window


def _mix(graphs, X, mode, B, T, N):
    return ops.stsgcn_mix(*graphs, X, mode, B, T, N)


def padded_graph(model):
    """(A^, A^T) zero-padded to 16-node tiles"""
    lp, lpt = rows_hip.padded_graph(model, model.a_hat, "_ss_cache", True)
    return lp[0], lpt[0]


def supported(model, x):
    """the HIP path serves: CUDA fp32 input of the module's input_window frames, GLU, at least two operations per layer of equal widths, channel
    widths that are multiples of 16 up to 128, no mask, and a node count whose slab fits the default LDS of a launch (N <= 448)"""
    fe = model.first_layer_embedding
    return fe is not None and windows_hip.supported(model, x, fe, model.input_window, [lay.layer.filters for lay in model.stsgcl_layers])


def forward(model, x, keep=True):
    """predictors.stsgcn.STSGCN.forward on the kernels: x (B, T, N, dim_in) -> (B, output_window, N, dim_out).  keep = False (no_grad, eval
    mode): nothing is saved for a backward"""
    _C.lib()
    B, T, N, _ = x.shape
    lp, lpt = padded_graph(model)
    mix = Mix(_mix, (lp,), (lpt,))
    fe = model.first_layer_embedding
    h = TapFn.apply(x.contiguous().view(B * T * N, -1), fe.weight.contiguous(), fe.bias.contiguous(), None, (0,), ACT_RELU, 0, T, N, keep)
    for lay in model.stsgcl_layers:
        lay = lay.layer
        H = lay.position_embedding(h.view(B, T, N, -1)).reshape(B * T * N, -1)
        h = LayerFn.apply(H, mix, SPAN, B, T, N, keep, *windows_hip.stacked_weights(lay, len(lay.filters)))
        T -= SPAN - 1
    return model.head(h.view(B, T, N, -1))
