"""The DMVSTNET predictor on HIP (csrc/dmvstnet.hip, the one-launch LSTM of csrc/stmgcn.hip, the node mix, tap GEMM and weight gradient of
csrc/stgcn.hip), forward and backward: what ``DMVSTNET(..., backend="hip")`` runs on CUDA fp32 input.

TIME-major inside: one permuted copy of x to (T, B, N, C) at the entry puts every later tensor in the LSTM's (t, b, n) row order — the node
mix and the row GEMMs do not care in which order the (b, t) units come — so the 4H-wide Gx0 is never transposed.  h = hidden_dim, H = 2 h.

    P    = x [W_spa | W_tem]^T + b                   one tap GEMM (rows_hip.TapFn), 2 h columns
    S    = Lin_spa(relu(lin(A spa))) + spa           ops.stgcn_nodemix with the zero-padded raw A, two row layers, the residual in the second's
                                                     epilogue
    Gx0  = [S | tem] W_ih^T + (b_ih + b_hh)          one tap GEMM on the concatenation (torch.cat: one copy of rows x H)
    ring = the LSTM's h of every step                ST-MGCN's launches at one layer (stmgcn_hip._LstmFn: ONE launch forward, ONE backward, the
                                                     weight gradient through ops.stgcn_wgrad), one row tile per workgroup above H = 64
    y    = ring Wa^T, (T, rows, O)                   the head's columns over h applied to the ring, BEFORE the last step is added: a torch matmul
    top  = y_t + y_{T-1}                             on (T, rows, O): `out_lstm + hid` is never materialised at width H, nor its concatenation
    z    = x V[n] + c[n]                             ops.dmvst_sen_fwd: Lin_in_sen, the per-node generated weight and the head's columns over the
                                                     semantic view composed by torch (``sen_pack``) into V (N, C, O), c (N, O)
    out  = top + z + b_out, permuted back to (B, T, N, O)

Both reassociations are exact algebra — there is no nonlinearity between h_t or the semantic view and the output — and change the
summation order only.  b_ih and b_hh only ever appear as their sum and take the same gradient.  Kept for the backward: the activated gates,
c and the h ring.  No float atomics; a step repeats bit for bit.  (The head applied inside the LSTM launches was built and measured: slower
forward + backward than this route at both conf shapes, so it is not here — DESIGN.md section 33.)
"""
import torch

from .. import _C, ops
from ..ops import ACT_NONE, ACT_RELU
from .rows_hip import LDS_MAX, TapFn, is_hip_input, nodemix_fits, padded_graph, widths_ok
from .stmgcn_hip import MAX_T, _LstmFn

TILES = 0                  # tests: force 1 or 2 row tiles per workgroup (0: row_tiles' choice)


def row_tiles(H):
    """16-row tiles per workgroup of the two LSTM launches.  Above H = 64 a wave owns two channel tiles and the two-tile forward kernel fills
    the 256 VGPRs, one wave a SIMD: one tile per workgroup measured 12 - 18 % faster forward + backward and 21 - 27 % forward only at the
    two conf shapes (H = 128).  Up to 64 the kernel's own rule stands (0)."""
    return TILES or (1 if H > 64 else 0)


class _MixFn(torch.autograd.Function):
    """x (units N, c) -> A x per unit; the graph takes no gradient (a buffer)"""

    @staticmethod
    def forward(ctx, x, Lp, LpT, N):
        ctx.N = N
        ctx.save_for_backward(LpT)
        return ops.stgcn_nodemix(Lp, x, N, x.shape[1], reduce=False)

    @staticmethod
    def backward(ctx, dy):
        LpT, = ctx.saved_tensors
        return ops.stgcn_nodemix(LpT, dy.contiguous(), ctx.N, dy.shape[1], reduce=False), None, None, None


class _SenFn(torch.autograd.Function):
    """x (rows, C), V (N, C, O), c (N, O) -> z (rows, O)"""

    @staticmethod
    def forward(ctx, x, V, c, N, keep):
        V, c = V.contiguous(), c.contiguous()
        if keep and any(ctx.needs_input_grad):
            ctx.N = N
            ctx.save_for_backward(x, V)
        return ops.dmvst_sen_fwd(x, V, c, N)

    @staticmethod
    def backward(ctx, dz):
        x, V = ctx.saved_tensors
        dx, dV, dc = ops.dmvst_sen_bwd(x, V, dz.contiguous(), ctx.N)
        return (dx if ctx.needs_input_grad[0] else None), dV, dc, None, None


def sen_pack(model):
    """-> (V (N, C, O), c (N, O)): V[n] = W_sen^T (sum_d E[n, d] w[d]) Wb^T and c[n] = b_sen (sum_d E[n, d] w[d]) Wb^T, Wb (O, h) the head's
    columns over the semantic view.  The head is applied to w first, so no (N, h, h) tensor is formed.  Plain differentiable tensor ops:
    autograd carries the gradients back to the five parameters."""
    Wb = model.output.weight[:, model.lstm_dim:]
    M = torch.einsum("nd,dip->nip", model.node_embeddings, torch.einsum("dio,po->dip", model.w, Wb))          # (N, h, O)
    return torch.einsum("ic,nip->ncp", model.Lin_in_sen.weight, M), torch.einsum("i,nip->np", model.Lin_in_sen.bias, M)


def supported(model, x):
    """the HIP path serves: CUDA fp32 4-D input of the module's own (T, N, dim_in); dim_in, hidden_dim and H multiples of 16 up to 128; a node
    count whose mix slab fits; at most 32 steps; dim_out 2; and an LDS plan within the 160 KB"""
    if not is_hip_input(x):
        return False
    B, T, N, C = x.shape
    H = model.lstm_dim
    if (T, N, C) != (model.input_window, model.num_nodes, model.dim_in) or B < 1 or model.dim_out != 2:
        return False
    if not widths_ok([C, model.hidden_dim, H]) or not nodemix_fits(N) or not 1 <= T <= MAX_T:
        return False
    tiles = ops.stmgcn_tiles(B * N, H, 1, row_tiles(H))
    return tiles > 0 and 0 < ops.stmgcn_lds_bytes(H, 1, tiles) <= LDS_MAX


def forward(model, x, keep=True):
    """predictors.dmvstnet.DMVSTNET.forward on the kernels: x (B, T, N, dim_in) -> (B, T, N, dim_out).  keep = False (no_grad, eval mode): the
    launches write nothing for a backward and nothing is saved"""
    _C.lib()
    B, T, N, C = x.shape
    h, H, O = model.hidden_dim, model.lstm_dim, model.dim_out
    rows = T * B * N
    X = x.permute(1, 0, 2, 3).contiguous().view(rows, C)                   # time-major from here on
    lp, lpt = padded_graph(model, model.adj_mx, "_dm_cache", True)
    tap = lambda a, W, b, act=ACT_NONE, res=None, res_w=0: TapFn.apply(a, W, b, res, (0,), act, res_w, T, N, keep)      # noqa: E731
    P = tap(X, torch.cat([model.Lin_in_spa.weight, model.Lin_in_tem.weight]).contiguous(),
            torch.cat([model.Lin_in_spa.bias, model.Lin_in_tem.bias]).contiguous())
    spa = P[:, :h].contiguous()
    G = tap(_MixFn.apply(spa, lp, lpt, N), model.Local_GNN1.lin.weight, model.Local_GNN1.lin.bias, ACT_RELU)
    S = tap(G, model.Lin_spa.weight, model.Lin_spa.bias, ACT_NONE, spa, h)
    lstm = model.lstm
    Gx0 = tap(torch.cat([S, P[:, h:]], dim=1), lstm.weight_ih_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0).view(T, B * N, 4 * H)
    ring = _LstmFn.apply(Gx0, lstm.weight_hh_l0.reshape(-1), Gx0.new_zeros(1, 4 * H), 1, keep, row_tiles(H))      # (row 0 of the bias is inside Gx0)
    y = ring @ model.output.weight[:, :H].t()
    V, c = sen_pack(model)
    z = _SenFn.apply(X, V, c, N, keep)
    out = y + y[T - 1:] + z.view(T, B * N, O) + model.output.bias
    return out.view(T, B, N, O).permute(1, 0, 2, 3).contiguous()
