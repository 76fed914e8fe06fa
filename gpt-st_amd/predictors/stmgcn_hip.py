"""The ST-MGCN predictor on HIP (csrc/stmgcn.hip + the hoisted tap GEMM and weight gradient of csrc/stgcn.hip), forward and backward: what
``STMGCN(..., backend="hip")`` runs on CUDA fp32 input.

The hot path is the stacked LSTM: L layers over the B N rows and T steps, once per graph.  A row (b, n) reads no other row, so the whole
recurrence of a branch is ONE launch forward (ops.stmgcn_lstm_fwd) and ONE backward (ops.stmgcn_lstm_bwd), states in LDS; rows are
TIME-major inside, (t, b, n).  Around it:

    hoisted forward     the context gate s (B, T) of each branch (torch: width T = 12 is not a kernel width);  P = X [W_ih0 of both branches]^T
                        over all B T N rows in one tap GEMM (rows_hip.TapFn, 2 * 4H columns);  Gx0 = s[b, t] P + (b_ih0 + b_hh0) — the scalar
                        gate commutes with the product, so ds, dX and dW_ih0 come out of autograd and the kernel sees neither x nor s
    hoisted backward    dW_hh0 = dG_0^T H_0[:T];  dW_ih_l = dG_l^T H_{l-1}[1:], dW_hh_l = dG_l^T H_l[:T] and the bias gradient of layers
                        l >= 1: ops.stgcn_wgrad over the T rows rows (row-split partials summed in a fixed order, no atomics) — dG and the h ring
                        are contiguous operands of it.  Its kernel takes any cw that is a multiple of 16, so cw = 4H = 512 at H = 128 is one
                        call like the others.  b_ih and b_hh only ever appear as their sum: the packing hands both the same gradient.
    torch               the output graph convolution and the head (1/36 of the LSTM's FLOPs), the packing of the weights

Kept for the backward: the activated gates, c and h of every (layer, step).  Where no LSTM parameter takes a gradient only layer 0's dG
leaves the launch and no weight gradient is formed; dx is bit-equal either way.  Without a backward to serve (no_grad, eval mode: the
module passes keep = False) the same forward launch writes the top layer's ring alone.
"""
import torch

from .. import _C, ops
from ..ops import ACT_NONE
from .rows_hip import LDS_MAX, TapFn, is_hip_input, widths_ok

MAX_L, MAX_T = 4, 32       # csrc/stmgcn.hip ST_MAXL, ST_MAXT
TILES = 0                  # tests: force 1 or 2 row tiles per workgroup (0: the kernel's rule)


def pack(lstm):
    """The LSTM's parameters in the kernels' form: (W flat = [W_hh0 (4H, H) | [W_ih_l | W_hh_l] (4H, 2H), l = 1 ..], bias (L, 4H) = b_ih_l +
    b_hh_l, W_ih0 (4H, C)).  Gate rows keep torch's order i, f, g, o: a wave reaches the four gates of its channel tile by stride H / 16
    over the column tiles, at any H.  Plain differentiable tensor ops: autograd carries the gradients back to the parameters."""
    g = lambda n, l: getattr(lstm, "%s_l%d" % (n, l))                      # noqa: E731
    L = lstm.num_layers
    W = [g("weight_hh", 0).reshape(-1)] + [torch.cat([g("weight_ih", l), g("weight_hh", l)], dim=1).reshape(-1) for l in range(1, L)]
    bias = torch.stack([g("bias_ih", l) + g("bias_hh", l) for l in range(L)])
    return torch.cat(W), bias, g("weight_ih", 0)


def unpack(W, H, L):
    """-> [(W_ih_l | None, W_hh_l)] of a flat W (or of a gradient in its layout)"""
    out, off = [(None, W[:4 * H * H].view(4 * H, H))], 4 * H * H
    for _ in range(1, L):
        w = W[off:off + 8 * H * H].view(4 * H, 2 * H)
        out.append((w[:, :H], w[:, H:]))
        off += 8 * H * H
    return out


def transposed(W, H, L):
    """the flat W with every block transposed: the weights of the backward's GEMM"""
    return torch.cat([(hh if ih is None else torch.cat([ih, hh], dim=1)).t().reshape(-1) for ih, hh in unpack(W, H, L)])


class _LstmFn(torch.autograd.Function):
    """Gx0 (T, rows, 4H), W flat, bias (L, 4H) -> the top layer's ring (T, rows, H)"""

    @staticmethod
    def forward(ctx, Gx0, W, bias, L, keep, tiles):
        keep = keep and any(ctx.needs_input_grad)
        W, bias = W.contiguous(), bias.contiguous()
        top, gates, c, h = ops.stmgcn_lstm_fwd(Gx0.contiguous(), W, bias, L, keep, tiles)
        if keep:
            ctx.cfg = (L, tiles)
            ctx.save_for_backward(W, gates, c, h)
        return top

    @staticmethod
    def backward(ctx, dTop):
        W, gates, c, h = ctx.saved_tensors
        L, tiles = ctx.cfg
        _, T, rows, H4 = gates.shape
        H = H4 // 4
        wgrad = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dG = ops.stmgcn_lstm_bwd(dTop.contiguous(), transposed(W, H, L), gates, c, L if wgrad else 1, tiles)
        dW = db = None
        if wgrad:
            parts, db = [], [dG.new_zeros(H4)]                             # (row 0 of the bias is inside Gx0: its gradient flows there)
            for l in range(L):
                d = dG[l].view(T * rows, H4)
                whh, bl = ops.stgcn_wgrad(d, h[l, :T].reshape(T * rows, H), (0,), T, rows, want_bias=l > 0)
                if l == 0:
                    parts.append(whh.reshape(-1))
                    continue
                wih, _ = ops.stgcn_wgrad(d, h[l - 1, 1:].reshape(T * rows, H), (0,), T, rows, want_bias=False)
                parts.append(torch.cat([wih, whh], dim=1).reshape(-1))
                db.append(bl)
            dW, db = torch.cat(parts), torch.stack(db)
        return (dG[0] if ctx.needs_input_grad[0] else None), dW, db, None, None, None


def supported(model, x):
    """the HIP path serves: CUDA fp32 4-D input of the module's own (T, N, C), lstm_hidden_dim a multiple of 16 up to 128, dim_in a
    multiple of 16 up to 128, at most 4 layers and 32 steps, and an LDS plan within the 160 KB"""
    if not is_hip_input(x):
        return False
    B, T, N, C = x.shape
    H, L = model.lstm_hidden_dim, model.lstm_num_layers
    if (T, N, C) != (model.seq_len, model.n_nodes, model.input_dim) or B < 1:
        return False
    if not widths_ok([C, H]) or not 1 <= L <= MAX_L or not 1 <= T <= MAX_T:
        return False
    tiles = ops.stmgcn_tiles(B * N, H, L, TILES)
    return tiles > 0 and 0 < ops.stmgcn_lds_bytes(H, L, tiles) <= LDS_MAX


def forward(model, x, keep=True):
    """predictors.stmgcn.STMGCN.forward on the kernels: x (B, T, N, dim_in) -> (B, T, N, dim_out).  keep = False (no_grad, eval mode): the
    launches write nothing for a backward and nothing is saved"""
    _C.lib()
    B, T, N, C = x.shape
    H, L, M = model.lstm_hidden_dim, model.lstm_num_layers, model.M
    packed = [pack(r.lstm) for r in model.rnn_list]
    Wih = torch.cat([p[2] for p in packed]).contiguous()                   # (M 4H, C): one GEMM for both branches
    zero = x.new_zeros(M * 4 * H)                                          # (both biases of layer 0 join after the gate, below)
    P = TapFn.apply(x.contiguous().view(B * T * N, C), Wih, zero, None, (0,), ACT_NONE, 0, T, N, keep).view(B, T, N, M, 4 * H)
    feats = []
    for m, A in enumerate(model.graphs()):
        W, bias, _ = packed[m]
        s = model.rnn_list[m].gate(A, x)
        Gx0 = (P[:, :, :, m] * s.view(B, T, 1, 1) + bias[0]).transpose(0, 1).reshape(T, B * N, 4 * H)       # time-major from here on
        top = _LstmFn.apply(Gx0, W, bias, L, keep, TILES)
        feats.append(top[T - 1].view(B, N, H))
    return model.head(feats)
