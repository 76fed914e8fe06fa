"""The TGCN predictor on HIP (csrc/tgcn.hip + the hoisted kernels of csrc/stgcn.hip), forward and backward: what ``TGCN(..., backend="hip")``
runs on CUDA fp32 input.

Channels-last rows (b, t, n) as in stgcn_hip.py; no permute is materialised.  ``rnn_units`` H is zero-padded to Hp = 16 ceil(H / 16) inside the
PACKED weights only (``pack``): a padded channel stays exactly 0 through the recurrence (sigmoid(0) = 1/2, tanh(0) = 0, h' = 0/2 + 0/2), and the
packing, being plain differentiable tensor ops, drops its weight gradients on the way back to the parameters, which keep the reference's shapes.

Hoisted out of the loop (L [x_t, h] = [L x_t, L h]):
    forward    LX = L X over all B T units (stgcn_nodemix);  Gx0 = LX W0[:C] + b0 (rows, 2 Hp),  Gx1 = LX W1[:C] + b1 (rows, Hp) (stgcn_tapgemm)
    backward   dW0 = [LX | m1]^T dPre0,  dW1 = [LX | m2]^T dPre1 with the biases, one stgcn_wgrad each over all rows;
               dX = L^T (dPre0 W0[:C]^T + dPre1 W1[:C]^T): two stgcn_tapgemm (the second adds the first) and one stgcn_nodemix
Sequential, two launches per step in each direction (ops.tgcn_fwd_gates / tgcn_fwd_state, tgcn_bwd_cand / tgcn_bwd_state).

Kept for the backward: h of every step, u, r, c, and m1 = L h, m2 = L (r h) in the right-hand columns of the [LX | .] buffers (only when a weight
takes a gradient).  Without a backward to serve (no_grad, eval mode: the module passes keep = False) the same launches run and nothing is written for one.
"""
import torch
import torch.nn.functional as F

from .. import _C, ops
from ..ops import ACT_NONE
from .rows_hip import LDS_MAX, is_hip_input, nodemix_fits, pad16 as padded, padded_graph, widths_ok

def pack(W0, b0, W1, b1, C, H):
    """The parameters (reference layout: W (C + H, gates * H), gate-major columns) in the kernels' GEMM form, outputs as rows:
    P0 (2 Hp, C + Hp) = [r rows | u rows], pb0 (2 Hp), P1 (Hp, C + Hp), pb1 (Hp); columns [0, C) act on L x_t, [C, C + Hp) on L h.  Padding is zero."""
    Hp = padded(H)

    def one(W, b, gates):
        P = F.pad(W.t().reshape(gates, H, C + H), (0, Hp - H, 0, Hp - H))           # (gates, Hp, C + Hp)
        return P.reshape(gates * Hp, C + Hp), F.pad(b.view(gates, H), (0, Hp - H)).reshape(gates * Hp)
    return one(W0, b0, 2) + one(W1, b1, 1)


class _RecurrenceFn(torch.autograd.Function):
    """x (B T N, C) -> h_T (B N, Hp)"""

    @staticmethod
    def forward(ctx, x, P0, pb0, P1, pb1, Lp, LpT, dims, keep):
        B, T, N = dims
        C, Hp, S, rows = x.shape[1], P1.shape[0], B * N, B * T * N
        keep = keep and any(ctx.needs_input_grad)
        keep_m = keep and any(ctx.needs_input_grad[1:5])                 # m1, m2 serve the weight gradients only
        LX = ops.stgcn_nodemix(Lp, x, N, C, reduce=False)
        Gx0 = ops.stgcn_tapgemm(LX, P0[:, :C].contiguous(), pb0.contiguous(), (0,), ACT_NONE, T, N)
        Gx1 = ops.stgcn_tapgemm(LX, P1[:, :C].contiguous(), pb1.contiguous(), (0,), ACT_NONE, T, N)
        W0h, W1h, L2 = P0[:, C:].contiguous(), P1[:, C:].contiguous(), Lp[0]
        Z0 = Z1 = U = R = Cc = None
        if keep_m:
            Z0, Z1 = x.new_empty(rows, C + Hp), x.new_empty(rows, C + Hp)
            Z0[:, :C] = LX
            Z1[:, :C] = LX
        if keep:
            Hs = x.new_empty(T + 1, S, Hp)
            U, R, Cc = x.new_empty(T, S, Hp), x.new_empty(T, S, Hp), x.new_empty(T, S, Hp)
        else:
            Hs, ubuf = x.new_empty(2, S, Hp), x.new_empty(S, Hp)
        Hs[0].zero_()
        q = x.new_empty(S, Hp)
        for t in range(T):
            h, hn = (Hs[t], Hs[t + 1]) if keep else (Hs[t % 2], Hs[(t + 1) % 2])
            u = U[t] if keep else ubuf
            ops.tgcn_fwd_gates(L2, W0h, h, Gx0, t, u, q, B, T, N, r=R[t] if keep else None, z=Z0, zoff=C)
            ops.tgcn_fwd_state(L2, W1h, q, Gx1, t, u, h, hn, B, T, N, c=Cc[t] if keep else None, z=Z1, zoff=C)
        if keep:
            ctx.dims = dims
            ctx.save_for_backward(P0, P1, LpT, Hs, U, R, Cc, Z0, Z1)
        return hn.clone() if keep else hn

    @staticmethod
    def backward(ctx, dhT):
        P0, P1, LpT, Hs, U, R, Cc, Z0, Z1 = ctx.saved_tensors
        B, T, N = ctx.dims
        Hp, rows = P1.shape[0], B * T * N
        C = P1.shape[1] - Hp
        dh, part = dhT.contiguous().clone(), torch.empty_like(dhT)
        dPre0, dPre1 = dh.new_empty(rows, 2 * Hp), dh.new_empty(rows, Hp)
        W1hT, W0hT, LT2 = P1[:, C:].t().contiguous(), P0[:, C:].t().contiguous(), LpT[0]
        for t in reversed(range(T)):
            ops.tgcn_bwd_cand(LT2, W1hT, dh, U[t], Cc[t], R[t], Hs[t], t, dPre1, dPre0, part, B, T, N)
            if t > 0:                                                      # (h_0 = 0 takes no gradient)
                ops.tgcn_bwd_state(LT2, W0hT, dPre0, part, t, dh, B, T, N)
        dx = dP0 = db0 = dP1 = db1 = None
        if any(ctx.needs_input_grad[1:5]):
            dP0, db0 = ops.stgcn_wgrad(dPre0, Z0, (0,), T, N)
            dP1, db1 = ops.stgcn_wgrad(dPre1, Z1, (0,), T, N)
        if ctx.needs_input_grad[0]:
            G = ops.stgcn_tapgemm(dPre1, P1[:, :C].t().contiguous(), None, (0,), ACT_NONE, T, N)
            G = ops.stgcn_tapgemm(dPre0, P0[:, :C].t().contiguous(), None, (0,), ACT_NONE, T, N, res=G, res_w=C)
            dx = ops.stgcn_nodemix(LpT, G, N, C, reduce=True)
        return dx, dP0, db0, dP1, db1, None, None, None, None


def supported(model, x):
    """the HIP path serves: CUDA fp32 4-D input of the module's own (T, N, C), dim_in a multiple of 16 up to 128, rnn_units <= 128 (any value: it is
    padded), and any N whose operand slabs fit the 160 KB of LDS"""
    if not is_hip_input(x):
        return False
    B, T, N, C = x.shape
    H = model.gru_units
    if (T, N, C) != (model.input_window, model.num_nodes, model.input_dim) or model.tgcn_model.L.shape[0] != N:
        return False
    if not widths_ok([C]) or not 1 <= H <= 128 or not 1 <= B <= 65535:
        return False
    return nodemix_fits(N) and 0 < _C.lib().value("gptst_tgcn_lds_bytes", N, padded(H), B) <= LDS_MAX


def forward(model, x, keep=True):
    """predictors.tgcn.TGCN.forward on the kernels: x (B, T, N, dim_in) -> (B, W, N, output_dim).  keep = False (no_grad, eval mode): no launch
    writes anything for a backward and nothing is saved"""
    _C.lib()
    B, T, N, C = x.shape
    cell, H = model.tgcn_model, model.gru_units
    lp, lpt = padded_graph(cell, cell.L, "_lp_cache", True)
    hT = _RecurrenceFn.apply(x.contiguous().view(B * T * N, C), *pack(cell.weights_0, cell.bias_0, cell.weights_1, cell.bias_1, C, H), lp, lpt,
                             (B, T, N), keep)
    return model.head(hT.view(B, N, -1)[:, :, :H])
