"""The CCRNN predictor on HIP (csrc/ccrnn.hip + the hoisted kernels of csrc/stgcn.hip and csrc/mtgnn.hip), forward and backward: what
``CCRNN(..., backend="hip")`` runs on CUDA fp32 input at one graph-conv layer, one support, k_hop 1..3, one or two RNN layers, hidden_size <= 32.

The polynomial stack, once per forward: P = [T_1(S) .. T_k(S)] of S = graph0 as (k, Np, Np) matrices, plain differentiable torch on N x N, zero
padded.  T_j(S) z = P_j z, so the k products of a cell step are independent and one mix launch, not a chain of k; the kernels return dP and
autograd carries it to ``nodevec1, nodevec2``.

``hidden_size`` H is zero-padded to Hp inside the PACKED weights only (``pack_cell``): a padded channel stays exactly 0 through the recurrence, and
the packing — plain differentiable tensor ops that also reorder the reference's ``c * num_matrices + m`` columns to matrix-major — drops its
weight gradients on the way back to the parameters, which keep the reference's shapes.

Encoder, a layer at a time (``_EncLayerFn``): the input half is hoisted over all B T units — stgcn_nodemix with [I | P], stgcn_tapgemm — and
layer 1 takes layer 0's states of all steps as its hoisted input.  Two launches per step in each direction (ops.ccrnn_*).
Decoder (``_DecoderFn``): nothing can be hoisted; the operand slab of a step is [h | input].  The feedback out(h) is formed while the slab of
the next step's first launch is filled (no launch of its own); the teacher-forcing decisions of all steps are drawn by the module before the
first launch.  A forced step reads targets[:, t] and sends no gradient into y_t.  The output Linear over all steps is one torch op outside.
Backward: dpre of every step is kept; after the loop every weight gradient is one stgcn_wgrad over all rows, and
dP_j = sum over units of (dpre W_j) z^T is ops.mtgnn_graphgrad of one tap GEMM.  No float atomics: a step repeats bit for bit.

Gradient presence matches the torch backend: the ``attlinear`` parameters, which nothing reads at one graph-conv layer, get zero tensors
(``_ZeroGradFn``); ``w1, w2, b1, b2`` get None.  Without a backward to serve (no_grad, eval mode) the same launches run and nothing is kept.
"""
import torch
import torch.nn.functional as F

from .. import _C, ops
from ..ops import ACT_NONE
from .rows_hip import LDS_MAX, is_hip_input, mirror, nodemix_fits, pad16, widths_ok

TILES = 0                        # row tiles per workgroup handed to every step launch (0: the library's rule; tests force 1 and 2)


def poly_stack(S, k):
    """S (N, N) -> [T_1(S) .. T_k(S)] (k, N, N) by the Chebyshev recursion on matrices: T_j = 2 S T_{j-1} - T_{j-2}"""
    Ts = [torch.eye(S.shape[0], device=S.device, dtype=S.dtype), S]
    for _ in range(2, k + 1):
        Ts.append(2 * S.mm(Ts[-1]) - Ts[-2])
    return torch.stack(Ts[1:k + 1], 0)


def pack_cell(W, b, Cin, H, gates, M):
    """A GraphConv Linear (reference layout: W (gates H, (Cin + H) M), column c M + m over the channels [input (Cin) | state (H)]) in the
    kernels' GEMM form, matrix-major: -> Wh (gates Hp, M, Hp) on the state, Wi (gates Hp, M, Cin) on the input, pb (gates Hp).  Padding is zero."""
    Hp = pad16(H)
    W4 = F.pad(W.view(gates, H, Cin + H, M).permute(0, 1, 3, 2), (0, 0, 0, 0, 0, Hp - H))     # (gates, Hp, M, Cin + H)
    Wi, Wh = W4[..., :Cin], F.pad(W4[..., Cin:], (0, Hp - H))
    return Wh.reshape(gates * Hp, M, Hp), Wi.reshape(gates * Hp, M, Cin), F.pad(b.view(gates, H), (0, Hp - H)).reshape(gates * Hp)


def slab_weight(Wh, Wi, Cp):
    """-> (NO, M (Hp + Cp)): the weight over [state | input] slabs, the input's columns zero-padded to Cp"""
    return torch.cat([Wh, F.pad(Wi, (0, Cp - Wi.shape[2]))], dim=2).reshape(Wh.shape[0], -1)


def _graph_grad(dPre, W, Z, Ks, k, T, N):
    """dP (k, N, N) of one GEMM of a cell over all rows: D = dPre W (rows, (k + 1) Ks), block j against the unmixed operand z = the first Ks
    columns of Z, read in place at Z's row pitch"""
    D = ops.stgcn_tapgemm(dPre, W.t().contiguous(), None, (0,), ACT_NONE, T, N)
    return ops.mtgnn_graphgrad(D, Z, N, Ks, k, dcol0=Ks)


def _padded(dP, Np):
    return F.pad(dP, (0, Np - dP.shape[2], 0, Np - dP.shape[1]))


class _EncLayerFn(torch.autograd.Function):
    """one encoder layer over all steps: x (B T N, C) seq -> the states of every step (T, B N, Hp)"""

    @staticmethod
    def forward(ctx, x, W0h, W0x, b0, W1h, W1x, b1, Pst, dims, keep):
        B, T, N = dims
        C, Hp, k, S, rows = x.shape[1], W1h.shape[0], Pst.shape[0], B * N, B * T * N
        keep = keep and any(ctx.needs_input_grad)
        eye = torch.zeros_like(Pst[:1])
        eye[0, :N, :N] = torch.eye(N, device=x.device)
        Pfull = torch.cat([eye, Pst], 0)
        LX = ops.stgcn_nodemix(Pfull, x, N, C, reduce=False)                 # [x | P_j x]_j over all B T units
        Gx0 = ops.stgcn_tapgemm(LX, W0x.contiguous(), b0.contiguous(), (0,), ACT_NONE, T, N)
        Gx1 = ops.stgcn_tapgemm(LX, W1x.contiguous(), b1.contiguous(), (0,), ACT_NONE, T, N)
        W0h, W1h = W0h.contiguous(), W1h.contiguous()
        Hs = x.new_empty(T + 1, S, Hp)
        Hs[0].zero_()
        Z0 = Z1 = U = R = Cc = None
        if keep:
            U, R, Cc = x.new_empty(T, S, Hp), x.new_empty(T, S, Hp), x.new_empty(T, S, Hp)
            Z0, Z1 = x.new_empty(rows, (k + 1) * Hp), x.new_empty(rows, (k + 1) * Hp)
        else:
            ubuf = x.new_empty(S, Hp)
        q = x.new_empty(S, Hp)
        for t in range(T):
            u = U[t] if keep else ubuf
            ops.ccrnn_fwd_gates(Pst, W0h, Hs[t], Gx0, t, u, q, B, T, N, r=R[t] if keep else None, z=Z0, tiles=TILES)
            ops.ccrnn_fwd_state(Pst, W1h, q, Gx1, t, u, Hs[t], Hs[t + 1], B, T, N, c=Cc[t] if keep else None, z=Z1, tiles=TILES)
        if keep:
            ctx.dims = dims
            ctx.save_for_backward(x, W0h, W0x, W1h, W1x, Pst, Pfull, LX, Hs, U, R, Cc, Z0, Z1)
        return Hs[1:]

    @staticmethod
    def backward(ctx, dHall):
        x, W0h, W0x, W1h, W1x, Pst, Pfull, LX, Hs, U, R, Cc, Z0, Z1 = ctx.saved_tensors
        B, T, N = ctx.dims
        C, Hp, k, rows = x.shape[1], W1h.shape[0], Pst.shape[0], B * T * N
        dHall = dHall.contiguous()
        dh, part = torch.zeros_like(Hs[0]), torch.empty_like(Hs[0])
        dPre0, dPre1 = x.new_empty(rows, 2 * Hp), x.new_empty(rows, Hp)
        W1hT, W0hT, PT = mirror(W1h, k + 1), mirror(W0h, k + 1), Pst.transpose(1, 2).contiguous()
        for t in reversed(range(T)):
            ops.ccrnn_bwd_cand(PT, W1hT, dh, U[t], Cc[t], R[t], Hs[t], t, dPre1, dPre0, part, B, T, N, dh2=dHall[t], tiles=TILES)
            if t > 0:                                                      # (h_0 = 0 takes no gradient)
                ops.ccrnn_bwd_state(PT, W0hT, dPre0, part, t, dh, B, T, N, tiles=TILES)
        need = ctx.needs_input_grad
        dx = dW0h = dW0x = db0 = dW1h = dW1x = db1 = dP = None
        if any(need[1:7]):
            dW0h, db0 = ops.stgcn_wgrad(dPre0, Z0, (0,), T, N)
            dW1h, db1 = ops.stgcn_wgrad(dPre1, Z1, (0,), T, N)
            dW0x, _ = ops.stgcn_wgrad(dPre0, LX, (0,), T, N, want_bias=False)
            dW1x, _ = ops.stgcn_wgrad(dPre1, LX, (0,), T, N, want_bias=False)
        if need[0] or need[7]:
            G = ops.stgcn_tapgemm(dPre1, W1x.t().contiguous(), None, (0,), ACT_NONE, T, N)
            G = ops.stgcn_tapgemm(dPre0, W0x.t().contiguous(), None, (0,), ACT_NONE, T, N, res=G, res_w=G.shape[1])
            if need[0]:
                dx = ops.stgcn_nodemix(Pfull.transpose(1, 2).contiguous(), G, N, C, reduce=True)
            if need[7]:
                dP = ops.mtgnn_graphgrad(G, x, N, C, k, dcol0=C)
                dP = dP + _graph_grad(dPre0, W0h, Z0, Hp, k, T, N) + _graph_grad(dPre1, W1h, Z1, Hp, k, T, N)
                dP = _padded(dP, Pst.shape[1])
        return dx, dW0h, dW0x, db0, dW1h, dW1x, db1, dP, None, None


class _DecoderFn(torch.autograd.Function):
    """all steps of all decoder layers: h0 (L, B N, Hp) -> the top layer's state of every step (P, B N, Hp).  ``wts``: per layer W0 (2 Hp, M Ks),
    b0, W1 (Hp, M Ks), b1 over [h | input] slabs; tp (P, B N, Cp) the targets in step layout (or None); forced[t]: step t + 1 reads tp[t]"""

    @staticmethod
    def forward(ctx, h0, Wout, bout, Pst, tp, forced, dims, keep, *wts):
        B, P, N = dims
        L, S, Hp = h0.shape
        k, rows, Cp0 = Pst.shape[0], B * P * N, Wout.shape[0]
        keep = keep and any(ctx.needs_input_grad)
        wts = [w.contiguous() for w in wts]
        Wout, bout = Wout.contiguous(), bout.contiguous()
        Hs = h0.new_empty(L, P + 1, S, Hp)
        Hs[:, 0] = h0
        Inp0 = h0.new_zeros(P, S, Cp0)                                       # layer 0's input of every step: zero, a target, or the feedback
        fed = [t > 0 and not forced[t - 1] for t in range(P)]
        for t in range(1, P):
            if forced[t - 1]:
                Inp0[t] = tp[t - 1]
        U = R = Cc = None
        Z0, Z1 = [None] * L, [None] * L
        if keep:
            U, R, Cc = h0.new_empty(L, P, S, Hp), h0.new_empty(L, P, S, Hp), h0.new_empty(L, P, S, Hp)
            Z0 = [h0.new_empty(rows, wts[4 * l].shape[1]) for l in range(L)]
            Z1 = [h0.new_empty(rows, wts[4 * l].shape[1]) for l in range(L)]
        else:
            ubuf = h0.new_empty(S, Hp)
        q = h0.new_empty(S, Hp)
        for t in range(P):
            for l in range(L):
                W0, b0, W1, b1 = wts[4 * l:4 * l + 4]
                u = U[l, t] if keep else ubuf
                inp = Inp0[t] if l == 0 else Hs[l - 1, t + 1]
                if l == 0 and fed[t]:
                    ops.ccrnn_fwd_gates(Pst, W0, Hs[l, t], b0, t, u, q, B, P, N, fb=(Hs[L - 1, t], Wout, bout), inp_out=Inp0[t],
                                        r=R[l, t] if keep else None, z=Z0[l], tiles=TILES)
                else:
                    ops.ccrnn_fwd_gates(Pst, W0, Hs[l, t], b0, t, u, q, B, P, N, inp=inp, r=R[l, t] if keep else None, z=Z0[l], tiles=TILES)
                ops.ccrnn_fwd_state(Pst, W1, q, b1, t, u, Hs[l, t], Hs[l, t + 1], B, P, N, inp=inp, c=Cc[l, t] if keep else None, z=Z1[l],
                                    tiles=TILES)
        if keep:
            ctx.dims, ctx.fed, ctx.L = dims, fed, L
            ctx.save_for_backward(Wout, Pst, Hs, U, R, Cc, *wts, *Z0, *Z1)
        return Hs[L - 1, 1:]

    @staticmethod
    def backward(ctx, dHtop):
        L, fed = ctx.L, ctx.fed
        Wout, Pst, Hs, U, R, Cc = ctx.saved_tensors[:6]
        wts, Z0, Z1 = ctx.saved_tensors[6:6 + 4 * L], ctx.saved_tensors[6 + 4 * L:6 + 5 * L], ctx.saved_tensors[6 + 5 * L:]
        B, P, N = ctx.dims
        S, Hp, k, rows, Cp0 = Hs.shape[2], Hs.shape[3], Pst.shape[0], B * P * N, Wout.shape[0]
        dHtop = dHtop.contiguous()
        PT = Pst.transpose(1, 2).contiguous()
        W0T, W1T = [mirror(wts[4 * l], k + 1) for l in range(L)], [mirror(wts[4 * l + 2], k + 1) for l in range(L)]
        dh, part = [torch.zeros_like(Hs[0, 0]) for _ in range(L)], torch.empty_like(Hs[0, 0])
        Dinp0 = Hs.new_zeros(P, S, Cp0)                                      # the gradient of layer 0's input of every step
        dinp = [None] + [Hs.new_empty(S, Hp) for _ in range(1, L)]
        dPre0, dPre1 = [Hs.new_empty(rows, 2 * Hp) for _ in range(L)], [Hs.new_empty(rows, Hp) for _ in range(L)]
        for t in reversed(range(P)):
            for l in reversed(range(L)):
                din = Dinp0[t] if l == 0 else dinp[l]
                ops.ccrnn_bwd_cand(PT, W1T[l], dh[l], U[l, t], Cc[l, t], R[l, t], Hs[l, t], t, dPre1[l], dPre0[l], part, B, P, N,
                                   dh2=dHtop[t] if l == L - 1 else dinp[l + 1], dinp=din, tiles=TILES)
                ops.ccrnn_bwd_state(PT, W0T[l], dPre0[l], part, t, dh[l], B, P, N, dinp=din, tiles=TILES)
            if fed[t]:                                                     # the input was out(h_top of step t - 1): its gradient joins that state's
                dh[L - 1].addmm_(Dinp0[t], Wout)
        need = ctx.needs_input_grad
        dWout = dbout = dP = None
        idx = [t for t in range(P) if fed[t]]
        if need[1] or need[2]:
            if idx:
                sel = torch.tensor(idx, device=Hs.device)
                D = Dinp0.index_select(0, sel).reshape(-1, Cp0)
                dWout, dbout = D.t().mm(Hs[L - 1].index_select(0, sel).reshape(-1, Hp)), D.sum(0)
            else:
                dWout, dbout = torch.zeros_like(Wout), Wout.new_zeros(Cp0)
        dw = [None] * (4 * L)
        if any(need[8:]):
            for l in range(L):
                dw[4 * l], dw[4 * l + 1] = ops.stgcn_wgrad(dPre0[l], Z0[l], (0,), P, N)
                dw[4 * l + 2], dw[4 * l + 3] = ops.stgcn_wgrad(dPre1[l], Z1[l], (0,), P, N)
        if need[3]:
            dP = 0
            for l in range(L):
                Ks = wts[4 * l].shape[1] // (k + 1)
                dP = dP + _graph_grad(dPre0[l], wts[4 * l], Z0[l], Ks, k, P, N) + _graph_grad(dPre1[l], wts[4 * l + 2], Z1[l], Ks, k, P, N)
            dP = _padded(dP, Pst.shape[1])
        return (torch.stack(dh, 0) if need[0] else None, dWout, dbout, dP, None, None, None, None, *dw)


class _ZeroGradFn(torch.autograd.Function):
    """y unchanged; the parameters nothing read take a zero gradient, as they do on the torch backend"""

    @staticmethod
    def forward(ctx, y, *unused):
        ctx.save_for_backward(*unused)
        return y.view_as(y)

    @staticmethod
    def backward(ctx, dy):
        return (dy,) + tuple(torch.zeros_like(p) for p in ctx.saved_tensors)


def slab_widths(model):
    """the input width Cp inside the slab of every decoder layer: dim_out padded for layer 0, Hp above"""
    return [pad16(model.output_dim)] + [pad16(model.hidden_size)] * (model.n_rnn_layers - 1)


def supported(model, x):
    """the HIP path serves: one graph-conv layer, one support, k_hop 1..3, one or two RNN layers, hidden_size <= 32, dim_out <= 16; CUDA fp32 4-D
    input of the module's own N, dim_in a multiple of 16 up to 128; any N whose operand slabs fit the 160 KB of LDS"""
    if model.n_gconv_layers != 1 or model.n_supports != 1 or model.n_rnn_layers not in (1, 2) or not 1 <= model.k_hop <= 3:
        return False
    if not 1 <= model.hidden_size <= 32 or not 1 <= model.output_dim <= 16 or not is_hip_input(x):
        return False
    B, T, N, C = x.shape
    if (N, C) != (model.num_nodes, model.input_dim) or T < 1 or not widths_ok([C]) or not 1 <= B <= 65535:
        return False
    return nodemix_fits(N) and 0 < _C.lib().value("gptst_ccrnn_lds_bytes", N, pad16(model.hidden_size), max(slab_widths(model)), model.k_hop, B) <= LDS_MAX


def forward(model, x, keep=True, targets=None, forced=None):
    """predictors.ccrnn.CCRNN.forward on the kernels: x (B, T, N, dim_in) -> (B, num_predict, N, dim_out).  forced: the teacher-forcing decision
    of every step, drawn by the module.  keep = False (no_grad, eval mode): no launch writes anything for a backward and nothing is saved"""
    _C.lib()
    B, T, N, C = x.shape
    H, k, P, OUT, L = model.hidden_size, model.k_hop, model.num_predict, model.output_dim, model.n_rnn_layers
    Hp, M, Np = pad16(H), k + 1, pad16(N)
    S0 = F.leaky_relu(torch.mm(model.nodevec1, model.nodevec2))
    Pst = F.pad(poly_stack(S0, k), (0, Np - N, 0, Np - N))

    xs, last = x.contiguous().view(B * T * N, C), []
    for l, cell in enumerate(model.encoder):
        Cin = C if l == 0 else H
        ru, cd = cell.ru_gate_g_conv.graphconv[0].out, cell.candidate_g_conv.graphconv[0].out
        W0h, W0i, b0 = pack_cell(ru.weight, ru.bias, Cin, H, 2, M)
        W1h, W1i, b1 = pack_cell(cd.weight, cd.bias, Cin, H, 1, M)
        Cx = pad16(Cin)
        W0x, W1x = (F.pad(W, (0, Cx - Cin)).reshape(W.shape[0], M * Cx) for W in (W0i, W1i))
        Hall = _EncLayerFn.apply(xs, W0h.reshape(2 * Hp, M * Hp), W0x, b0, W1h.reshape(Hp, M * Hp), W1x, b1, Pst, (B, T, N), keep)
        last.append(Hall[-1])
        if l + 1 < L:
            xs = Hall.view(T, B, N, Hp).permute(1, 0, 2, 3).reshape(B * T * N, Hp)

    wts, Cps = [], slab_widths(model)
    for l in range(L):                                                     # (the decoder's ModuleList holds ``out`` too)
        cell = model.decoder[l]
        Cin = OUT if l == 0 else H
        ru, cd = cell.ru_gate_g_conv.graphconv[0].out, cell.candidate_g_conv.graphconv[0].out
        W0h, W0i, b0 = pack_cell(ru.weight, ru.bias, Cin, H, 2, M)
        W1h, W1i, b1 = pack_cell(cd.weight, cd.bias, Cin, H, 1, M)
        wts += [slab_weight(W0h, W0i, Cps[l]), b0, slab_weight(W1h, W1i, Cps[l]), b1]
    out = model.decoder.out
    Wout, bout = F.pad(out.weight, (0, Hp - H, 0, Cps[0] - OUT)), F.pad(out.bias, (0, Cps[0] - OUT))
    forced = [False] * P if forced is None else [bool(f) for f in forced]
    tp = None
    if targets is not None and any(forced):
        tp = F.pad(targets.detach().to(x.dtype).permute(1, 0, 2, 3).reshape(P, B * N, OUT), (0, Cps[0] - OUT)).contiguous()
    Htop = _DecoderFn.apply(torch.stack(last, 0), Wout, bout, Pst, tp, forced, (B, P, N), keep, *wts)
    y = out(Htop[..., :H]).view(P, B, N, OUT).permute(1, 0, 2, 3)
    if keep:
        att = [p for cells in (model.encoder, model.decoder) for cell in list(cells)[:L] for conv in (cell.ru_gate_g_conv, cell.candidate_g_conv)
               for p in conv.attlinear.parameters() if p.requires_grad]
        if att:
            y = _ZeroGradFn.apply(y, *att)
    return y
