"""The MSDR predictor on HIP (csrc/msdr.hip + the hoisted kernels of csrc/stgcn.hip and csrc/mtgnn.hip), forward and backward: what
``MSDR(..., backend="hip")`` runs on CUDA fp32 input.

Layer l never reads layer l + 1, and the decoder is not autoregressive (its step t reads the encoder's top output of step t), so the model is
four recurrences run one after the other — encoder 0, encoder 1, decoder 0, decoder 1 — each a ``_CellFn`` with its input half hoisted.
Rows are TIME-major inside, (t, b, n): the state ring ``Hs`` (T + K, B N, Hp) holds the K initial states and then every output, so ``Hs[K:]``
IS the next recurrence's input sequence and the first ``horizon`` steps of the encoder's top output are a prefix of it.  ``rnn_units`` d is
zero-padded to Hp = 16 ceil(d / 16) inside the PACKED weights only (``pack``): a padded channel stays exactly 0 — its Theta rows and columns,
beta, W, b, R and w are 0, so pre = 0, c = leaky_relu(0) = 0 and o = 0 W + 0 + sum a_k (0 + 0) — and the packing, being plain
differentiable tensor ops, drops its gradients on the way back to the parameters, which keep the reference's shapes.

Per recurrence, with Lp = [the fixed supports | A] zero-padded and M = [I | Lp]:
    hoisted forward     [U | Lp U] (stgcn_nodemix) and Gx = [U | Lp U] Px^T + beta (stgcn_tapgemm) over all T B units; wr_k = w . R_k + bias
    per step, forward   ONE launch (ops.msdr_fwd_step): the state-side product, leaky_relu, W, b, the attention mix, the partials of w . o
    per step, backward  TWO launches (ops.msdr_bwd_pre, ops.msdr_bwd_state)
    hoisted backward    dTheta, dbeta: stgcn_wgrad of dPre against [U | Lp U] and the kept [h | Lp h]; dW: stgcn_wgrad of dO against c;
                        dU = dPre Px (two stgcn_tapgemm) folded through Lp^T (stgcn_nodemix, reduce); dA: mtgnn_graphgrad on the input and on
                        the state side; db, dR, dw: sums over the T B units of dO, a, de (torch reductions, a fixed order); attlinear.bias: exactly 0
Kept in torch autograd: A's own chain softmax(relu(E1 E2)), the projection head (output_dim is 1 or 2: not a kernel width), the packing.
The encoder's ``mlp`` is a tap GEMM (rows_hip.TapFn).

Kept for the backward: the ring, c and a of every step, and — only when Theta takes a gradient — [U | Lp U] and [h | Lp h].  Without a backward
to serve (no_grad, eval mode: the module passes keep = False) the same launches run and nothing is written for one.
"""
import torch
import torch.nn.functional as F

from .. import _C, ops
from ..ops import ACT_NONE
from .rows_hip import LDS_MAX, TapFn, is_hip_input, nodemix_fits, pad16, padded_graph, widths_ok

MAX_K = 8                  # kept states a step launch folds (csrc/msdr.hip MS_MAXK)


def pack(cell, d, Hp, M):
    """The cell's parameters in the kernels' form: Px, Ph (Hp, M Hp) = the input and the state rows of Theta as GEMM weights, output channel
    by row, column m Hp + i = (matrix m, channel i);  beta (Hp);  W2 (Hp, Hp) = W^T;  b, w (N, Hp);  R (K, N, Hp).  Padding is zero."""
    N, p = cell.num_nodes, Hp - d
    th = cell.theta.view(2, d, M, d).permute(0, 3, 2, 1)                   # (half, out j, matrix m, in i)
    th = F.pad(th, (0, p, 0, 0, 0, p)).reshape(2, Hp, M * Hp)
    return (th[0].contiguous(), th[1].contiguous(), F.pad(cell.beta, (0, p)), F.pad(cell.W.t(), (0, p, 0, p)).contiguous(),
            F.pad(cell.b, (0, p)), F.pad(cell.R, (0, p)), F.pad(cell.attlinear.weight.view(N, d), (0, p)))


class _CellFn(torch.autograd.Function):
    """One recurrence: U (T B N, Hp), the K initial states S0 (K, B N, Hp) with the partials of their logits sig0 (K, B, G) -> the ring Hs
    (T + K, B N, Hp) and, where w2 is given, the partials of w2 . o for the recurrence that starts from these states (not differentiable:
    that recurrence accounts for them itself)"""

    @staticmethod
    def forward(ctx, U, S0, sig0, Px, Ph, beta, W2, bvec, R, w, abias, A, w2, Lfix, LfixT, dims, keep):
        B, T, N = dims
        K, Hp, rows = R.shape[0], U.shape[1], T * B * N
        need = ctx.needs_input_grad
        keep = keep and any(need)
        need_theta, need_A = keep and any(need[3:6]), keep and need[11]
        Np = Lfix.shape[1]
        Ap = F.pad(A, (0, Np - N, 0, Np - N))[None]
        Lp = torch.cat([Lfix, Ap]).contiguous()
        ks = Lp.shape[0]
        Zx = torch.cat([U, ops.stgcn_nodemix(Lp, U, N, Hp, reduce=False)], dim=1)
        Gx = ops.stgcn_tapgemm(Zx, Px, beta.contiguous(), (0,), ACT_NONE, T, N)
        wr = ((w * R).sum(dim=(1, 2)) + abias).contiguous()
        G = ops.msdr_groups(N, B)
        Hs, sig = U.new_empty(T + K, B * N, Hp), U.new_empty(T + K, B, G)
        Hs[:K], sig[:K] = S0, sig0
        sig2 = None
        if w2 is not None:                                                 # (with T < K some of the initial states are still among the final ones)
            sig2 = torch.empty_like(sig)
            sig2[:K] = 0
            sig2[:K, :, 0] = torch.mv(S0.reshape(K * B, N * Hp), w2.reshape(-1)).view(K, B)
        Cc = U.new_empty(rows, Hp) if keep else None
        att = U.new_empty(T, B, K) if keep else None
        Zh = U.new_empty(rows, (ks + 1) * Hp) if need_theta else None
        bvec, R, w, W2 = bvec.contiguous(), R.contiguous(), w.contiguous(), W2.contiguous()
        w2 = w2.contiguous() if w2 is not None else None
        for t in range(T):
            ops.msdr_fwd_step(Lp, Ph, W2, bvec, R, w, wr, Gx, Hs, sig, t, B, T, N, w2=w2, sig2=sig2, c=Cc, z=Zh, a=att)
        if keep:
            ctx.dims = dims
            LpT = torch.cat([LfixT, Ap.transpose(1, 2)]).contiguous()
            ctx.save_for_backward(Hs, Cc, att, Zx if need_theta else None, Zh, U if need_A else None, Px, Ph, W2, R, w, LpT)
        if sig2 is None:
            sig2 = sig.new_empty(0)
        ctx.mark_non_differentiable(sig2)
        return Hs, sig2

    @staticmethod
    def backward(ctx, dHs, _):
        Hs, Cc, att, Zx, Zh, U, Px, Ph, W2, R, w, LpT = ctx.saved_tensors
        B, T, N = ctx.dims
        K, Hp, rows, ks = R.shape[0], R.shape[2], T * B * N, LpT.shape[0]
        need = ctx.needs_input_grad
        dH = dHs.contiguous().clone()
        dPre, de = dH.new_empty(rows, Hp), dH.new_empty(T, B, K)
        pa = dH.new_empty(B, ops.msdr_groups(N, B), 8)
        Wm = W2.t().contiguous()                                           # W itself: dc = dO W^T
        PhT = Ph.view(Hp, ks + 1, Hp).permute(2, 1, 0).reshape(Hp, (ks + 1) * Hp).contiguous()
        for t in reversed(range(T)):
            ops.msdr_bwd_pre(Wm, R, Hs, dH, Cc, dPre, pa, t, B, T, N)
            ops.msdr_bwd_state(LpT, PhT, w, att, pa, dPre, dH, de, t, B, T, N)
        dO = dH[K:].view(rows, Hp)                                         # slot K + t is final once step t has run: the whole gradient of o_t
        g = [None] * 17
        if need[1]:
            g[1] = dH[:K]
        if any(need[3:6]):
            g[3], g[5] = ops.stgcn_wgrad(dPre, Zx, (0,), T, N)
            g[4], _ = ops.stgcn_wgrad(dPre, Zh, (0,), T, N, want_bias=False)
        if need[6]:
            g[6], _ = ops.stgcn_wgrad(dO, Cc, (0,), T, N, want_bias=False)       # (j, i) = sum dO[., j] c[., i]: the gradient of W^T
        if need[7]:
            g[7] = dO.view(T * B, N, Hp).sum(0)
        if need[8] or need[9]:
            a2, de2 = att.view(T * B, K), de.view(T * B, K)
            des = de2.sum(0)
            if need[8]:
                g[8] = torch.mm(a2.t(), dO.view(T * B, N * Hp)).view(K, N, Hp) + des.view(K, 1, 1) * w
            if need[9]:
                dw = (des.view(K, 1, 1) * R).sum(0).view(1, N * Hp)
                for k in range(K):
                    dw = dw + torch.mm(de2[:, k:k + 1].t(), Hs[k:k + T].reshape(T * B, N * Hp))
                g[9] = dw.view(N, Hp)
        if need[10]:
            g[10] = torch.zeros(1, device=dH.device, dtype=dH.dtype)           # a constant added to every logit of a softmax: exactly 0
        if need[0] or need[11]:
            G12 = ops.stgcn_tapgemm(dPre, Px[:, Hp:].t().contiguous(), None, (0,), ACT_NONE, T, N)
            if need[0]:
                G0 = ops.stgcn_tapgemm(dPre, Px[:, :Hp].t().contiguous(), None, (0,), ACT_NONE, T, N)
                g[0] = ops.stgcn_nodemix(LpT, G12, N, Hp, reduce=True, res=G0)
            if need[11]:
                GAh = ops.stgcn_tapgemm(dPre, Ph[:, ks * Hp:].t().contiguous(), None, (0,), ACT_NONE, T, N)
                g[11] = (ops.mtgnn_graphgrad(G12, U, N, Hp, 1, dcol0=(ks - 1) * Hp)[0]
                         + ops.mtgnn_graphgrad(GAh, Hs[K - 1:K - 1 + T].view(rows, Hp), N, Hp, 1)[0])
        return tuple(g)


def supported(model, x):
    """the HIP path serves: CUDA fp32 4-D input of the module's own (T, N, C), pre_v = 1 and max_diffusion_step = 1, one or two fixed
    supports, 1 <= pre_k <= 8, horizon <= seq_len, dim_in a multiple of 16 up to 128, rnn_units <= 128 (any value: it is padded), and any N
    whose operand slabs fit the 160 KB of LDS"""
    if not is_hip_input(x):
        return False
    B, T, N, C = x.shape
    cell = model.encoder_model.gmsdr_layers[0]
    if (T, N, C) != (model.seq_len, model.num_nodes, model.input_dim) or cell.supports.shape[1] != N:
        return False
    if model.pre_v != 1 or model.max_diffusion_step != 1 or not 1 <= cell.supports.shape[0] <= 2 or not 1 <= model.pre_k <= MAX_K:
        return False
    if not widths_ok([C]) or not 1 <= model.rnn_units <= 128 or not 1 <= B <= 65535 or not 1 <= model.horizon <= T:
        return False
    return nodemix_fits(N) and 0 < _C.lib().value("gptst_msdr_lds_bytes", N, pad16(model.rnn_units), B, cell.supports.shape[0] + 1) <= LDS_MAX


def forward(model, x, keep=True):
    """predictors.msdr.MSDR.forward on the kernels: x (B, T, N, dim_in) -> (B, horizon, N, output_dim).  keep = False (no_grad, eval mode): no
    launch writes anything for a backward and nothing is saved"""
    _C.lib()
    B, T, N, C = x.shape
    d, K, P = model.rnn_units, model.pre_k, model.horizon
    Hp = pad16(d)
    enc, dec = model.encoder_model, model.decoder_model
    M = enc.gmsdr_layers[0].num_matrices
    G = ops.msdr_groups(N, B)
    mlp_w, mlp_b = F.pad(enc.mlp.weight, (0, 0, 0, Hp - d)).contiguous(), F.pad(enc.mlp.bias, (0, Hp - d)).contiguous()
    u = TapFn.apply(x.contiguous().view(B * T * N, C), mlp_w, mlp_b, None, (0,), ACT_NONE, 0, T, N, keep)
    inp = u.view(B, T, N, Hp).transpose(0, 1).reshape(T * B * N, Hp)        # time-major from here on
    S0, sig0 = x.new_zeros(K, B * N, Hp), x.new_zeros(K, B, G)

    def run(cell, inp, S0, sig0, w2, steps):
        lf, lft = padded_graph(cell, cell.supports, "_lp_cache", True)
        return _CellFn.apply(inp, S0, sig0, *pack(cell, d, Hp, M), cell.attlinear.bias, cell.adaptive(), w2, lf, lft, (B, steps, N), keep)

    last = []
    for l, cell in enumerate(enc.gmsdr_layers):
        w_next = F.pad(dec.gmsdr_layers[l].attlinear.weight.detach().view(N, d), (0, Hp - d))
        Hs, sig2 = run(cell, inp, S0, sig0, w_next, T)
        inp = Hs[K:].reshape(T * B * N, Hp)
        last.append((Hs[T:], sig2[T:]))                                     # the encoder's final K states of this layer
    inp = inp[:P * B * N]                                                   # decoder step t reads the encoder's top output of step t
    for l, cell in enumerate(dec.gmsdr_layers):
        Hs, _ = run(cell, inp, last[l][0], last[l][1].contiguous(), None, P)
        inp = Hs[K:].reshape(P * B * N, Hp)
    y = dec.projection_layer(inp.view(P, B, N, Hp)[..., :d])
    return y.transpose(0, 1).contiguous()
