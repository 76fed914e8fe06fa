"""The MTGNN predictor on HIP (csrc/mtgnn.hip + the node mix, one-tap GEMM, weight gradient and LayerNorm of csrc/stgcn.hip), forward and
backward: what ``MTGNN(..., backend="hip")`` runs on CUDA fp32 input.

Channels-last rows (b, t, n) as in stgcn_hip.py; no permute is materialised.  Every layer's activation is a dense buffer of its own time
length (19 -> 13 -> 7 -> 1 at the conf): a valid temporal convolution is a tap GEMM whose output frame is shorter than its input frame.

    filter + gate   ONE gated tap GEMM per layer (ops.mtgnn_tapgemm): the four inception kernels of either branch packed right-aligned into a
                    7-tap weight with zeros where a kernel has no tap (``inception_weight``), filter rows then gate rows;
                    g = tanh(P) sigmoid(Q) keep in the epilogue, keep = the dropout multiplier of the site (0 or 1 / (1 - p)).
    skips           whole-axis contractions (T_out = 1; skip0 has K = 20 * dim_in), each adding the running skip in its epilogue; skip0's
                    dropout multiplies its operand inside the kernel.  skipE is one more tap GEMM; the T = output_dim + T = 1 sum is a broadcast add.
    mix-hop         Z = [x | M1 x | M2 x | M1' x | M2' x] in one stgcn_nodemix expand (M1 = alpha I + (1 - alpha) a, M2 = alpha I + alpha (1 - alpha) a
                    + (1 - alpha)^2 a^2 for a = the normalised adp, M' the same for adp^T; the identity is the first "graph" so that both 1x1
                    ``mlp``s become ONE GEMM over Z with the cropped residual in its epilogue).  This re-associates a (a x) as a^2 x.
    backward        dZ = dY Wm^T (stgcn_tapgemm), dWm (stgcn_wgrad), dM_k = sum dZ_k x^T (mtgnn_graphgrad: the graph is learned),
                    dg = sum_k M_k^T dZ_k + the skip's gradient (stgcn_nodemix, reduce), dPre (mtgnn_gate_bwd), dW, db of the packed inception
                    weight (mtgnn_wgrad), dX = the mirrored tap GEMM of dPre with dY, the residual's gradient, in its epilogue.
    in torch        the graph constructor and its top-k (N x 40), M1 / M2 from adp (N x N; their backward is autograd's and receives dM_k),
                    the weight packing (which carries the packed gradients back to the parameters), the left pad of the input, the head's two
                    1x1 convolutions (torch.addmm) and the LayerNorm weights' (C, N, T) -> (T, N, C) repack.
    LayerNorm       stgcn_ln_fwd / bwd / bwd_param with units = B and M = T N C.

Dropout masks come from the module's ``_keep(tag, like)`` hook with ``like`` in THIS layout, (B, T, N, C): the default draws them with
``F.dropout`` on the device, a stream of its own that is not claimed equal to the torch backend's.
Kept for the backward: every layer's input, tanh, sigmoid, g and Z, the LayerNorm's mean and rstd.  Without a backward to serve (no_grad, eval
mode: the module passes keep = False) the same launches run and nothing is kept.
"""
import torch
import torch.nn.functional as F

from .. import _C, ops
from .mtgnn import KERNEL_SET, MixProp
from .rows_hip import LNFn, is_hip_input, mirror as _mirror, nodemix_fits, pad16, widths_ok

MAX_TAPS = 32


def inception_weight(filt, gate):
    """two DilatedInception modules -> (W (2 cout, 7 * cin) tap-major, b (2 cout), offs): kernel k of ``kern`` taps occupies tap slots
    7 - kern .. 6 (cropping every output to the 7-tap length right-aligns the kernels), zeros elsewhere; filter rows, then gate rows"""
    K = KERNEL_SET[-1]

    def one(m):
        ws = [F.pad(conv.weight[:, :, 0, :].permute(0, 2, 1), (0, 0, K - conv.kernel_size[1], 0)) for conv in m.tconv]      # (cout / 4, 7, cin)
        return torch.cat(ws, 0), torch.cat([conv.bias for conv in m.tconv])
    (wf, bf), (wg, bg) = one(filt), one(gate)
    W = torch.cat([wf, wg], 0)
    d = filt.tconv[0].dilation[1]
    return W.reshape(W.shape[0], -1), torch.cat([bf, bg]), tuple(d * s for s in range(K))


def time_weight(conv):
    """a (1, k) convolution -> (W (cout, k * cin) tap-major, b, offs = 0 .. k - 1)"""
    w = conv.weight[:, :, 0, :].permute(0, 2, 1)
    return w.reshape(w.shape[0], -1), conv.bias, tuple(range(conv.kernel_size[1]))


def mix_graphs(adp, alpha):
    """adp (N, N) -> (4, N, N): [M1(a), M2(a), M1(a'), M2(a')], a = normalised adp, a' = normalised adp^T: h1 = M1 x and h2 = M2 x of a MixProp"""
    eye = torch.eye(adp.shape[0], dtype=adp.dtype, device=adp.device)
    out = []
    for adj in (adp, adp.transpose(1, 0)):
        a = MixProp.normalised(adj)
        out += [alpha * eye + (1 - alpha) * a, alpha * eye + alpha * (1 - alpha) * a + (1 - alpha) ** 2 * (a @ a)]
    return torch.stack(out)


def mix_weight(g1, g2):
    """the two MixProp ``mlp``s over [x | h1 | h2] -> one GEMM over [x | M1 x | M2 x | M1' x | M2' x]: (W (cout, 5 cin), b)"""
    w1, w2 = (g.mlp.mlp.weight[:, :, 0, 0] for g in (g1, g2))
    c = w1.shape[1] // 3
    return torch.cat([w1[:, :c] + w2[:, :c], w1[:, c:], w2[:, c:]], 1), g1.mlp.mlp.bias + g2.mlp.mlp.bias


def norm_weight(ln, numel, like):
    """LayerNorm weights (C, N, T) -> (gamma, beta) flat in the rows' order (T, N, C); ones and zeros where the norm has no affine weights"""
    if not ln.elementwise_affine:
        return like.new_ones(numel), like.new_zeros(numel)
    return ln.weight.permute(2, 1, 0).reshape(-1), ln.bias.permute(2, 1, 0).reshape(-1)


class _ConvFn(torch.autograd.Function):
    """y[b, to, n] = sum_j (x xmask)[b, to + offs[j], n] W_j + b + prev[b, to, n]   (valid convolution along time; prev, xmask optional)"""

    @staticmethod
    def forward(ctx, x, W, b, prev, xmask, cfg, keep):
        offs, B, Tsrc, Tdst, N = cfg
        y = ops.mtgnn_tapgemm(x, W, b, offs, B, Tsrc, Tdst, N, xmask=xmask, res=prev)
        if keep and any(ctx.needs_input_grad):
            ctx.cfg = cfg
            ctx.save_for_backward(x, W, xmask)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W, xmask = ctx.saved_tensors
        offs, B, Tsrc, Tdst, N = ctx.cfg
        dy = dy.contiguous()
        dx = dW = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dW, db = ops.mtgnn_wgrad(dy, x, offs, B, Tsrc, Tdst, N, xmask=xmask)
        if ctx.needs_input_grad[0]:
            dx = ops.mtgnn_tapgemm(dy, _mirror(W, len(offs)), None, tuple(-o for o in offs), B, Tdst, Tsrc, N, omask=xmask)
        return dx, dW, db, (dy if ctx.needs_input_grad[3] else None), None, None, None


class _LayerFn(torch.autograd.Function):
    """x (B Tsrc N, R) -> g = tanh(filter(x)) sigmoid(gate(x)) kmask (B Tdst N, C)   and   y = [g | M_k g]_k Wm + bm + x[:, -Tdst:] (B Tdst N, R).
    L4 (4, N, N) are the mix graphs as a function of the parameters (its gradient is what comes back); L5p, L5pT the same with the identity
    in front, zero-padded to 16-node tiles, and their transposes."""

    @staticmethod
    def forward(ctx, x, Wg, bg, kmask, L4, L5p, L5pT, Wm, bm, cfg, keep):
        offs, B, Tsrc, Tdst, N = cfg
        keep = keep and any(ctx.needs_input_grad)
        C = Wg.shape[0] // 2
        tn = s = None
        if keep:
            g, tn, s = ops.mtgnn_tapgemm(x, Wg, bg, offs, B, Tsrc, Tdst, N, gated=True, omask=kmask, keep=True)
        else:
            g = ops.mtgnn_tapgemm(x, Wg, bg, offs, B, Tsrc, Tdst, N, gated=True, omask=kmask)
        Z = ops.stgcn_nodemix(L5p, g, N, C, reduce=False)
        y = ops.mtgnn_tapgemm(Z, Wm, bm, (0,), B, Tdst, Tdst, N, res=x, res_frame=Tsrc, res_off=Tsrc - Tdst)
        if keep:
            ctx.cfg = cfg
            ctx.save_for_backward(x, Wg, kmask, tn, s, g, Z, Wm, L5pT)
        return g, y

    @staticmethod
    def backward(ctx, dg_skip, dy):
        x, Wg, kmask, tn, s, g, Z, Wm, L5pT = ctx.saved_tensors
        offs, B, Tsrc, Tdst, N = ctx.cfg
        need = ctx.needs_input_grad
        C = g.shape[1]
        dy = dy.contiguous()
        dx = dWg = dbg = dL4 = dWm = dbm = None
        if need[7] or need[8]:
            dWm, dbm = ops.stgcn_wgrad(dy, Z, (0,), Tdst, N)
        dZ = ops.stgcn_tapgemm(dy, Wm.t().contiguous(), None, (0,), ops.ACT_NONE, Tdst, N)               # (rows, 5 C): dZ_k = dY Wm_k^T
        if need[4]:
            dL4 = ops.mtgnn_graphgrad(dZ, g, N, C, 4, dcol0=C)
        dg = ops.stgcn_nodemix(L5pT, dZ, N, C, reduce=True, res=dg_skip.contiguous())
        dPre = ops.mtgnn_gate_bwd(dg, tn, s, kmask)
        if need[1] or need[2]:
            dWg, dbg = ops.mtgnn_wgrad(dPre, x, offs, B, Tsrc, Tdst, N)
        if need[0]:
            dx = ops.mtgnn_tapgemm(dPre, _mirror(Wg, len(offs)), None, tuple(-o for o in offs), B, Tdst, Tsrc, N, res=dy, res_frame=Tdst,
                                   res_off=Tdst - Tsrc)
        return dx, dWg, dbg, None, dL4, None, None, dWm, dbm, None, None


def supported(model, x):
    """the HIP path serves: CUDA fp32 4-D input of the module's own (T, N, dim_in); dim_in and every channel width a multiple of 16 up to 128
    (conv_channels divisible by 4 follows); gcn_true with gcn_depth 2; a time axis of at most 32 steps (the tap table); N whose node-mix
    slab fits the LDS"""
    if not is_hip_input(x):
        return False
    if tuple(x.shape[1:]) != (model.input_window, model.num_nodes, model.feature_dim) or not model.gcn_true or model.gcn_depth != 2:
        return False
    widths = (model.feature_dim, model.conv_channels, model.residual_channels, model.skip_channels)
    if not widths_ok(widths) or model.total_window > MAX_TAPS or model.frames[-1] < 1:
        return False
    return nodemix_fits(model.num_nodes)


def forward(model, x, keep=True):
    """predictors.mtgnn.MTGNN.forward on the kernels: x (B, T, N, dim_in) -> (B, output_window, N, output_dim).  keep = False (no_grad, eval
    mode): no launch writes anything for a backward and nothing is saved"""
    _C.lib()
    m = model
    B, T, N, Cin = x.shape
    Tt, R, S = m.total_window, m.residual_channels, m.skip_channels
    xp = F.pad(x, (0, 0, 0, 0, Tt - T, 0)) if Tt > T else x.contiguous()                                 # zeros on the left of the time axis
    kin = m._keep("in", xp)
    xr = xp.view(B * Tt * N, Cin)
    adp = m.adjacency()
    L4 = mix_graphs(adp, m.propalpha)
    pad = pad16(N) - N
    L5p = F.pad(torch.cat([torch.eye(N, dtype=L4.dtype, device=L4.device)[None], L4.detach()]), (0, pad, 0, pad)).contiguous()
    L5pT = L5p.transpose(1, 2).contiguous()

    def conv(c, h, Tsrc, prev=None, xmask=None):
        W, b, offs = time_weight(c)
        return _ConvFn.apply(h, W.contiguous(), b.contiguous(), prev, xmask, (offs, B, Tsrc, Tsrc - len(offs) + 1, N), keep)

    skip = conv(m.skip0, xr, Tt, xmask=None if kin is None else kin.contiguous().view_as(xr))          # (B N, S): T = 1
    h = conv(m.start_conv, xr, Tt)
    for i in range(m.layers):
        Tsrc, Tdst = m.frames[i], m.frames[i + 1]
        Wg, bg, offs = inception_weight(m.filter_convs[i], m.gate_convs[i])
        Wm, bm = mix_weight(m.gconv1[i], m.gconv2[i])
        km = m._keep("l%d" % i, x.new_empty(B, Tdst, N, m.conv_channels))
        g, h = _LayerFn.apply(h, Wg.contiguous(), bg.contiguous(), None if km is None else km.contiguous().view(B * Tdst * N, -1), L4, L5p, L5pT,
                              Wm.contiguous(), bm.contiguous(), (offs, B, Tsrc, Tdst, N), keep)
        skip = conv(m.skip_convs[i], g, Tdst, prev=skip)
        ln = m.norm[i]
        gamma, beta = norm_weight(ln, Tdst * N * R, h)
        h = LNFn.apply(h, gamma.contiguous(), beta.contiguous(), B, ln.eps, keep)
    To = m.frames[-1] - len(time_weight(m.skipE)[2]) + 1
    e = conv(m.skipE, h, m.frames[-1])                                                                  # (B To N, S)
    z = F.relu(e.view(B, To, N, S) + skip.view(B, 1, N, S)).view(B * To * N, S)                          # T = output_dim + T = 1: broadcasts
    e1, e2 = m.end_conv_1, m.end_conv_2
    z = F.relu(torch.addmm(e1.bias, z, e1.weight.view(e1.out_channels, -1).t()))
    y = torch.addmm(e2.bias, z, e2.weight.view(e2.out_channels, -1).t())
    return y.view(B, To, N, e2.out_channels).permute(0, 3, 2, 1)
