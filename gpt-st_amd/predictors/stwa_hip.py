"""The ST-WA predictor on HIP (csrc/stwa.hip), forward and backward: what ``STWA(..., backend="hip")`` runs on CUDA fp32 input.

The three Layers run on the kernels, cut by cut (12 + 3 + 1 strictly sequential cuts: cut i reads out_{i-1}).  The generated per-(sample, node)
weights never exist: the last Linear of a generator is ``Linear(5, C C)``, so with the trunk's output co (B, N, 5)

    x W(b, n) + bias(b, n) = x V_0 + sum_k co[b, n, k] (x V_k) + u_0 + sum_k cb[b, n, k] u_k        (``pack``, ``coefficients``)

and a thread folds its column of W(b, n) from the six shared V_k in registers.  The N x N scores of the spatial attention are recomputed from
the sample's keys and values in LDS, forward and backward (the forward keeps each softmax row's maximum and sum).

Per cut, forward     TWO launches:   ops.stwa_local_fwd    rows, the temporal keys / values and softmax, projection1 -> tanh -> projection2, the spatial
                                                           keys and values                                       -> T, Ks, Vs (B, 2, N, C)
                                     ops.stwa_spatial_fwd  the softmax over the nodes, projection1 -> relu -> projection2, the gate, the sum over the
                                                           proxies                                               -> slot i of the layer's output
Per cut, backward    THREE launches, cuts in reverse:
                                     ops.stwa_spatial_bwd_q   the gate and the spatial projections backwards, the query side of the attention
                                     ops.stwa_spatial_bwd_kv  the key / value side: a thread owns a key and sweeps the queries in index order
                                     ops.stwa_local_bwd       the node-local half (its forward recomputed): dh rows, the proxies' gradient, dco, dcb, the
                                                              gradient handed to cut i - 1 through out_{i-1}
One training step is 2 x 16 + 3 x 16 = 80 launches of this family.  Weight gradients (dV, du, the six shared C x C Linears) are per-workgroup
partials: a workgroup adds into its own slab across the cut launches of a layer, and the slabs are summed once per layer (``slab.sum(0)``);
the proxies' gradient is written per sample and summed once per layer.  No float atomics anywhere: a repeated step is bit-identical.
Parameters that take no gradient get no slab and no weight-gradient phase; the input's gradient does not depend on that.

Two gradients are exactly zero and are left there rather than computed to rounding: the temporal key's bias (generator 0: ``du[0]`` and its
share of dcb) and the node-independent part of the spatial key's bias (``du[2, 0]``) — a bias common to all keys of a query cancels in the
softmax.

Kept in torch autograd (rocBLAS-sized or tiny): ``eval_dimin``, the two estimators and the reparameterisations; the generator trunks
M -> 32 -> 5 (co, cb (B, N, 4, 5) per layer); ``start_fc``; the three skip Linears; the ``projections`` head; and the packing of V (4, 6, C, C)
and u (4, 6, C) from the generators' last Linears — plain differentiable tensor ops, so their gradients flow back to the parameters, which
keep the reference's shapes.

Kept for the backward, per cut: T, Ks, Vs, the mixed values S (B, 2, N, C) and the softmax maxima and sums (B, 2, N, 8).  Without a backward to
serve (no_grad, eval mode: the module passes keep = False) the same launches run and nothing is written for one.

LDS: ``gptst_stwa_lds_bytes(N, C)`` is the widest of the five launches — the sample's K and V (or T and dS) of both proxies, 16 N C bytes, plus
the tile's arrays or the per-row statistics: 119 168 bytes at N = 266, C = 16 (the launches opt in to dynamic LDS above 64 KB).  ``supported`` refuses
what exceeds the 160 KB of a CU; such a call takes the module's torch ops.
"""
import torch

from .. import _C, ops
from .rows_hip import LDS_MAX, is_hip_input
from .stwa import reparameterize

WIDTHS = (16, 32)          # channels the kernels are compiled for (head width 2 or 4)
MAX_CUT = 6                # data rows of a cut (csrc/stwa.hip SW_RC - 2)


def pack(layer):
    """The layer's parameters in the kernels' form: V (4, 6, C, C) with V[g, 0] = weight_generator[4].bias as a matrix and V[g, 1 + k][i, j] =
    weight_generator[4].weight[i C + j, k];  u (4, 6, C) likewise from bias_generator[4];  Wl (6, C, C), bl (6, C) = the temporal projections,
    the spatial projections, the aggregator's two Linears.  g = temporal key, temporal value, spatial key, spatial value."""
    C = layer.dim
    V, u = [], []
    for g in layer.generators():
        w, b = g.weight_generator[4], g.bias_generator[4]
        V.append(torch.cat([w.bias.view(1, C, C), w.weight.view(C, C, 5).permute(2, 0, 1)]))
        u.append(torch.cat([b.bias.view(1, C), b.weight.t()]))
    lin = [layer.temporal_att.projection1, layer.temporal_att.projection2, layer.spatial_att.projection1, layer.spatial_att.projection2,
           layer.aggregator[0], layer.aggregator[2]]
    return torch.stack(V), torch.stack(u), torch.stack([m.weight for m in lin]), torch.stack([m.bias for m in lin])


def coefficients(layer, z):
    """co, cb (B, N, 4, 5): the generator trunks M -> 32 -> 5 (both ReLUs included) on the memory z (B, N, M)"""
    gens = layer.generators()
    return (torch.stack([g.weight_generator[:4](z) for g in gens], dim=2), torch.stack([g.bias_generator[:4](z) for g in gens], dim=2))


class _LayerFn(torch.autograd.Function):
    """One Layer: h (B, T, N, C), prox (2 cuts, N, C), co, cb (B, N, 4, 5), V, u, Wl, bl (``pack``) -> (B, cuts, N, C)"""

    @staticmethod
    def forward(ctx, h, prox, co, cb, V, u, Wl, bl, dims, keep):
        cuts, cs = dims
        B, T, N, C = h.shape
        keep = keep and any(ctx.needs_input_grad[:8])
        h, prox, co, cb, V, u, Wl, bl = (t.contiguous() for t in (h, prox, co, cb, V, u, Wl, bl))
        WlT = Wl.transpose(1, 2).contiguous()
        Y = h.new_empty(B, cuts, N, C)
        lead = (cuts,) if keep else (1,)
        Tq, Ks, Vs = (h.new_empty(lead + (B, 2, N, C)) for _ in range(3))
        S = h.new_empty(cuts, B, 2, N, C) if keep else None
        mx, sm = (h.new_empty(cuts, B, 2, N, 8) for _ in range(2)) if keep else (None, None)
        for i in range(cuts):
            k = i if keep else 0
            ops.stwa_local_fwd(h, prox, Y, co, cb, V, u, WlT, bl, Tq[k], Ks[k], Vs[k], i, cs)
            ops.stwa_spatial_fwd(Tq[k], Ks[k], Vs[k], WlT, bl, Y, i, S=S[i] if keep else None, mx=mx[i] if keep else None,
                                 sm=sm[i] if keep else None)
        if keep:
            ctx.dims = dims
            ctx.save_for_backward(h, prox, co, cb, V, u, Wl, WlT, bl, Y, Tq, Ks, Vs, S, mx, sm)
        return Y

    @staticmethod
    def backward(ctx, dY):
        h, prox, co, cb, V, u, Wl, WlT, bl, Y, Tq, Ks, Vs, S, mx, sm = ctx.saved_tensors
        cuts, cs = ctx.dims
        B, T, N, C = h.shape
        need = ctx.needs_input_grad
        dY = dY.contiguous()
        slab = h.new_zeros(ops.stwa_slab_shape(B, N, C)) if any(need[4:8]) else None
        dh = torch.zeros_like(h) if need[0] else None                      # (rows past the last cut are read by nothing: their gradient is 0)
        dPb = h.new_empty(B, 2 * cuts, N, C) if need[1] else None
        dco, dcb = torch.zeros_like(co), torch.zeros_like(cb)
        carry = h.new_empty(B, N, C) if cuts > 1 else None
        dS, dTq, dKs, dVs = (h.new_empty(B, 2, N, C) for _ in range(4))
        Dq = h.new_empty(B, 2, N, 8)
        for i in reversed(range(cuts)):
            ops.stwa_spatial_bwd_q(Tq[i], Ks[i], Vs[i], S[i], mx[i], sm[i], Wl, WlT, bl, dY, carry if i < cuts - 1 else None, dS, Dq, dTq, slab, i)
            ops.stwa_spatial_bwd_kv(Tq[i], Ks[i], Vs[i], dS, Dq, mx[i], sm[i], dKs, dVs)
            ops.stwa_local_bwd(h, prox, Y, co, cb, V, u, Wl, WlT, bl, dTq, dKs, dVs, dh, dPb, carry if i > 0 else None, dco, dcb, slab, i, cs)
        g = [dh, dPb.sum(0) if need[1] else None, dco if need[2] else None, dcb if need[3] else None, None, None, None, None, None, None]
        if slab is not None:
            s = slab.sum(0)                                                # the one reduction of the layer, in a fixed order
            nV, nu, nW = 24 * C * C, 24 * C, 6 * C * C
            g[4], g[5] = s[:nV].view(4, 6, C, C), s[nV:nV + nu].view(4, 6, C).clone()
            g[5][2, 0] = 0                                                 # the node-independent part of the spatial key's bias: exactly 0
            g[6], g[7] = s[nV + nu:nV + nu + nW].view(6, C, C), s[nV + nu + nW:].view(6, C)
        return tuple(g)


def plan(N, C):
    """the dynamic LDS, in bytes, of the widest launch at this shape (the one source: csrc/stwa.hip); negative where C is not a kernel width"""
    return _C.lib().value("gptst_stwa_lds_bytes", N, C)


def supported(model, x):
    """the HIP path serves: CUDA fp32 4-D input of the module's own (N, dim_in), channels 16 or 32, any lag >= 1, any B up to 65535, any
    memory_size, and any N whose sample fits the 160 KB of LDS"""
    if not is_hip_input(x):
        return False
    B, T, N, D = x.shape
    if (N, D) != (model.num_nodes, model.input_dim) or T != model.lag or model.channels not in WIDTHS or not 1 <= B <= 65535:
        return False
    if any(layer.cut_size > MAX_CUT for layer in model.layers):
        return False
    return 0 < plan(N, model.channels) <= LDS_MAX


def forward(model, x, keep=True, noise=None):
    """predictors.stwa.STWA.forward on the kernels: x (B, lag, N, dim_in) -> (B, horizon, N, out_dim), with the noise the module drew.
    keep = False (no_grad, eval mode): no launch writes anything for a backward and nothing is saved"""
    _C.lib()
    eps_d, eps_l = noise
    B, N = x.shape[0], model.num_nodes
    z_data = model.z_data(x, eps_d)
    h = model.start_fc(x)
    skip = 0
    for layer, skip_layer, eps in zip(model.layers, model.skip_layers, eps_l):
        z = z_data + reparameterize(layer.mu, layer.logvar, eps)
        co, cb = coefficients(layer, z)
        h = _LayerFn.apply(h, layer.proxies[0], co, cb, *pack(layer), (layer.cuts, layer.cut_size), keep)
        skip = skip + skip_layer(h.transpose(2, 1).reshape(B, N, -1))
    return model.head(skip, B)
