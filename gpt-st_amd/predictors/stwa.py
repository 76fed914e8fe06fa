"""ST-WA predictor (Cirstea et al., "Towards Spatio-Temporal Aware Traffic Time Series Forecasting", ICDE 2022) as the reference wires it
behind the enhanced embedding: ``-mode eval -model STWA`` (reference model/ST_WA/ST_WA.py ``STWA``, attention.py, built in
model/Model.py:76-78).  x (B, lag, N, dim_in) -> (B, horizon, N, out_dim).  C = channels, M = memory_size, 8 heads of C / 8:

    xd      = eval_dimin(x)                        (B, lag, N, 1); the Linear exists only where dim_in != 1
    mu_d, logvar_d = the two estimators lag -> 32 -> 32 -> M (tanh) on (B, N, lag)
    z_data  = mu_d + eps_d exp(logvar_d / 2)       eps_d ~ randn (B, N, M)
    h       = start_fc(x)                          (B, lag, N, C), then three Layers of (cuts, cut_size) = (12, 6), (3, 4), (1, 3); after layer
                                                   l the time axis is that layer's ``cuts``
    skip   += skip_layers[l](h.transpose(2, 1).reshape(B, N, cuts C))        widths 12 C, 3 C, C -> 256
    out     = projections(relu(skip))              256 -> 512 -> horizon out_dim, reshaped as at ST_WA.py:91-94 (both branches)

Inside a Layer, z = z_data + mu_l + eps_l exp(logvar_l / 2) with eps_l ~ randn (N, M); four ParameterGenerators (temporal key, temporal
value, spatial key, spatial value) each turn z into a per-sample, per-node weight W (B, N, C, C) and bias (B, N, C) through two MLPs
M -> 32 -> 5 -> C C (and -> C).  Cut i, with out_{-1} = 0:

    rows    = [proxies[2 i : 2 i + 2] + out_{i-1} | h[:, i cs : (i + 1) cs]]          2 + r rows, r = clamp(T - i cs, 0, cs)
    temporal, per node:      q = the 2 raw proxy rows;  K, V = rows W + bias of all 2 + r rows;  softmax over the 2 + r keys of q K / sqrt(C / 8)
                             per head;  o = projection2(tanh(projection1(.)))
    spatial, per (sample, proxy, head):  q = o;  K, V = o W + bias;  softmax over the N nodes;  o = projection2(relu(projection1(.)))
    out_i   = sum over the 2 proxies of aggregator(o) * o                             aggregator = C -> C relu C -> C sigmoid

and the layer's output is out_0 .. out_{cuts-1} along time.

The reference's quirks, restated as written:
 1. At lag 12 the first layer's cuts 2 .. 11 slice past the end of the input: they read no data row and attend over their 2 proxy rows
    alone (at lag 8, cut 1 has 2 rows).  Here that comes from the slicing, as in the reference.
 2. ``self.supports`` is built from ``adj_mx`` and read by nothing: this predictor takes no graph, and Run.py computes none for it.
 3. ``--dynamic`` is ``type=str`` (ST_WA/args.py:48): every conf value is truthy and the static ``Using FC`` branch is dead.  It is parsed
    the same way, only the dynamic model is built, and an empty value raises ``ValueError``.
 4. The noise is drawn in ``eval()`` too: the reference's test metrics are stochastic, and so are these.
 5. ``proxies``, ``mu`` and ``logvar`` are ``nn.Parameter(..).to(device)`` in the reference, a parameter on the CPU only; here they are
    parameters on every device (the difference predictors/msdr.py documents for ``nodevec*``).  The ``print('Using DYNAMIC')`` lines are
    dropped.

Same parameter tree, key for key and in the reference's order (215 keys at dim_in != 1, 213 at dim_in = 1, no buffers), and the same
consumption of the random stream by the constructor, so a seeded construction equals the reference's and its checkpoints load with
``strict=True``.

``forward(x, noise=None)``: ``noise`` = (eps_d (B, N, M), [eps_l (N, M)] * 3).  With None the four tensors are drawn with ``torch.randn`` in
the reference's order (data, then layers 0, 1, 2), in x's dtype and on x's device, before anything else runs: under one ``torch.manual_seed``
on the CPU the module sees the reference's noise.  Both backends draw this way.  ``probe``, a list, receives every cut's spatial softmax weights
(8 B, 2, N, N) and selects the torch ops: tests measure how far from uniform they are.

``STWA(..., backend="hip")`` runs the same parameters on the project's kernels wherever those serve the call (predictors/stwa_hip.py,
csrc/stwa.hip); elsewhere the forward takes the torch ops below.  ``backend_used`` records which of the two the last forward took.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _backend

HEADS = 8
LAYERS = ((12, 6), (3, 4), (1, 3))           # (cuts, cut_size) of the three Layers; 2 proxies per cut
PROXIES = 2


def reparameterize(mu, logvar, eps):
    return mu + eps * torch.exp(0.5 * logvar)


def linear_custom(x, params):
    """x (B, R, N, C) times the generated per-(sample, node) weight (B, N, C, C), plus the bias (B, N, C) (attention.py ``LinearCustom``:
    the same products, by broadcasting where the reference repeats the weight along R)"""
    w, b = params
    return torch.matmul(x.unsqueeze(-2), w.unsqueeze(1)).squeeze(-2) + b.unsqueeze(1)


def _heads(x, hs):
    return torch.cat(torch.split(x, hs, dim=-1), dim=0)


class TemporalAttention(nn.Module):
    def __init__(self, in_dim):
        super().__init__()
        if in_dim % HEADS != 0:
            raise ValueError("ST-WA: channels must be a multiple of the %d attention heads, got %r" % (HEADS, in_dim))
        self.head_size = in_dim // HEADS
        self.projection1 = nn.Linear(in_dim, in_dim)
        self.projection2 = nn.Linear(in_dim, in_dim)

    def forward(self, query, rows, parameters):
        B, hs = query.shape[0], self.head_size
        key, value = linear_custom(rows, parameters[0]), linear_custom(rows, parameters[1])
        q = _heads(query, hs).permute(0, 2, 1, 3)                          # (8 B, N, 2, hs)
        k = _heads(key, hs).permute(0, 2, 3, 1)                            # (8 B, N, hs, 2 + r)
        v = _heads(value, hs).permute(0, 2, 1, 3)
        a = F.softmax(torch.matmul(q, k) / (hs ** 0.5), dim=-1)
        o = torch.matmul(a, v).permute(0, 2, 1, 3)
        o = torch.cat(torch.split(o, B, dim=0), dim=-1)
        return self.projection2(torch.tanh(self.projection1(o)))


class SpatialAttention(nn.Module):
    def __init__(self, in_dim):
        super().__init__()
        self.head_size = in_dim // HEADS
        self.projection1 = nn.Linear(in_dim, in_dim)
        self.projection2 = nn.Linear(in_dim, in_dim)

    def weights(self, x, parameters):
        """the softmax weights (8 B, 2, N, N): what forward mixes the values by (tests measure their sharpness)"""
        hs = self.head_size
        k = _heads(linear_custom(x, parameters[0]), hs)
        return F.softmax(torch.matmul(_heads(x, hs), k.transpose(2, 3)) / (hs ** 0.5), dim=-1)

    def forward(self, x, parameters):
        B, hs = x.shape[0], self.head_size
        v = _heads(linear_custom(x, parameters[1]), hs)
        o = torch.matmul(self.weights(x, parameters), v)
        o = torch.cat(torch.split(o, B, dim=0), dim=-1)
        return self.projection2(F.relu(self.projection1(o)))


class ParameterGenerator(nn.Module):
    def __init__(self, memory_size, dim):
        super().__init__()
        self.dim = dim
        self.weight_generator = nn.Sequential(nn.Linear(memory_size, 32), nn.ReLU(), nn.Linear(32, 5), nn.ReLU(), nn.Linear(5, dim * dim))
        self.bias_generator = nn.Sequential(nn.Linear(memory_size, 32), nn.ReLU(), nn.Linear(32, 5), nn.ReLU(), nn.Linear(5, dim))

    def forward(self, z):                                                  # z (B, N, M) -> W (B, N, C, C), bias (B, N, C)
        return self.weight_generator(z).view(z.shape[0], z.shape[1], self.dim, self.dim), self.bias_generator(z)


class Layer(nn.Module):
    def __init__(self, dim, num_nodes, cuts, cut_size, memory_size):
        super().__init__()
        self.dim, self.num_nodes, self.cuts, self.cut_size = dim, num_nodes, cuts, cut_size
        self.proxies = nn.Parameter(torch.randn(1, cuts * PROXIES, num_nodes, dim))        # drawn and registered as in ST_WA.py:111-119
        self.temporal_att = TemporalAttention(dim)
        self.spatial_att = SpatialAttention(dim)
        self.mu = nn.Parameter(torch.randn(num_nodes, memory_size))
        self.logvar = nn.Parameter(torch.randn(num_nodes, memory_size))
        self.temporal_parameter_generators = nn.ModuleList([ParameterGenerator(memory_size, dim) for _ in range(2)])
        self.spatial_parameter_generators = nn.ModuleList([ParameterGenerator(memory_size, dim) for _ in range(2)])
        self.aggregator = nn.Sequential(nn.Linear(dim, dim), nn.ReLU(), nn.Linear(dim, dim), nn.Sigmoid())

    def generators(self):
        return list(self.temporal_parameter_generators) + list(self.spatial_parameter_generators)

    def forward(self, x, z_data, eps, probe=None):
        z = z_data + reparameterize(self.mu, self.logvar, eps)
        tp = [g(z) for g in self.temporal_parameter_generators]
        sp = [g(z) for g in self.spatial_parameter_generators]
        outs, out = [], 0
        for i in range(self.cuts):
            t = x[:, i * self.cut_size:(i + 1) * self.cut_size]             # r rows; r = 0 past the end of the input
            prox = self.proxies[:, i * PROXIES:(i + 1) * PROXIES] + out
            if prox.shape[0] != x.shape[0]:
                prox = prox.expand(x.shape[0], -1, -1, -1)
            o = self.temporal_att(prox, torch.cat([prox, t], dim=1), tp)
            if probe is not None:
                probe.append(self.spatial_att.weights(o, sp))
            o = self.spatial_att(o, sp)
            out = (self.aggregator(o) * o).sum(1, keepdim=True)
            outs.append(out)
        return torch.cat(outs, dim=1)


class STWA(nn.Module):
    """``args_predictor``: num_nodes, lag, horizon, out_dim, channels, dynamic (a string, as the reference parses it), memory_size — the
    fields of reference ST_WA/args.py:41-49; no graph.

    As with the other predictors the two backends differ in one observable way: in eval mode the HIP path runs under ``no_grad`` and keeps
    nothing for a backward.  Gradients through ``backend="hip"`` need ``train()`` mode."""

    def __init__(self, args_predictor, device, dim_in, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("STWA", backend), None
        a = args_predictor
        if not a.dynamic:
            raise ValueError("ST-WA: --dynamic is a string in the reference and every conf value is truthy; only the dynamic model is "
                             "built, got an empty value")
        self.num_nodes, self.input_dim, self.output_dim, self.channels = a.num_nodes, dim_in, a.out_dim, a.channels
        self.horizon, self.lag, self.memory_size = a.horizon, a.lag, a.memory_size
        C, M = a.channels, a.memory_size
        self.start_fc = nn.Linear(dim_in, C)
        if dim_in != 1:
            self.eval_dimin = nn.Linear(dim_in, 1)
        self.layers = nn.ModuleList([Layer(C, a.num_nodes, cuts, cs, M) for cuts, cs in LAYERS])
        self.skip_layers = nn.ModuleList([nn.Linear(cuts * C, 256) for cuts, _ in LAYERS])
        self.projections = nn.Sequential(nn.Linear(256, 512), nn.ReLU(), nn.Linear(512, a.horizon * a.out_dim))
        self.mu_estimator = nn.Sequential(nn.Linear(a.lag, 32), nn.Tanh(), nn.Linear(32, 32), nn.Tanh(), nn.Linear(32, M))
        self.logvar_estimator = nn.Sequential(nn.Linear(a.lag, 32), nn.Tanh(), nn.Linear(32, 32), nn.Tanh(), nn.Linear(32, M))
        self.to(device)

    def draw_noise(self, x):
        """(eps_d (B, N, M), [eps_l (N, M)] * 3) in the reference's order of draws"""
        kw = dict(dtype=x.dtype, device=x.device)
        eps_d = torch.randn(x.shape[0], self.num_nodes, self.memory_size, **kw)
        return eps_d, [torch.randn(self.num_nodes, self.memory_size, **kw) for _ in self.layers]

    def z_data(self, x, eps_d):
        xd = self.eval_dimin(x) if x.shape[-1] != 1 else x
        xd = xd.transpose(3, 1).squeeze(1)                                  # (B, N, lag)
        return reparameterize(self.mu_estimator(xd), self.logvar_estimator(xd), eps_d)

    def head(self, skip, B):
        out = self.projections(torch.relu(skip))
        if self.output_dim == 1:
            return out.transpose(2, 1).unsqueeze(-1)
        return out.unsqueeze(-1).reshape(B, self.num_nodes, self.horizon, -1).transpose(2, 1)

    def forward(self, x, noise=None, probe=None):                          # x (B, lag, N, dim_in)
        if noise is None:
            noise = self.draw_noise(x)
        if probe is None:                                                  # (a probe asks for the softmax weights, which only the torch ops form)
            y = _backend.hip_forward(self, "stwa_hip", x, noise=noise)
            if y is not None:
                return y
        else:
            self.backend_used = "torch"
        eps_d, eps_l = noise
        B = x.shape[0]
        z_data = self.z_data(x, eps_d)
        h = self.start_fc(x)
        skip = 0
        for layer, skip_layer, eps in zip(self.layers, self.skip_layers, eps_l):
            h = layer(h, z_data, eps, probe)
            skip = skip + skip_layer(h.transpose(2, 1).reshape(B, self.num_nodes, -1))
        return self.head(skip, B)
