"""STGODE predictor (Fang et al., KDD 2021) as the reference wires it behind the enhanced embedding: ``-mode eval -model STGODE``
(reference model/STGODE/STGODE.py ``ODEGCN``, odegcn.py).  Restated with the SAME parameter tree, key for key and in the same order —
``sp_blocks.L.{0,1}`` and ``se_blocks.L.{0,1}``, each with ``temporal1`` / ``odeg.odeblock.odefunc`` / ``temporal2`` / ``batch_norm``, and
``pred.0`` / ``pred.2`` — so a reference checkpoint loads with ``load_state_dict``, and the same arithmetic.  Rows (b, t, n), channels last: the
input is (B, T, N, C) as the enhanced embedding arrives; the reference transposes to (B, N, T, C), this file never does.

    block       BN_nodes(relu(temporal2(relu(odeg(temporal1(X))))))
    temporal    the reference's ``F.relu(self.network(y) + self.downsample(y) if self.downsample else y)`` parses as
                ``relu(network(y) + downsample(y)) if downsample else relu(y)``: with ``num_inputs == num_channels[-1]`` (every TCN of the model
                at the confs' sizes: dim_in = 64 = out_channels[-1]) the block is relu(y) and its convolutions NEVER run.  They are built
                all the same — the keys (with the ``conv`` alias of the last level, as the reference's attribute leaves it), the seeded draws
                and the order are the reference's — and their ``.grad`` stays None.  With a downsample the convolutions do run (torch only).
    odeg        ``odeint(f, x, [0, 6], method='euler')[1]`` is ONE Euler step on a two-point grid, z = x + 6 f(0, x), then relu, with
                    f = alpha_n / 2 (A x) + x W + (x along time) W2 - 3 x + x0,     W = (w clamp(d, 0, 1)) w^T,   W2 = (w2 clamp(d2, 0, 1)) w2^T
                alpha = sigmoid(alpha) per OUTPUT node.  x0 is ``x.clone().detach()``: the value is 3 alpha A x + 6 x W + 6 x W2 - 11 x, the
                gradient that of ... - 17 x.  torchdiffeq is not needed: the step is written out (``ode_step``).
    batch norm  ``BatchNorm2d(num_nodes)`` on the reference's (B, N, T, C): the channel is the NODE, statistics over (b, t, c)
    model       n_layers sequences of two blocks on the spatial graph and as many on the semantic (DTW) graph, all fed the same input; the
                element-wise max over the 2 n_layers outputs (``torch.max``: exact ties go to the lowest index); the heads
                Linear(T C -> P out_channels[1]), relu, Linear(-> P dim_out) over rows (b, n)

The two graphs (``graph.stgode_graphs``) are buffers outside the state dict.  ``STGODE(..., backend="hip")`` runs the same parameter tree on the
project's kernels wherever those serve the call (predictors/stgode_hip.py); elsewhere the forward takes the torch modules.  ``backend_used``
records which of the two the last forward took.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _backend

ODE_TIME = 6.0            # reference STGODE.py:98 ``ODEG(..., time=6)``: the length of the one Euler step


class Chomp1d(nn.Module):
    """drops the ``chomp_size`` steps the padding of a causal convolution added at the end"""

    def __init__(self, chomp_size):
        super().__init__()
        self.chomp_size = chomp_size

    def forward(self, x):
        return x[:, :, :, :-self.chomp_size].contiguous()


class TemporalConvNet(nn.Module):
    def __init__(self, num_inputs, num_channels, kernel_size=2, dropout=0.2):
        super().__init__()
        layers = []
        for i, co in enumerate(num_channels):
            dil = 2 ** i
            ci = num_inputs if i == 0 else num_channels[i - 1]
            pad = (kernel_size - 1) * dil
            self.conv = nn.Conv2d(ci, co, (1, kernel_size), dilation=(1, dil), padding=(0, pad))     # (the attribute keeps the last level: a key)
            self.conv.weight.data.normal_(0, 0.01)
            self.chomp, self.relu, self.dropout = Chomp1d(pad), nn.ReLU(), nn.Dropout(dropout)
            layers.append(nn.Sequential(self.conv, self.chomp, self.relu, self.dropout))
        self.network = nn.Sequential(*layers)
        self.downsample = nn.Conv2d(num_inputs, num_channels[-1], (1, 1)) if num_inputs != num_channels[-1] else None
        if self.downsample is not None:
            self.downsample.weight.data.normal_(0, 0.01)

    def forward(self, x):                                                  # x (B, T, N, C)
        if self.downsample is None:
            return torch.relu(x)                                           # the reference's precedence: the convolutions are never reached
        y = x.permute(0, 3, 2, 1)                                          # (B, C, N, T)
        return torch.relu(self.network(y) + self.downsample(y)).permute(0, 3, 2, 1)


class ODEFunc(nn.Module):
    def __init__(self, feature_dim, temporal_dim, num_nodes):
        super().__init__()
        self.alpha = nn.Parameter(0.8 * torch.ones(num_nodes))
        self.w = nn.Parameter(torch.eye(feature_dim))
        self.d = nn.Parameter(torch.zeros(feature_dim) + 1)
        self.w2 = nn.Parameter(torch.eye(temporal_dim))
        self.d2 = nn.Parameter(torch.zeros(temporal_dim) + 1)

    def mats(self):
        """(sigmoid(alpha) (N), W (C, C), W2 (T, T)): the small-parameter chains, torch's on either backend"""
        return (torch.sigmoid(self.alpha), torch.mm(self.w * torch.clamp(self.d, min=0, max=1), self.w.t()),
                torch.mm(self.w2 * torch.clamp(self.d2, min=0, max=1), self.w2.t()))

    def forward(self, x, x0, adj):                                         # x (B, T, N, C)
        alpha, w, w2 = self.mats()
        xa = torch.einsum("ij,btjc->btic", adj, x)
        xw = torch.einsum("btnc,cm->btnm", x, w)
        xw2 = torch.einsum("bknc,km->bmnc", x, w2)
        return alpha[:, None] / 2 * xa - x + xw - x + xw2 - x + x0


class ODEblock(nn.Module):
    def __init__(self, odefunc):
        super().__init__()
        self.odefunc = odefunc


class ODEG(nn.Module):
    def __init__(self, feature_dim, temporal_dim, num_nodes):
        super().__init__()
        self.odeblock = ODEblock(ODEFunc(feature_dim, temporal_dim, num_nodes))

    def forward(self, x, adj):
        return torch.relu(x + ODE_TIME * self.odeblock.odefunc(x, x.detach(), adj))


class STGCNBlock(nn.Module):
    def __init__(self, time_steps, in_channels, out_channels, num_nodes):
        super().__init__()
        self.temporal1 = TemporalConvNet(in_channels, out_channels)
        self.odeg = ODEG(out_channels[-1], time_steps, num_nodes)
        self.temporal2 = TemporalConvNet(out_channels[-1], out_channels)
        self.batch_norm = nn.BatchNorm2d(num_nodes)

    def identity_form(self):
        """both temporal nets are relu alone: what the HIP backend serves"""
        return self.temporal1.downsample is None and self.temporal2.downsample is None

    def forward(self, x, adj):                                             # x (B, T, N, C)
        t = self.temporal2(torch.relu(self.odeg(self.temporal1(x), adj)))
        return self.batch_norm(t.transpose(1, 2)).transpose(1, 2)          # the node as the channel


class STGODE(nn.Module):
    """``args``: num_nodes, num_timesteps_input, num_timesteps_output, in_channels, out_channels, n_layers, and the two normalised graphs
    A_sp_wave and A_se_wave (N, N) — the fields of reference STGODE.py:131-152.

    Takes (B, num_timesteps_input, N, dim_in), returns (B, num_timesteps_output, N, dim_out)."""

    def __init__(self, args, device, dim_in, dim_out, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("STGODE", backend), None
        a = args
        oc = list(a.out_channels)
        self.num_nodes, self.window, self.horizon, self.dim_out, self.n_layers = a.num_nodes, a.num_timesteps_input, a.num_timesteps_output, dim_out, a.n_layers
        self.out_channels = oc
        for name, g in (("A_sp", a.A_sp_wave), ("A_se", a.A_se_wave)):
            g = torch.as_tensor(g, dtype=torch.float32)
            if tuple(g.shape) != (a.num_nodes, a.num_nodes):
                raise ValueError("STGODE %s must be (N, N) = %d squared, got %r" % (name, a.num_nodes, tuple(g.shape)))
            self.register_buffer(name, g.clone(), persistent=False)

        def branch():
            return nn.Sequential(STGCNBlock(a.num_timesteps_input, dim_in, oc, a.num_nodes),
                                 STGCNBlock(a.num_timesteps_input, a.in_channels, oc, a.num_nodes))
        self.sp_blocks = nn.ModuleList([branch() for _ in range(a.n_layers)])
        self.se_blocks = nn.ModuleList([branch() for _ in range(a.n_layers)])
        self.pred = nn.Sequential(nn.Linear(a.num_timesteps_input * oc[2], a.num_timesteps_output * oc[1]), nn.ReLU(),
                                  nn.Linear(a.num_timesteps_output * oc[1], a.num_timesteps_output * dim_out))
        self.to(device)

    def branches(self):
        """[(sequence of blocks, its graph)]: the spatial ones, then the semantic ones — the order of the max"""
        return [(seq, self.A_sp) for seq in self.sp_blocks] + [(seq, self.A_se) for seq in self.se_blocks]

    def head(self, h):
        """h (B, T, N, C) -> (B, horizon, N, dim_out): the two linears over rows (b, n) with (t, c) flattened"""
        b, _, n, _ = h.shape
        return self.pred(h.transpose(1, 2).reshape(b, n, -1)).reshape(b, n, self.horizon, self.dim_out).transpose(1, 2)

    def forward(self, x):                                                  # x (B, T, N, dim_in)
        y = _backend.hip_forward(self, "stgode_hip", x)
        if y is not None:
            return y
        outs = []
        for seq, adj in self.branches():
            h = x
            for blk in seq:
                h = blk(h, adj)
            outs.append(h)
        return self.head(torch.max(torch.stack(outs), dim=0)[0])
