"""MSDR predictor (Liu et al., "MSDR: Multi-Step Dependency Relation Networks", KDD 2022) as the reference wires it behind the enhanced
embedding: ``-mode eval -model MSDR`` (reference model/MSDR/gmsdr_model.py ``GMSDRModel``, gmsdr_cell.py ``GMSDRCell``, built in
model/Model.py:79-82).  A sequence-to-sequence stack of cells that each keep their last ``pre_k`` outputs S = (s_1 .. s_K), oldest first:

    h   = [s_K | s_{K-1} | ..]  (pre_v of them)                 Z = [u | h]
    A   = softmax_rows(relu(nodevec1 nodevec2))                  the cell's own adaptive graph
    G   = [Z, L~ Z, .., A Z]                                     Chebyshev terms of every fixed support, then of A (gmsdr_cell.py:137-170)
    c   = leaky_relu(G Theta + beta)                             Theta row = channel * matrices + matrix
    a   = softmax_k(attlinear(vec(s_k + R_k)))                   one logit per kept state
    o   = c W + b + sum_k a_k (s_k + R_k)                        S <- (s_2 .. s_K, o); the cell's output is o

The encoder (``mlp`` then the layers, S = 0 at t = 0) runs over the T input steps; decoder layer l starts from the encoder's final S of layer
l, and — the decoder is NOT autoregressive — decoder step t reads the encoder's top-layer output of step t; y_t = projection_layer(o_top).

Restated with the SAME parameter tree, key for key and in the reference's order AFTER its first forward (42 keys at two layers): the
reference creates Theta and beta (``gconv_weight_(rows, d)``, ``gconv_biases_d``) inside the first forward, here they are registered by the
constructor and drawn last, in the order that forward creates them (encoder layers, then decoder layers), so a seeded construction equals
the reference's seeded construction plus one forward, and a reference checkpoint saved after training loads with ``strict=True``.
Deliberate differences: Theta and beta are ordinary trained parameters (the reference builds its optimizer before they exist and never
trains them); ``nodevec1`` / ``nodevec2`` are parameters on every device (the reference's ``nn.Parameter(..).to(device)`` is one on the
CPU only); the supports are dense non-persistent buffers (``graph.msdr_supports``); ``out`` is kept as the dead Linear it is.

``MSDR(..., backend="hip")`` runs the same parameters on the project's kernels wherever those serve the call (predictors/msdr_hip.py,
csrc/msdr.hip); elsewhere the forward takes the torch ops below.  ``backend_used`` records which of the two the last forward took.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _backend


class GMSDRCell(nn.Module):
    def __init__(self, num_units, supports, max_diffusion_step, num_nodes, pre_k, pre_v):
        super().__init__()
        self.num_units, self.num_nodes, self.max_diffusion_step, self.pre_k, self.pre_v = num_units, num_nodes, max_diffusion_step, pre_k, pre_v
        self.register_buffer("supports", supports.clone(), persistent=False)     # (S, N, N) dense; the reference keeps sparse plain attributes
        self.nodevec1 = nn.Parameter(torch.randn(num_nodes, 10))           # the random stream is consumed as in gmsdr_cell.py:77-78,98
        self.nodevec2 = nn.Parameter(torch.randn(10, num_nodes))
        self.W = nn.Parameter(torch.zeros(num_units, num_units))
        self.b = nn.Parameter(torch.zeros(num_nodes, num_units))
        self.R = nn.Parameter(torch.zeros(pre_k, num_nodes, num_units))
        self.input_size = num_units * (1 + pre_v)                          # every cell's input is d wide: the encoder's mlp comes first
        self.num_matrices = (supports.shape[0] + 1) * max_diffusion_step + 1
        shape = (self.input_size * self.num_matrices, num_units)
        self.theta_name, self.beta_name = "gconv_weight_%s" % (shape,), "gconv_biases_%d" % num_units
        self.register_parameter(self.theta_name, nn.Parameter(torch.empty(*shape)))      # drawn by MSDR.__init__, after everything else
        self.register_parameter(self.beta_name, nn.Parameter(torch.empty(num_units)))
        self.attlinear = nn.Linear(num_nodes * num_units, 1)

    @property
    def theta(self):
        return getattr(self, self.theta_name)

    @property
    def beta(self):
        return getattr(self, self.beta_name)

    def adaptive(self):
        return F.softmax(F.relu(torch.mm(self.nodevec1, self.nodevec2)), dim=1)

    def gconv(self, z):
        """z (B, N, F) -> (B, N, d): the reference's recurrences as written, the swap of x0 / x1 it leaves behind included"""
        x0, xs = z, [z]
        if self.max_diffusion_step > 0:
            for k in range(self.supports.shape[0]):
                x1 = torch.matmul(self.supports[k], x0)
                xs.append(x1)
                for _ in range(2, self.max_diffusion_step + 1):
                    x2 = 2 * torch.matmul(self.supports[k], x1) - x0
                    xs.append(x2)
                    x1, x0 = x2, x1
        adp = self.adaptive()
        x1 = torch.matmul(adp, x0)
        xs.append(x1)
        for _ in range(2, self.max_diffusion_step + 1):
            x2 = torch.matmul(adp, x1) - x0
            xs.append(x2)
            x1, x0 = x2, x1
        g = torch.stack(xs, dim=-1)                                        # (B, N, F, matrices): column = channel * matrices + matrix
        return torch.matmul(g.reshape(z.shape[0], self.num_nodes, -1), self.theta) + self.beta

    def forward(self, u, S):
        """u (B, N, d), S (B, K, N, d) -> (o (B, N, d), the new S)"""
        h = torch.cat([S[:, S.shape[1] - 1 - i] for i in range(self.pre_v)], dim=-1)
        c = F.leaky_relu(self.gconv(torch.cat([u, h], dim=-1)))
        xs = S + self.R.unsqueeze(0)
        a = F.softmax(self.attlinear(xs.reshape(xs.shape[0], xs.shape[1], -1)), dim=1)     # (B, K, 1)
        o = torch.matmul(c, self.W) + self.b.unsqueeze(0) + (xs * a.unsqueeze(-1)).sum(dim=1)
        return o, torch.cat([S[:, 1:], o.unsqueeze(1)], dim=1)


class _Encoder(nn.Module):
    def __init__(self, dim_in, cell, layers):
        super().__init__()
        self.mlp = nn.Linear(dim_in, cell[0])
        self.gmsdr_layers = nn.ModuleList([GMSDRCell(*cell) for _ in range(layers)])


class _Decoder(nn.Module):
    def __init__(self, output_dim, cell, layers):
        super().__init__()
        self.projection_layer = nn.Linear(cell[0], output_dim)
        self.gmsdr_layers = nn.ModuleList([GMSDRCell(*cell) for _ in range(layers)])


class MSDR(nn.Module):
    """``args_predictor``: num_nodes, seq_len, horizon, rnn_units, num_rnn_layers, pre_k, pre_v, max_diffusion_step, output_dim, and the
    supports (S, N, N) = graph.msdr_supports(adjacency, filter_type) — the fields of reference MSDR/args.py:90-109 with the graph already
    normalised (the reference normalises ``adj_mx`` inside every cell).

    As with the other predictors the two backends differ in one observable way: in eval mode the HIP path runs under ``no_grad`` and keeps
    nothing for a backward.  Gradients through ``backend="hip"`` need ``train()`` mode."""

    def __init__(self, args_predictor, device, dim_in, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("MSDR", backend), None
        a = args_predictor
        self.num_nodes, self.input_dim, self.output_dim, self.rnn_units = a.num_nodes, dim_in, a.output_dim, a.rnn_units
        self.seq_len, self.horizon, self.num_rnn_layers, self.pre_k, self.pre_v = a.seq_len, a.horizon, a.num_rnn_layers, a.pre_k, a.pre_v
        self.max_diffusion_step = a.max_diffusion_step
        if not 1 <= a.pre_v <= a.pre_k or a.horizon > a.seq_len:
            raise ValueError("MSDR needs 1 <= pre_v <= pre_k and horizon <= seq_len (decoder step t reads the encoder's output of step t), got "
                             "pre_v %r, pre_k %r, horizon %r, seq_len %r" % (a.pre_v, a.pre_k, a.horizon, a.seq_len))
        sup = torch.as_tensor(a.supports, dtype=torch.float32)
        if sup.dim() != 3 or tuple(sup.shape[1:]) != (a.num_nodes, a.num_nodes):
            raise ValueError("MSDR supports must be (S, N, N) with N = %d, got %r" % (a.num_nodes, tuple(sup.shape)))
        cell = (a.rnn_units, sup, a.max_diffusion_step, a.num_nodes, a.pre_k, a.pre_v)
        self.encoder_model = _Encoder(dim_in, cell, a.num_rnn_layers)
        self.decoder_model = _Decoder(a.output_dim, cell, a.num_rnn_layers)
        self.out = nn.Linear(a.rnn_units, a.output_dim)                    # gmsdr_model.py:105: built, in the state dict, read by nothing
        for c in self.cells():                                             # what the reference's first forward creates, in its order
            nn.init.xavier_normal_(c.theta)
            nn.init.constant_(c.beta, 1.0)
        self.to(device)

    def cells(self):
        return list(self.encoder_model.gmsdr_layers) + list(self.decoder_model.gmsdr_layers)

    def forward(self, x):                                                  # x (B, T, N, dim_in)
        y = _backend.hip_forward(self, "msdr_hip", x)
        if y is not None:
            return y
        B, N, d = x.shape[0], self.num_nodes, self.rnn_units
        S = [x.new_zeros(B, self.pre_k, N, d) for _ in range(self.num_rnn_layers)]
        tops = []
        for t in range(self.seq_len):
            o = self.encoder_model.mlp(x[:, t])
            for l, cell in enumerate(self.encoder_model.gmsdr_layers):
                o, S[l] = cell(o, S[l])
            tops.append(o)
        ys = []
        for t in range(self.horizon):
            o = tops[t]
            for l, cell in enumerate(self.decoder_model.gmsdr_layers):
                o, S[l] = cell(o, S[l])
            ys.append(self.decoder_model.projection_layer(o))
        return torch.stack(ys, dim=1)                                      # (B, horizon, N, output_dim)
