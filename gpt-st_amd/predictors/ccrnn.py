"""CCRNN predictor (Ye et al., "Coupled Layer-wise Graph Convolution for Transportation Demand Prediction", AAAI 2021) as the reference wires
it behind the enhanced embedding: ``-mode eval -model CCRNN`` (reference model/CCRNN_demand/CCRNN.py ``EvoNN2``, ``DCRNNEncoder``,
``DCRNNDecoder``, ``DCGRUCell``, ``EvolutionCell``, ``GraphConv_``).  x (B, T, N, dim_in) -> (B, num_predict, N, dim_out).

    graph0 = leaky_relu(nodevec1 nodevec2);  graph1, graph2 from the node vectors sent through (w1, b1) and then (w2, b2): NOT normalised
    a cell:  [r, u] = sigmoid(conv_ru([x, h]));  c = tanh(conv_c([x, r h]));  h' = u h + (1 - u) c
    conv:    layer i = Linear over [T_0 .. T_k](graph i) z (Chebyshev recursion on ONE support, columns channel-major, matrix-minor:
             c * num_matrices + m), layer i + 1 reads layer i's output; the layers' outputs are mixed by a softmax over ``attlinear``
    encoder: the cells of layer l over all T steps, layer l + 1 reads layer l's outputs; zero initial states
    decoder: starts from a zero input and the encoder's last states; its input at step t + 1 is out(h_t), or targets[:, t] when targets are
             given and ``random.random() < teacher_force`` (Python's ``random``: one draw per step, none without targets)

Restated with the SAME parameter tree, key for key and in the reference's order (24 keys at one RNN layer and one graph-conv layer, 40 at two
RNN layers or at three graph-conv layers).  Kept as the reference has them:
  * graph-conv layer i reads graph i only, so with one layer ``w1, w2, b1, b2`` take no gradient (``.grad`` stays None) and every
    ``attlinear`` takes an exactly zero one (the softmax runs over one entry);
  * more than three graph-conv layers have no graph to read (an IndexError in the reference): refused at construction;
  * ``k_hop = 0`` is served (the Linear reads z alone);
  * the reference's Model.py hands ``batch_seen = None`` always, so the threshold is the constant 0.5; ``_compute_sampling_threshold`` serves a
    caller that passes ``batch_seen``.
``nodevec1, nodevec2`` come from ``torch.svd(support)`` truncated to ``n_dim``; ``n_dim > N`` cannot build a model (``w1 = eye(n_dim)`` meets
node vectors of N columns) and raises.

``CCRNN(..., backend="hip")`` runs the same parameters on the project's kernels wherever those serve the call (predictors/ccrnn_hip.py,
csrc/ccrnn.hip); elsewhere the forward takes the torch ops below.  ``backend_used`` records which of the two the last forward took.
"""
import math
import random

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _backend


class GraphConv(nn.Module):
    """Linear([T_0(S) z | .. | T_k(S) z]) per support, columns c * num_matrices + m"""

    def __init__(self, input_dim, output_dim, num_nodes, n_supports, max_step):
        super().__init__()
        self._num_nodes, self._max_diffusion_step = num_nodes, max_step
        self.out = nn.Linear(input_dim * (max_step * n_supports + 1), output_dim)

    def forward(self, inputs, supports):
        b, n, input_dim = inputs.shape
        x0 = inputs.permute(1, 2, 0).reshape(n, -1)                          # (N, input_dim * B)
        xs = [x0]
        if self._max_diffusion_step > 0:
            for support in supports:
                x1 = support.mm(x0)
                xs.append(x1)
                for _ in range(2, self._max_diffusion_step + 1):
                    x2 = 2 * support.mm(x1) - x0
                    xs.append(x2)
                    x1, x0 = x2, x1                                        # (carried over to the next support, as the reference does)
        x = torch.stack(xs, 0).reshape(-1, n, input_dim, b).transpose(0, 3)  # (B, N, input_dim, num_matrices)
        return self.out(x.reshape(b, n, -1))


class EvolutionCell(nn.Module):
    def __init__(self, input_dim, output_dim, num_nodes, n_supports, max_step, layer):
        super().__init__()
        self.layer = layer
        self.graphconv = nn.ModuleList()                                     # registered first, drawn second: the reference's key and draw orders
        self.attlinear = nn.Linear(num_nodes * output_dim, 1)
        self.graphconv.append(GraphConv(input_dim, output_dim, num_nodes, n_supports, max_step))
        for _ in range(1, layer):
            self.graphconv.append(GraphConv(output_dim, output_dim, num_nodes, n_supports, max_step))

    def forward(self, inputs, supports):
        outputs = []
        for i in range(self.layer):
            inputs = self.graphconv[i](inputs, [supports[i]])
            outputs.append(inputs)
        return self.attention(torch.stack(outputs, dim=1))

    def attention(self, inputs):
        b, g, n, f = inputs.shape
        x = inputs.reshape(b, g, -1)
        weight = F.softmax(self.attlinear(x), dim=1)                         # (B, g, 1)
        return (x * weight).sum(dim=1).reshape(b, n, f)


class DCGRUCell(nn.Module):
    def __init__(self, input_size, hidden_size, num_node, n_supports, k_hop, e_layer):
        super().__init__()
        self.hidden_size = hidden_size
        self.ru_gate_g_conv = EvolutionCell(input_size + hidden_size, hidden_size * 2, num_node, n_supports, k_hop, e_layer)
        self.candidate_g_conv = EvolutionCell(input_size + hidden_size, hidden_size, num_node, n_supports, k_hop, e_layer)

    def forward(self, inputs, supports, states):
        r_u = torch.sigmoid(self.ru_gate_g_conv(torch.cat([inputs, states], -1), supports))
        r, u = r_u.split(self.hidden_size, -1)
        c = torch.tanh(self.candidate_g_conv(torch.cat([inputs, r * states], -1), supports))
        return u * states + (1 - u) * c


class Encoder(nn.ModuleList):
    def __init__(self, input_size, hidden_size, num_node, n_supports, k_hop, n_layers, e_layer):
        super().__init__()
        self.hidden_size = hidden_size
        self.append(DCGRUCell(input_size, hidden_size, num_node, n_supports, k_hop, e_layer))
        for _ in range(1, n_layers):
            self.append(DCGRUCell(hidden_size, hidden_size, num_node, n_supports, k_hop, e_layer))

    def forward(self, inputs, supports):
        """inputs (B, T, N, input_size) -> the layers' last states (n_layers, B, N, hidden_size)"""
        b, t, n, _ = inputs.shape
        states = list(inputs.new_zeros(len(self), b, n, self.hidden_size))
        inputs = list(inputs.transpose(0, 1))
        for i_layer, cell in enumerate(self):
            for i_t in range(t):
                inputs[i_t] = states[i_layer] = cell(inputs[i_t], supports, states[i_layer])
        return torch.stack(states)


class Decoder(nn.ModuleList):
    def __init__(self, output_size, hidden_size, num_node, n_supports, k_hop, n_layers, n_preds, e_layer):
        super().__init__()
        self.output_size, self.n_preds = output_size, n_preds
        self.append(DCGRUCell(output_size, hidden_size, num_node, n_supports, k_hop, e_layer))
        for _ in range(1, n_layers):
            self.append(DCGRUCell(hidden_size, hidden_size, num_node, n_supports, k_hop, e_layer))
        self.out = nn.Linear(hidden_size, output_size)

    def draw(self, targets, teacher_force=0.5):
        """the teacher-forcing decision of every step, drawn in the reference's order: one ``random.random()`` per step, and only with targets"""
        return [targets is not None and random.random() < teacher_force for _ in range(self.n_preds)]

    def forward(self, supports, states, targets=None, teacher_force=0.5, forced=None):
        """states (n_layers, B, N, hidden_size) -> (B, n_preds, N, output_size).  ``forced``: the decisions already drawn (``draw``)"""
        n_layers, b, n, _ = states.shape
        forced = self.draw(targets, teacher_force) if forced is None else forced
        inputs = states.new_zeros(b, n, self.output_size)
        states = list(states)
        outputs = []
        for i_t in range(self.n_preds):
            for i_layer in range(n_layers):
                inputs = states[i_layer] = self[i_layer](inputs, supports, states[i_layer])
            inputs = self.out(inputs)
            outputs.append(inputs)
            if forced[i_t]:
                inputs = targets[:, i_t]
        return torch.stack(outputs, 1)


class CCRNN(nn.Module):
    """``args_predictor``: num_predict, hidden_size, num_nodes, n_dim, n_supports, k_hop, n_rnn_layers, n_gconv_layers, cl_decay_steps and
    support (N, N) = graph.ccrnn_support(...) — the fields of reference CCRNN_demand/args.py:79-121.

    ``forward(x, targets=None, batch_seen=None)``; ``takes_targets`` tells the front end to hand the labels over (reference Model.py:110-114).
    As with the other predictors, in eval mode the HIP path runs under ``no_grad`` and keeps nothing for a backward."""

    takes_targets = True

    def __init__(self, args_predictor, device, dim_in, dim_out, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("CCRNN", backend), None
        a = args_predictor
        self.num_nodes, self.n_dim, self.hidden_size, self.n_supports, self.k_hop = a.num_nodes, a.n_dim, a.hidden_size, a.n_supports, a.k_hop
        self.n_rnn_layers, self.n_gconv_layers, self.num_predict, self.cl_decay_steps = a.n_rnn_layers, a.n_gconv_layers, a.num_predict, a.cl_decay_steps
        self.input_dim, self.output_dim = dim_in, dim_out
        support = torch.as_tensor(a.support, dtype=torch.float32)
        if support.dim() != 2 or tuple(support.shape) != (a.num_nodes, a.num_nodes):
            raise ValueError("CCRNN support must be (N, N) with N = %d, got %r" % (a.num_nodes, tuple(support.shape)))
        if a.n_dim > a.num_nodes:
            raise ValueError("CCRNN n_dim = %d exceeds num_nodes = %d: the SVD of the support has only N singular vectors, and w1 = eye(n_dim) "
                             "cannot multiply node vectors of N columns" % (a.n_dim, a.num_nodes))
        if not 1 <= a.n_gconv_layers <= 3:
            raise ValueError("CCRNN n_gconv_layers must be 1, 2 or 3 (graph-conv layer i reads graph i of three), got %r" % (a.n_gconv_layers,))
        m, p, n = torch.svd(support.to(device))
        self.nodevec1 = nn.Parameter(torch.mm(m[:, :a.n_dim], torch.diag(p[:a.n_dim] ** 0.5)))
        self.nodevec2 = nn.Parameter(torch.mm(torch.diag(p[:a.n_dim] ** 0.5), n[:, :a.n_dim].t()))
        self.encoder = Encoder(dim_in, a.hidden_size, a.num_nodes, a.n_supports, a.k_hop, a.n_rnn_layers, a.n_gconv_layers)
        self.decoder = Decoder(dim_out, a.hidden_size, a.num_nodes, a.n_supports, a.k_hop, a.n_rnn_layers, a.num_predict, a.n_gconv_layers)
        self.w1 = nn.Parameter(torch.eye(a.n_dim))
        self.w2 = nn.Parameter(torch.eye(a.n_dim))
        self.b1 = nn.Parameter(torch.zeros(a.n_dim))
        self.b2 = nn.Parameter(torch.zeros(a.n_dim))
        self.to(device)

    def graphs(self):
        """[graph0, graph1, graph2]: not normalised"""
        v1, v2 = self.nodevec1, self.nodevec2
        out = [F.leaky_relu(torch.mm(v1, v2))]
        for w, b in ((self.w1, self.b1), (self.w2, self.b2)):
            v1 = v1.mm(w) + b
            v2 = (v2.t().mm(w) + b).t()
            out.append(F.leaky_relu(torch.mm(v1, v2)))
        return out

    def _compute_sampling_threshold(self, batches_seen):
        return self.cl_decay_steps / (self.cl_decay_steps + math.exp(batches_seen / self.cl_decay_steps))

    def forward(self, x, targets=None, batch_seen=None):                   # x (B, T, N, dim_in)
        teacher_force = 0.5 if batch_seen is None else self._compute_sampling_threshold(batch_seen)
        forced = self.decoder.draw(targets, teacher_force)                 # before anything else: both backends consume the same draws
        y = _backend.hip_forward(self, "ccrnn_hip", x, targets=targets, forced=forced)
        if y is not None:
            return y
        graph = self.graphs()
        return self.decoder(graph, self.encoder(x, graph), targets, forced=forced)
