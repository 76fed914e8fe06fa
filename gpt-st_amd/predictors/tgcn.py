"""TGCN predictor (Zhao et al., T-ITS 2019) as the reference wires it behind the enhanced embedding: ``-mode eval -model TGCN``
(reference model/TGCN/TGCN.py:28-175, constructed in model/Model.py:67-69).  A GRU over the T input steps whose two gate transforms are
graph convolutions with the normalised adjacency L (gptst_amd.graph.tgcn_graph), then one Linear from the last state to the whole forecast:

    [r, u] = sigmoid(L [x_t, h] W0 + b0)         c = tanh(L [x_t, r * h] W1 + b1)         h <- u * h + (1 - u) * c          h_0 = 0
    y = Linear(h_T) viewed as (B, N, W, output_dim) -> (B, W, N, output_dim)

Restated with the SAME parameter tree (``tgcn_model.weights_0 / weights_1 / bias_0 / bias_1``, ``output_model.weight / bias``; L is a dense
non-persistent buffer where the reference keeps a sparse attribute), so a reference checkpoint loads with ``load_state_dict(strict=True)``,
and the same initialisation order, so a seeded construction equals the reference's.

The torch ops below are the default.  ``TGCN(..., backend="hip")`` runs the same parameters on the project's own kernels
(predictors/tgcn_hip.py, csrc/tgcn.hip) wherever those serve the call; elsewhere (a CPU input, an unsupported width) the forward takes the
torch ops.  ``backend_used`` records which of the two the last forward took.
"""
import torch
import torch.nn as nn

from . import _backend


class _Cell(nn.Module):
    """the parameter holder ``tgcn_model``: W0 (C + H, 2 H), b0 (2 H), W1 (C + H, H), b1 (H), registered in the reference's order (TGCN.py:41-56)"""

    def __init__(self, num_units, lap, input_dim):
        super().__init__()
        self.num_units, self.input_dim = num_units, input_dim
        self.register_buffer("L", lap, persistent=False)                 # (N, N) dense; the reference keeps a sparse plain attribute
        w0, b0 = torch.empty(input_dim + num_units, 2 * num_units), torch.empty(2 * num_units)
        w1, b1 = torch.empty(input_dim + num_units, num_units), torch.empty(num_units)
        nn.init.xavier_normal_(w0)                                         # the random stream is consumed as in TGCN.py:48-51
        nn.init.xavier_normal_(w1)
        nn.init.constant_(b0, 0.0)                                         # (the reference passes bias_start=1.0 to _gc and never uses it)
        nn.init.constant_(b1, 0.0)
        self.weights_0, self.weights_1 = nn.Parameter(w0), nn.Parameter(w1)
        self.bias_0, self.bias_1 = nn.Parameter(b0), nn.Parameter(b1)

    def gc(self, x, s, W, b):
        """graph convolution of [x, s] (B, N, C + H): L mixes the nodes, W the channels (TGCN.py:93-129)"""
        return torch.matmul(torch.matmul(self.L, torch.cat([x, s], dim=-1)), W) + b

    def forward(self, x, h):
        r, u = torch.sigmoid(self.gc(x, h, self.weights_0, self.bias_0)).split(self.num_units, dim=-1)
        c = torch.tanh(self.gc(x, r * h, self.weights_1, self.bias_1))
        return u * h + (1.0 - u) * c


class TGCN(nn.Module):
    """``args_predictor``: num_nodes, input_window, output_window, rnn_units, output_dim, G (N, N) = graph.tgcn_graph(adjacency) — the fields of
    reference TGCN/args.py:14-21 with the graph already normalised (the reference normalises ``adj_mx`` inside the cell).

    As with STGCN the two backends differ in one observable way: in eval mode the HIP path runs under ``no_grad`` and keeps nothing for a
    backward, so its output has ``requires_grad == False`` even when gradients are enabled.  Gradients through ``backend="hip"`` need ``train()`` mode."""

    def __init__(self, args_predictor, device, dim_in, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("TGCN", backend), None
        a = args_predictor
        self.num_nodes, self.input_dim, self.output_dim, self.gru_units = a.num_nodes, dim_in, a.output_dim, a.rnn_units
        self.input_window, self.output_window = a.input_window, a.output_window
        self.tgcn_model = _Cell(a.rnn_units, torch.as_tensor(a.G, dtype=torch.float32).to(device), dim_in)
        self.output_model = nn.Linear(a.rnn_units, a.output_window * a.output_dim)

    def head(self, h):
        """h (B, N, H) -> (B, W, N, output_dim)   (TGCN.py:171-175)"""
        y = self.output_model(h).view(h.shape[0], self.num_nodes, self.output_window, self.output_dim)
        return y.permute(0, 2, 1, 3)

    def forward(self, x):                                                  # x (B, T, N, dim_in)
        y = _backend.hip_forward(self, "tgcn_hip", x)
        if y is not None:
            return y
        h = x.new_zeros(x.shape[0], self.num_nodes, self.gru_units)
        for t in range(x.shape[1]):
            h = self.tgcn_model(x[:, t], h)
        return self.head(h)
