"""DMVST-Net predictor (after Yao et al., "Deep Multi-View Spatial-Temporal Network for Taxi Demand Prediction", AAAI 2018) as the reference
wires it behind the enhanced embedding: ``-mode eval -model DMVSTNET`` (reference model/DMVSTNET_demand/DMVSTNET.py ``DMVSTNet``,
``Local_GNN``).  x (B, T, N, dim_in) -> (B, T, N, dim_out), T = input_window.  Three views of x, with h = hidden_dim and H = h * dim_out:

    spatial     spa = Lin_in_spa(x);   S = Lin_spa(relu(Local_GNN1.lin(A spa))) + spa        A the raw, unnormalised (N, N) adjacency,
                                                                                              (A spa)[v] = sum_n A[v, n] spa[n]
    temporal    a one-layer LSTM(H -> H) over the B N rows of [S | Lin_in_tem(x)], zero initial state;
                top[t] = h_t + h_{T-1}: every step's output plus the last one
    semantic    sen[b, t, n] = Lin_in_sen(x)[b, t, n] W_n,   W_n (h, h) = sum_d node_embeddings[n, d] w[d]
    head        output([top | sen]): Linear(H + h, dim_out)

Restated with the SAME parameter tree, 22 keys in the reference's order and drawn in its construction order (the Linears and the LSTM, then
``node_embeddings`` and ``w`` with ``xavier_uniform_``, then ``output``).  What the restatement keeps and drops:

  * ``Local_GNN2`` and ``Local_GNN3`` are built and read by nothing: they keep their keys, never receive a gradient, and ``torch.optim.Adam``
    skips them, as in the reference.
  * the width of the LSTM's input, [S | tem], is 2 h, and the reference views it as h * dim_out: dim_out must be 2.
  * the reference's two ``squeeze`` calls (``hid.mean(0).squeeze(0)``, ``out_lstm.squeeze(1)``) are no-ops whenever T > 1 and B N > 1 (the
    squeezed axes then have more than one entry; ``hid`` has one layer, so its mean over them is itself): the code below has neither.
  * ``output_window`` is parsed and read by nothing in the model: the output has input_window steps.
  * the adjacency is a non-persistent buffer (a plain attribute of the reference's modules): no key of the state dict.

``DMVSTNET(..., backend="hip")`` runs the same parameters on the project's kernels wherever those serve the call (predictors/dmvstnet_hip.py,
csrc/dmvstnet.hip); elsewhere the forward takes the torch ops below.  ``backend_used`` records which of the two the last forward took.
"""
import torch
import torch.nn as nn

from . import _backend


class LocalGNN(nn.Module):
    """relu(lin(A x)): x (B, T, N, h), A (N, N)"""

    def __init__(self, hidden_dim):
        super().__init__()
        self.lin = nn.Linear(hidden_dim, hidden_dim)

    def forward(self, A, x):
        return torch.relu(self.lin(torch.einsum("vn,btnd->btvd", A, x)))


class DMVSTNET(nn.Module):
    """``args_predictor``: num_nodes, hidden_dim, topo_embedded_dim, input_window, output_window and the raw adjacency adj_mx (N, N) =
    graph.dmvstnet_adjacency — the fields of reference DMVSTNET_demand/args.py:16-33.

    As with the other predictors the two backends differ in one observable way: in eval mode the HIP path runs under ``no_grad`` and keeps
    nothing for a backward.  Gradients through ``backend="hip"`` need ``train()`` mode."""

    def __init__(self, args_predictor, device, dim_in, dim_out, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("DMVSTNET", backend), None
        a = args_predictor
        self.num_nodes, self.hidden_dim, self.topo_embedded_dim = a.num_nodes, a.hidden_dim, a.topo_embedded_dim
        self.input_window, self.output_window, self.dim_in, self.dim_out = a.input_window, a.output_window, dim_in, dim_out
        if dim_out != 2:
            raise ValueError("DMVSTNET feeds [spatial | temporal] (2 * hidden_dim wide) to an LSTM of width hidden_dim * dim_out: dim_out must "
                             "be 2, got %r" % (dim_out,))
        adj = torch.as_tensor(a.adj_mx, dtype=torch.float32)
        if tuple(adj.shape) != (a.num_nodes, a.num_nodes):
            raise ValueError("DMVSTNET adjacency must be (N, N) with N = %d, got %r" % (a.num_nodes, tuple(adj.shape)))
        self.register_buffer("adj_mx", adj.clone(), persistent=False)
        h, H = a.hidden_dim, a.hidden_dim * dim_out
        self.lstm_dim = H
        self.Lin_in_spa = nn.Linear(dim_in, h)                              # drawn in the reference's order
        self.Lin_in_tem = nn.Linear(dim_in, h)
        self.Lin_in_sen = nn.Linear(dim_in, h)
        self.Local_GNN1 = LocalGNN(h)
        self.Local_GNN2 = LocalGNN(h)                                      # built and read by nothing, as in the reference
        self.Local_GNN3 = LocalGNN(h)
        self.Lin_spa = nn.Linear(h, h)
        self.lstm = nn.LSTM(input_size=H, hidden_size=H, batch_first=True, num_layers=1)
        self.node_embeddings = nn.Parameter(torch.empty(a.num_nodes, a.topo_embedded_dim))
        nn.init.xavier_uniform_(self.node_embeddings)
        self.w = nn.Parameter(torch.empty(a.topo_embedded_dim, h, h))
        nn.init.xavier_uniform_(self.w)
        self.output = nn.Linear(H + h, dim_out)
        # the state dict lists parameters in registration order: the reference registers the two bare parameters after the LSTM, and
        # nn.Module keeps direct parameters ahead of the sub-modules' whatever the order — node_embeddings and w come first there too
        self.to(device)

    def forward(self, x):                                                  # x (B, T, N, dim_in)
        y = _backend.hip_forward(self, "dmvstnet_hip", x)
        if y is not None:
            return y
        B, T, N, _ = x.shape
        H = self.lstm_dim
        spa, tem, sen = self.Lin_in_spa(x), self.Lin_in_tem(x), self.Lin_in_sen(x)
        S = self.Lin_spa(self.Local_GNN1(self.adj_mx, spa)) + spa
        rows = torch.cat([S, tem], dim=-1).permute(0, 2, 1, 3).reshape(B * N, T, H)
        out, _ = self.lstm(rows)                                           # zero initial state
        top = (out + out[:, -1:, :]).view(B, N, T, H).transpose(1, 2)      # h_t + h_{T-1}
        weights = torch.einsum("nd,dio->nio", self.node_embeddings, self.w)
        sen = torch.einsum("btni,nio->btno", sen, weights)
        return self.output(torch.cat([top, sen], dim=-1))
