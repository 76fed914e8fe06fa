"""ST-MGCN predictor (Geng et al., "Spatiotemporal Multi-Graph Convolution Network for Ride-hailing Demand Forecasting", AAAI 2019) as the
reference wires it behind the enhanced embedding: ``-mode eval -model STMGCN`` (reference model/STMGCN_demand/STMGCN.py ``ST_MGCN``,
``CG_LSTM``, GCN.py ``GCN``).  x (B, T, N, dim_in) -> (B, T, N, dim_out), T = seq_len; M = 2 branches, branch 0 on the distance graph and
branch 1 on the correlation graph, each graph a (3, N, N) stack of Chebyshev supports (``graph.stmgcn_supports``).  Per branch:

    x_seq = x.sum(-1) as (B, N, T);   x_hat = x_seq + relu(GCN_T(x_seq));   z = mean over the nodes (B, T)
    s     = sigmoid(fc(relu(fc(z))))                       the SAME Linear(T, T) twice: the context gate, one scalar per (b, t)
    LSTM(dim_in -> H, L layers) over the B N rows of s[b, t] x, zero initial state;  the top layer's last step (B, N, H)
    GCN(3 H -> gcn_hidden_dim, relu) on that graph

The branches are summed, then Linear(gcn_hidden_dim, dim_out T), viewed (B, N, T, dim_out) and transposed to (B, T, N, dim_out).

Restated with the SAME parameter tree, key for key and drawn in the reference's order (38 keys at three LSTM layers): ``rnn_list.m.
{gconv_temporal_feats.W, .b, fc.weight, fc.bias, lstm.*}``, ``gcn_list.m.{W, b}``, ``fc.weight``, ``fc.bias``; the LSTM is ``nn.LSTM``.  The
graph convolutions apply ReLU whatever ``gconv_activation`` says (the reference parses it and reads it nowhere).  The two graphs are
non-persistent buffers (plain attributes of the reference's module): no key of the state dict.

``STMGCN(..., backend="hip")`` runs the same parameters on the project's kernels wherever those serve the call (predictors/stmgcn_hip.py,
csrc/stmgcn.hip); elsewhere the forward takes the torch ops below.  ``backend_used`` records which of the two the last forward took.
"""
import torch
import torch.nn as nn

from . import _backend


class GCN(nn.Module):
    """relu([A_k x]_k W + b): x (B, N, input_dim), A (K, N, N) -> (B, N, hidden_dim)"""

    def __init__(self, K, input_dim, hidden_dim, bias=True):
        super().__init__()
        self.K, self.input_dim, self.hidden_dim = K, input_dim, hidden_dim
        self.W = nn.Parameter(torch.empty(K * input_dim, hidden_dim))
        nn.init.xavier_normal_(self.W)
        if bias:
            self.b = nn.Parameter(torch.zeros(hidden_dim))
        else:
            self.b = None

    def forward(self, A, x):
        cat = torch.cat([torch.matmul(A[k], x) for k in range(self.K)], dim=-1)
        out = torch.matmul(cat, self.W)
        if self.b is not None:
            out = out + self.b
        return torch.relu(out)


class CGLSTM(nn.Module):
    """the context-gated LSTM of one graph"""

    def __init__(self, seq_len, n_nodes, input_dim, hidden_dim, num_layers, K, bias):
        super().__init__()
        self.seq_len, self.n_nodes, self.input_dim, self.hidden_dim, self.num_layers = seq_len, n_nodes, input_dim, hidden_dim, num_layers
        self.gconv_temporal_feats = GCN(K, seq_len, seq_len, bias)
        self.fc = nn.Linear(seq_len, seq_len)
        self.lstm = nn.LSTM(input_size=input_dim, hidden_size=hidden_dim, num_layers=num_layers, batch_first=True)

    def gate(self, A, x):
        """s (B, T): the weight of every step of every sample"""
        x_seq = x.sum(dim=-1).permute(0, 2, 1)                             # (B, N, T)
        x_hat = x_seq + self.gconv_temporal_feats(A, x_seq)
        z = x_hat.sum(dim=1) / x_hat.shape[1]
        return torch.sigmoid(self.fc(torch.relu(self.fc(z))))

    def forward(self, A, x):
        B, T, N, C = x.shape
        xs = x * self.gate(A, x).view(B, T, 1, 1)
        out, _ = self.lstm(xs.permute(0, 2, 1, 3).reshape(B * N, T, C))     # zero initial state
        return out[:, -1, :].reshape(B, N, self.hidden_dim)


class STMGCN(nn.Module):
    """``args_predictor``: seq_len, M (2), n_nodes, lstm_hidden_dim, lstm_num_layers, gcn_hidden_dim, gconv_use_bias, and the two support
    stacks dis_graph, pcc_graph (3, N, N) = graph.stmgcn_supports(raw graph) — the fields of reference STMGCN_demand/args.py:16-53.

    As with the other predictors the two backends differ in one observable way: in eval mode the HIP path runs under ``no_grad`` and keeps
    nothing for a backward.  Gradients through ``backend="hip"`` need ``train()`` mode."""

    def __init__(self, args_predictor, device, dim_in, dim_out, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("STMGCN", backend), None
        a = args_predictor
        self.M, self.seq_len, self.n_nodes, self.input_dim, self.output_dim = a.M, a.seq_len, a.n_nodes, dim_in, dim_out
        self.lstm_hidden_dim, self.lstm_num_layers, self.gcn_hidden_dim = a.lstm_hidden_dim, a.lstm_num_layers, a.gcn_hidden_dim
        graphs = [torch.as_tensor(g, dtype=torch.float32) for g in (a.dis_graph, a.pcc_graph)]
        if self.M != len(graphs):
            raise ValueError("STMGCN has two graphs (distance, correlation): M must be 2, got %r" % (a.M,))
        for g in graphs:
            if g.dim() != 3 or tuple(g.shape[1:]) != (a.n_nodes, a.n_nodes):
                raise ValueError("STMGCN supports must be (K, N, N) with N = %d, got %r" % (a.n_nodes, tuple(g.shape)))
        self.register_buffer("dis_graph", graphs[0].clone(), persistent=False)
        self.register_buffer("pcc_graph", graphs[1].clone(), persistent=False)
        K = graphs[0].shape[0]
        self.rnn_list, self.gcn_list = nn.ModuleList(), nn.ModuleList()
        for _ in range(self.M):                                            # drawn in the reference's order: CG_LSTM, GCN, CG_LSTM, GCN, fc
            self.rnn_list.append(CGLSTM(a.seq_len, a.n_nodes, dim_in, a.lstm_hidden_dim, a.lstm_num_layers, K, a.gconv_use_bias))
            self.gcn_list.append(GCN(K, a.lstm_hidden_dim, a.gcn_hidden_dim, a.gconv_use_bias))
        self.fc = nn.Linear(a.gcn_hidden_dim, dim_out * a.seq_len)
        self.to(device)

    def graphs(self):
        return [self.dis_graph, self.pcc_graph]

    def head(self, feats):
        """feats: the M branch outputs (B, N, H) of the LSTMs -> y (B, T, N, dim_out)"""
        fused = sum(self.gcn_list[m](A, feats[m]) for m, A in enumerate(self.graphs()))
        out = self.fc(fused)
        return out.view(out.shape[0], out.shape[1], self.seq_len, -1).transpose(1, 2)

    def forward(self, x):                                                  # x (B, T, N, dim_in)
        y = _backend.hip_forward(self, "stmgcn_hip", x)
        if y is not None:
            return y
        return self.head([self.rnn_list[m](A, x) for m, A in enumerate(self.graphs())])
