"""STSGCN predictor (Song et al., AAAI 2020) as the reference wires it behind the enhanced embedding: ``-mode eval -model STSGCN``
(reference model/STSGCN/STSGCN.py).  Restated with the SAME parameter tree, key for key and in the same order — the ``ouput_layer`` typo and
the ``stsgcl_layers.L.layer.gcms.W.layers.J.layer`` path included, so a reference checkpoint loads with ``load_state_dict`` — and the same
arithmetic.  Rows (b, t, n), channels last.

    embedding   relu(Linear) of the input
    layer       for each entry of filter_list, over the T current frames: add the position embeddings (1, T, 1, C) and (1, 1, N, C); for each of
                the W = T - 2 windows of three frames, with the window's own weights (``individual``) or one set (``sharing``), J operations
                act(Linear(adj3 . data)) on the 3N rows of the window; each operation's output cropped to the middle N rows, element-wise max
                over the J operations; T shrinks by 2
    heads       output_window heads Linear(T' C -> 128), Linear(128 -> dim_out), no activation between; concatenated to (B, P, N, dim_out)

adj3 (3N, 3N) is the reference's ``construct_adj``: A on the three diagonal blocks, identity on the blocks of adjacent steps, every diagonal
entry 1.  With A^ = graph.stsgcn_graph(A) (A with a unit diagonal) that is  (adj3 S)_k = A^ S_k + [k >= 1] S_{k-1} + [k <= 1] S_{k+1};  the
torch backend keeps the dense product, the HIP backend (predictors/stsgcn_hip.py) never forms the matrix.  It is a buffer outside the state dict.

The reference's loop over the windows (W x J small matmuls and Linears per layer) is batched here: the windows are stacked, the weights of an
operation are stacked (W, cw, ci), and an operation is one matmul with adj3 and one ``baddbmm``.  The heads are stacked the same way: one ``addmm``
over the concatenated hidden weights, one ``baddbmm`` for the output layers.  The position embeddings are zeros at construction, on the module's
device (the reference pins them to 'cuda:0').  ``use_mask=True`` is not built: no conf uses it, and the reference's form (a Parameter multiplied
into the adjacency once, at construction) needs ``retain_graph`` on every backward.

``STSGCN(..., backend="hip")`` runs the same parameter tree on the project's kernels wherever those serve the call; elsewhere the forward takes
the torch modules.  ``backend_used`` records which of the two the last forward took.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _backend
from ..graph import stsgcn_graph


def window_adjacency(a_hat, steps=3):
    """adj3 (steps N, steps N) from A^ (N, N): A^ on the diagonal blocks, identity on the blocks of adjacent steps (= construct_adj)"""
    n = a_hat.shape[0]
    adj = a_hat.new_zeros(steps * n, steps * n)
    eye = torch.eye(n, dtype=a_hat.dtype, device=a_hat.device)
    for k in range(steps):
        adj[k * n:(k + 1) * n, k * n:(k + 1) * n] = a_hat
        if k + 1 < steps:
            adj[k * n:(k + 1) * n, (k + 1) * n:(k + 2) * n] = eye
            adj[(k + 1) * n:(k + 2) * n, k * n:(k + 1) * n] = eye
    return adj


class PositionEmbedding(nn.Module):
    def __init__(self, t, n, c, temporal, spatial, device):
        super().__init__()
        self.temporal, self.spatial = temporal, spatial
        self.temporal_emb = nn.Parameter(torch.zeros(1, t, 1, c, device=device))
        self.spatial_emb = nn.Parameter(torch.zeros(1, 1, n, c, device=device))

    def forward(self, data):
        if self.temporal:
            data = data + self.temporal_emb
        if self.spatial:
            data = data + self.spatial_emb
        return data


class GcnOperation(nn.Module):
    """the parameters of act(Linear(adj3 . data)), one operation of one window.  The layer runs all its windows at once from the stacked
    weights (``_Layer.candidates``), so this module has no forward of its own."""

    def __init__(self, num_of_filter, num_of_features, activation):
        super().__init__()
        assert activation in {"GLU", "relu"}
        self.layer = nn.Linear(num_of_features, (2 if activation == "GLU" else 1) * num_of_filter)


def _activate(pre, co, activation):
    if activation == "GLU":
        lhs, rhs = pre.split(co, -1)
        return lhs * torch.sigmoid(rhs)
    return torch.relu(pre)


class Stsgcm(nn.Module):
    def __init__(self, filters, num_of_features, activation):
        super().__init__()
        self.layers = nn.ModuleList()
        for f in filters:
            self.layers.append(GcnOperation(f, num_of_features, activation))
            num_of_features = f


class _Layer(nn.Module):
    """STSGCNLayerIndividual (``gcms``: one Stsgcm per window) or STSGCNLayerSharing (``gcm``: one for all)"""

    def __init__(self, t, n, c, filters, activation, temporal, spatial, individual, device):
        super().__init__()
        self.T, self.N, self.filters, self.activation, self.individual = t, n, list(filters), activation, individual
        self.position_embedding = PositionEmbedding(t, n, c, temporal, spatial, device)
        if individual:
            self.gcms = nn.ModuleList([Stsgcm(filters, c, activation) for _ in range(t - 2)])
        else:
            self.gcm = Stsgcm(filters, c, activation)

    def stacked(self, j):
        """weight (W | 1, cw, ci) and bias (W | 1, cw) of operation j"""
        ms = self.gcms if self.individual else [self.gcm]
        return torch.stack([m.layers[j].layer.weight for m in ms]), torch.stack([m.layers[j].layer.bias for m in ms])

    def candidates(self, data, adj):
        """data (B, T, N, C), embeddings added -> (J, B, W, N, co): every operation's output on the middle block of every window"""
        b, t, n, _ = data.shape
        w = t - 2
        cur = torch.stack([data[:, i:i + 3].reshape(b, 3 * n, -1) for i in range(w)])             # (W, B, 3N, C)
        out = []
        for j, co in enumerate(self.filters):
            wt, bs = self.stacked(j)
            z = torch.matmul(adj, cur).reshape(w, b * 3 * n, -1)
            if self.individual:
                pre = torch.baddbmm(bs[:, None, :], z, wt.transpose(1, 2))
            else:
                pre = F.linear(z, wt[0], bs[0])
            cur = _activate(pre, co, self.activation).reshape(w, b, 3 * n, co)
            out.append(cur[:, :, n:2 * n].transpose(0, 1))
        return torch.stack(out)

    def forward(self, data, adj):
        return self.candidates(self.position_embedding(data), adj).max(dim=0)[0]


class STSGCL(nn.Module):
    def __init__(self, t, n, c, filters, module_type, activation, temporal, spatial, device):
        super().__init__()
        assert module_type in {"sharing", "individual"}
        self.layer = _Layer(t, n, c, filters, activation, temporal, spatial, module_type == "individual", device)

    def forward(self, data, adj):
        return self.layer(data, adj)


class OutputLayer(nn.Module):
    def __init__(self, input_length, num_of_features, num_of_filters, predict_length, output_dim):
        super().__init__()
        self.hidden_layer = nn.Linear(input_length * num_of_features, num_of_filters)
        self.ouput_layer = nn.Linear(num_of_filters, predict_length * output_dim)


class STSGCN(nn.Module):
    """``args``: num_nodes, feature_dim, input_window, output_window, filter_list, module_type, activation, temporal_emb, spatial_emb, use_mask,
    steps, first_layer_embedding_size and A, the raw (N, N) adjacency — the fields of reference STSGCN.py:256-313.

    Takes (B, input_window, N, dim_in), returns (B, output_window, N, dim_out)."""

    def __init__(self, args, device, dim_in, dim_out, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("STSGCN", backend), None
        a = args
        if a.use_mask:
            raise NotImplementedError("STSGCN use_mask=True is not built: no conf uses it and the reference's form needs retain_graph")
        if a.steps != 3:
            raise NotImplementedError("STSGCN is built for windows of 3 steps (every conf), got %r" % (a.steps,))
        self.num_nodes, self.feature_dim, self.dim_out = a.num_nodes, a.feature_dim, dim_out
        self.input_window, self.output_window = a.input_window, a.output_window
        self.module_type, self.activation, self.use_mask = a.module_type, a.activation, False
        a_hat = stsgcn_graph(np.asarray(a.A))
        self.register_buffer("a_hat", a_hat, persistent=False)
        self.register_buffer("adj", window_adjacency(a_hat, a.steps), persistent=False)
        c = dim_in
        if a.first_layer_embedding_size:
            self.first_layer_embedding = nn.Linear(c, a.first_layer_embedding_size)
            c = a.first_layer_embedding_size
        else:
            self.first_layer_embedding = None
        t = a.input_window
        self.stsgcl_layers = nn.ModuleList()
        for filters in a.filter_list:
            self.stsgcl_layers.append(STSGCL(t, a.num_nodes, c, filters, a.module_type, a.activation, a.temporal_emb, a.spatial_emb, device))
            t, c = t - 2, filters[-1]
        self.outputs = nn.ModuleList([OutputLayer(t, c, 128, 1, dim_out) for _ in range(a.output_window)])
        self.to(device)

    def head(self, h):
        """h (B, T', N, C) -> (B, P, N, dim_out): the P heads as one addmm over the concatenated hidden weights and one baddbmm"""
        b, _, n, _ = h.shape
        p = len(self.outputs)
        flat = h.transpose(1, 2).reshape(b * n, -1)
        hw = torch.cat([o.hidden_layer.weight for o in self.outputs])                                  # (P 128, T' C)
        hid = torch.addmm(torch.cat([o.hidden_layer.bias for o in self.outputs]), flat, hw.t())
        ow = torch.stack([o.ouput_layer.weight for o in self.outputs])                                 # (P, dim_out, 128)
        ob = torch.stack([o.ouput_layer.bias for o in self.outputs])
        y = torch.baddbmm(ob[:, None, :], hid.view(b * n, p, -1).transpose(0, 1), ow.transpose(1, 2))  # (P, B N, dim_out)
        return y.view(p, b, n, -1).permute(1, 0, 2, 3)

    def forward(self, x):                                                  # x (B, T, N, dim_in)
        if x.shape[-1] > self.feature_dim:
            x = x[..., :self.feature_dim]
        y = _backend.hip_forward(self, "stsgcn_hip", x)
        if y is not None:
            return y
        h = x
        if self.first_layer_embedding is not None:
            h = torch.relu(self.first_layer_embedding(h))
        for lay in self.stsgcl_layers:
            h = lay(h, self.adj)
        return self.head(h)
