"""STFGNN predictor (Li & Zhu, AAAI 2021) as the reference wires it behind the enhanced embedding: ``-mode eval -model STFGNN``
(reference model/STFGNN/STFGNN.py).  Restated with the SAME parameter tree, key for key and in the same order — ``First_FC``,
``STSGCLS.L.temporal_embedding`` / ``.spatial_embedding`` / ``.conv1`` / ``.conv2`` / ``.STSGCMS.W.gcn_operations.J.FC``, ``predictLayer.P.FC1`` /
``.FC2`` — so a reference checkpoint loads with ``load_state_dict``, and the same arithmetic.  Rows (b, t, n), channels last.

    embedding   relu(First_FC) of the input
    layer       for each entry of hidden_dims, over the T current frames: add the position embeddings (1, T, 1, C) and (1, 1, N, C), then
                  gated branch   sigmoid(conv1(x)) * tanh(conv2(x)), each conv two taps with dilation 3 along T:
                                 out[t] = W[..., 0] x[t] + W[..., 1] x[t + 3] + b, T - 3 frames
                  windows        for each of the W = T - 3 windows of four frames, with the window's own weights, J operations
                                 act(Linear(adj . data)) on the 4N rows of the window; each operation's output cropped to rows N .. 2N,
                                 element-wise max over the J operations
                the layer returns max + gated branch; T shrinks by 3
    heads       horizon heads FC2(FC1(.)), T' C -> out_layer_dim -> output_dim, no activation between; concatenated to (B, horizon, N, output_dim)

adj (4N, 4N) is the reference's spatial-temporal fusion graph (``graph.stfgnn_fusion_graph``); the torch backend keeps the dense product, the
HIP backend (predictors/stfgnn_hip.py) multiplies by its two N x N blocks where ``graph.stfgnn_blocks`` recognises the form.  It is a buffer
outside the state dict.

The reference declares the two convolutions as ``nn.Conv1d`` with 2-tuple kernels and applies them to 4-D input, which the PyTorch it was
written for ran as a 2-D convolution and a current one refuses.  Here they are ``nn.Conv2d`` of the same arguments: the same (Cout, C, 1, 2)
parameters under the same keys, the same seeded initialisation, the same arithmetic.

The reference's loop over the windows is batched as in stsgcn.py: the windows are stacked, the weights of an operation are stacked (W, cw, ci),
and an operation is one matmul with adj and one ``baddbmm``; the heads are one ``addmm`` over the concatenated FC1 weights and one
``baddbmm``.  The position embeddings are drawn as the reference draws them, ``xavier_normal_`` with gain 0.0003.  ``use_mask=True`` is not
built: no conf uses it, and the reference's form (a Parameter multiplied into the adjacency inside every operation) is another model.

``STFGNN(..., backend="hip")`` runs the same parameter tree on the project's kernels wherever those serve the call; elsewhere the forward takes
the torch modules.  ``backend_used`` records which of the two the last forward took.
"""
import torch
import torch.nn as nn

from . import _backend
from ..graph import stfgnn_blocks


class GcnOperation(nn.Module):
    """the parameters of act(Linear(adj . data)), one operation of one window.  The layer runs all its windows at once from the stacked
    weights (``STSGCL.candidates``), so this module has no forward of its own."""

    def __init__(self, in_dim, out_dim, activation):
        super().__init__()
        assert activation in {"GLU", "relu"}
        self.FC = nn.Linear(in_dim, (2 if activation == "GLU" else 1) * out_dim)


class STSGCM(nn.Module):
    def __init__(self, in_dim, out_dims, activation):
        super().__init__()
        self.gcn_operations = nn.ModuleList()
        for f in out_dims:
            self.gcn_operations.append(GcnOperation(in_dim, f, activation))
            in_dim = f


def _activate(pre, co, activation):
    if activation == "GLU":
        lhs, rhs = pre.split(co, -1)
        return lhs * torch.sigmoid(rhs)
    return torch.relu(pre)


class STSGCL(nn.Module):
    def __init__(self, history, n, in_dim, out_dims, strides, activation, temporal, spatial):
        super().__init__()
        self.T, self.N, self.in_dim, self.out_dims, self.strides, self.activation = history, n, in_dim, list(out_dims), strides, activation
        self.temporal_emb, self.spatial_emb = temporal, spatial
        self.conv1 = nn.Conv2d(in_dim, out_dims[-1], kernel_size=(1, 2), stride=(1, 1), dilation=(1, 3))
        self.conv2 = nn.Conv2d(in_dim, out_dims[-1], kernel_size=(1, 2), stride=(1, 1), dilation=(1, 3))
        self.STSGCMS = nn.ModuleList([STSGCM(in_dim, out_dims, activation) for _ in range(history - strides + 1)])
        if temporal:
            self.temporal_embedding = nn.Parameter(torch.empty(1, history, 1, in_dim))
            nn.init.xavier_normal_(self.temporal_embedding, gain=0.0003)
        if spatial:
            self.spatial_embedding = nn.Parameter(torch.empty(1, 1, n, in_dim))
            nn.init.xavier_normal_(self.spatial_embedding, gain=0.0003)

    def embed(self, x):
        if self.temporal_emb:
            x = x + self.temporal_embedding
        if self.spatial_emb:
            x = x + self.spatial_embedding
        return x

    def gated(self, x):
        """x (B, T, N, C), embeddings added -> (B, T - 3, N, Cout)"""
        xt = x.permute(0, 3, 2, 1)                                          # (B, C, N, T)
        return (torch.sigmoid(self.conv1(xt)) * torch.tanh(self.conv2(xt))).permute(0, 3, 2, 1)

    def stacked(self, j):
        """weight (W, cw, ci) and bias (W, cw) of operation j"""
        return (torch.stack([m.gcn_operations[j].FC.weight for m in self.STSGCMS]),
                torch.stack([m.gcn_operations[j].FC.bias for m in self.STSGCMS]))

    def candidates(self, x, adj):
        """x (B, T, N, C), embeddings added -> (J, B, W, N, co): every operation's output on rows N .. 2N of every window"""
        b, t, n, _ = x.shape
        k = self.strides
        w = t - k + 1
        cur = torch.stack([x[:, i:i + k].reshape(b, k * n, -1) for i in range(w)])               # (W, B, 4N, C)
        out = []
        for j, co in enumerate(self.out_dims):
            wt, bs = self.stacked(j)
            z = torch.matmul(adj, cur).reshape(w, b * k * n, -1)
            pre = torch.baddbmm(bs[:, None, :], z, wt.transpose(1, 2))
            cur = _activate(pre, co, self.activation).reshape(w, b, k * n, co)
            out.append(cur[:, :, n:2 * n].transpose(0, 1))
        return torch.stack(out)

    def forward(self, x, adj):
        x = self.embed(x)
        return self.candidates(x, adj).max(dim=0)[0] + self.gated(x)


class OutputLayer(nn.Module):
    def __init__(self, history, in_dim, out_dim, hidden_dim, horizon):
        super().__init__()
        self.FC1 = nn.Linear(in_dim * history, hidden_dim)
        self.FC2 = nn.Linear(hidden_dim, horizon * out_dim)


class STFGNN(nn.Module):
    """``args``: window, horizon, num_nodes, hidden_dims, first_layer_embedding_size, out_layer_dim, output_dim, strides, temporal_emb,
    spatial_emb, activation, use_mask and adj, the dense (4N, 4N) fusion matrix — the fields of reference STFGNN.py:245-264.

    Takes (B, window, N, dim_in), returns (B, horizon, N, output_dim)."""

    def __init__(self, args, device, dim_in, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("STFGNN", backend), None
        a = args
        if a.use_mask:
            raise NotImplementedError("STFGNN use_mask=True is not built: no conf uses it and the reference's form is a model of its own")
        if a.strides != 4:
            raise NotImplementedError("STFGNN is built for windows of 4 steps (every conf, and the fusion graph's four blocks), got %r" % (a.strides,))
        self.num_nodes, self.window, self.horizon, self.output_dim = a.num_nodes, a.window, a.horizon, a.output_dim
        self.hidden_dims, self.activation, self.use_mask, self.strides = [list(h) for h in a.hidden_dims], a.activation, False, a.strides
        adj = torch.as_tensor(a.adj, dtype=torch.float32)
        if tuple(adj.shape) != (4 * a.num_nodes, 4 * a.num_nodes):
            raise ValueError("STFGNN adj must be (4 N, 4 N) = %d squared, got %r" % (4 * a.num_nodes, tuple(adj.shape)))
        self.register_buffer("adj", adj.clone(), persistent=False)
        blocks = stfgnn_blocks(adj)                                          # (S^, D) where adj is a fusion graph: what the HIP backend multiplies by
        self.register_buffer("s_hat", None if blocks is None else blocks[0], persistent=False)
        self.register_buffer("d_hat", None if blocks is None else blocks[1], persistent=False)
        self.First_FC = nn.Linear(dim_in, a.first_layer_embedding_size)
        t, c = a.window, a.first_layer_embedding_size
        self.STSGCLS = nn.ModuleList()
        for dims in self.hidden_dims:
            self.STSGCLS.append(STSGCL(t, a.num_nodes, c, dims, a.strides, a.activation, a.temporal_emb, a.spatial_emb))
            t, c = t - (a.strides - 1), dims[-1]
        self.predictLayer = nn.ModuleList([OutputLayer(t, c, a.output_dim, a.out_layer_dim, 1) for _ in range(a.horizon)])
        self.to(device)

    def head(self, h):
        """h (B, T', N, C) -> (B, horizon, N, output_dim): the heads as one addmm over the concatenated FC1 weights and one baddbmm"""
        b, _, n, _ = h.shape
        p = len(self.predictLayer)
        flat = h.transpose(1, 2).reshape(b * n, -1)
        hw = torch.cat([o.FC1.weight for o in self.predictLayer])                                      # (P hidden, T' C)
        hid = torch.addmm(torch.cat([o.FC1.bias for o in self.predictLayer]), flat, hw.t())
        ow = torch.stack([o.FC2.weight for o in self.predictLayer])                                    # (P, output_dim, hidden)
        ob = torch.stack([o.FC2.bias for o in self.predictLayer])
        y = torch.baddbmm(ob[:, None, :], hid.view(b * n, p, -1).transpose(0, 1), ow.transpose(1, 2))  # (P, B N, output_dim)
        return y.view(p, b, n, -1).permute(1, 0, 2, 3)

    def forward(self, x):                                                  # x (B, T, N, dim_in)
        y = _backend.hip_forward(self, "stfgnn_hip", x)
        if y is not None:
            return y
        h = torch.relu(self.First_FC(x))
        for lay in self.STSGCLS:
            h = lay(h, self.adj)
        return self.head(h)
