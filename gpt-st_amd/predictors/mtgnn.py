"""MTGNN predictor (Wu et al., KDD 2020) as the reference wires it behind the enhanced embedding: ``-mode eval -model MTGNN``
(reference model/MTGNN/MTGNN.py:330-501 with ``idx=None``, constructed in model/Model.py:52-54).  A WaveNet-style stack over a graph the
model learns itself:

    adp   = relu(tanh(a (n1 n2^T - n2 n1^T))) * topk-mask          n_i = tanh(a lin_i(emb_i))                       (GraphConstructor)
    x_0   = start_conv(pad(input))          skip = skip0(dropout(pad(input)))          pad: zeros on the left up to the receptive field
    layer:  g = dropout(tanh(filter(x)) * sigmoid(gate(x)))        filter, gate: four valid time convolutions (2, 3, 6, 7 taps), right-aligned
            skip += skip_conv(g)                                    (contracts the whole remaining time axis: T = 1)
            x = LayerNorm_(C,N,T)(mixprop(g, adp) + mixprop(g, adp^T) + x[..., -T:])
    y     = end_conv_2(relu(end_conv_1(relu(skipE(x) + skip))))    (B, output_window, N, output_dim)

Restated with the SAME module tree and attribute names (94 state-dict keys at three layers, ``residual_convs.*`` included although nothing
uses them with ``gcn_true``), so a reference checkpoint loads with ``load_state_dict(strict=True)``, and the same construction order, so a
seeded construction equals the reference's.  ``predefined_A`` is a plain attribute and ``idx`` a non-persistent buffer: neither is in the
state dict, as in the reference.

Dropout masks are drawn through one hook, ``_keep(tag, like)``; by default it draws what ``F.dropout`` draws for the reference's tensors in
the reference's order, so on the CPU a seeded training-mode forward equals the reference's.  Tests replace it to inject fixed masks.

The torch ops below are the default.  ``MTGNN(..., backend="hip")`` runs the same parameters on the project's own kernels
(predictors/mtgnn_hip.py, csrc/mtgnn.hip) wherever those serve the call, active dropout included; elsewhere (a CPU input, an unsupported
width) the forward takes the torch ops.  ``backend_used`` records which of the two the last forward took.  As with STGCN and TGCN, in eval
mode the HIP path runs under ``no_grad`` and keeps nothing for a backward, so its output has ``requires_grad == False`` even when gradients
are enabled: gradients through ``backend="hip"`` need ``train()`` mode.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _backend

KERNEL_SET = (2, 3, 6, 7)                                                  # the inception's tap counts; the widest sets the output length


class _Lin(nn.Module):
    """``mlp``: a 1x1 convolution (MTGNN.py:27-33)"""

    def __init__(self, c_in, c_out):
        super().__init__()
        self.mlp = nn.Conv2d(c_in, c_out, kernel_size=(1, 1))

    def forward(self, x):
        return self.mlp(x)


class MixProp(nn.Module):
    """mix-hop propagation: h_0 = x, h_k = alpha x + (1 - alpha) a h_{k-1} with a = (adj + I) / rowsum, then a 1x1 over [h_0 .. h_gdep]
    (MTGNN.py:57-77).  ``a`` multiplies untransposed: out[v] = sum_w a[v, w] h[w]."""

    def __init__(self, c_in, c_out, gdep, alpha):
        super().__init__()
        self.mlp = _Lin((gdep + 1) * c_in, c_out)
        self.gdep, self.alpha = gdep, alpha

    @staticmethod
    def normalised(adj):
        adj = adj + torch.eye(adj.shape[0], dtype=adj.dtype, device=adj.device)
        return adj / adj.sum(1).view(-1, 1)

    def forward(self, x, adj):                                             # x (B, C, N, T)
        a, h, hops = self.normalised(adj), x, [x]
        for _ in range(self.gdep):
            h = self.alpha * x + (1 - self.alpha) * torch.einsum("ncwl,vw->ncvl", h, a).contiguous()
            hops.append(h)
        return self.mlp(torch.cat(hops, dim=1))


class DilatedInception(nn.Module):
    """four valid convolutions along time with 2, 3, 6 and 7 taps, cout / 4 channels each, cropped on the left to the 7-tap length and
    concatenated (MTGNN.py:130-146)"""

    def __init__(self, cin, cout, dilation_factor=1):
        super().__init__()
        self.kernel_set = list(KERNEL_SET)
        self.tconv = nn.ModuleList(nn.Conv2d(cin, cout // len(KERNEL_SET), (1, k), dilation=(1, dilation_factor)) for k in KERNEL_SET)

    def forward(self, x):
        ys = [conv(x) for conv in self.tconv]
        return torch.cat([y[..., -ys[-1].shape[3]:] for y in ys], dim=1)


class GraphConstructor(nn.Module):
    """the learned, directed, top-k sparsified adjacency (MTGNN.py:149-187).  The mask is a constant: gradients reach the embeddings through
    the kept entries.  It is built in the dtype of ``adj``, so a ``.double()`` copy of the module works."""

    def __init__(self, nnodes, k, dim, alpha=3):
        super().__init__()
        self.nnodes, self.k, self.dim, self.alpha = nnodes, k, dim, alpha
        self.emb1, self.emb2 = nn.Embedding(nnodes, dim), nn.Embedding(nnodes, dim)
        self.lin1, self.lin2 = nn.Linear(dim, dim), nn.Linear(dim, dim)

    def dense(self, idx):
        n1 = torch.tanh(self.alpha * self.lin1(self.emb1(idx)))
        n2 = torch.tanh(self.alpha * self.lin2(self.emb2(idx)))
        a = torch.mm(n1, n2.transpose(1, 0)) - torch.mm(n2, n1.transpose(1, 0))
        return F.relu(torch.tanh(self.alpha * a))

    def topk_mask(self, adj):
        with torch.no_grad():
            return torch.zeros_like(adj).scatter_(1, adj.topk(self.k, 1)[1], 1.0)

    def forward(self, idx):
        adj = self.dense(idx)
        return adj * self.topk_mask(adj)


class LayerNorm(nn.Module):
    """layer norm over all of (C, N, T) of a batch element with affine weights of that shape (MTGNN.py:294-323 at idx = all nodes)"""

    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True):
        super().__init__()
        self.normalized_shape, self.eps, self.elementwise_affine = tuple(normalized_shape), eps, elementwise_affine
        if elementwise_affine:
            self.weight = nn.Parameter(torch.ones(*normalized_shape))
            self.bias = nn.Parameter(torch.zeros(*normalized_shape))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)

    def forward(self, x):
        return F.layer_norm(x, tuple(x.shape[1:]), self.weight, self.bias, self.eps)


def time_spans(layers, q, kernel=7):
    """how many time steps the first j layers consume, j = 0 .. layers, and each layer's dilation (MTGNN.py:385-434)"""
    spans = [(kernel - 1) * (q ** j - 1) // (q - 1) if q > 1 else j * (kernel - 1) for j in range(layers + 1)]
    return spans, [q ** j for j in range(layers)]


class MTGNN(nn.Module):
    """``args_predictor``: the fields of reference MTGNN/args.py:13-34 and ``adj_mx`` (it feeds only ``predefined_A``, which nothing reads
    with ``buildA_true``).  ``use_curriculum_learning`` and ``task_level`` are stored and, as in the reference, read by nothing."""

    def __init__(self, args_predictor, device, dim_in, dim_out, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("MTGNN", backend), None
        a = args_predictor
        self.num_nodes, self.feature_dim, self.output_dim = a.num_nodes, dim_in, dim_out
        self.input_window, self.output_window = a.input_window, a.output_window
        self.gcn_true, self.buildA_true, self.gcn_depth, self.dropout = a.gcn_true, a.buildA_true, a.gcn_depth, a.dropout
        self.subgraph_size, self.node_dim, self.dilation_exponential = a.subgraph_size, a.node_dim, a.dilation_exponential
        self.conv_channels, self.residual_channels = a.conv_channels, a.residual_channels
        self.skip_channels, self.end_channels = a.skip_channels, a.end_channels
        self.layers, self.propalpha, self.tanhalpha, self.layer_norm_affline = a.layers, a.propalpha, a.tanhalpha, a.layer_norm_affline
        self.use_curriculum_learning, self.task_level = a.use_curriculum_learning, a.task_level
        self.register_buffer("idx", torch.arange(self.num_nodes, device=device), persistent=False)
        adj = getattr(a, "adj_mx", None)
        self.predefined_A = None if adj is None else (torch.as_tensor(adj) - torch.eye(self.num_nodes)).to(device)

        spans, dilations = time_spans(self.layers, self.dilation_exponential)
        self.receptive_field = dim_out + spans[-1]
        self.total_window = max(self.input_window, self.receptive_field)  # the time length after the left pad
        self.frames = [self.total_window - s for s in spans]              # T of the input and of every layer's output
        C, R, S = self.conv_channels, self.residual_channels, self.skip_channels

        # registration order (= state-dict order) and construction order (= random stream) are both the reference's (MTGNN.py:372-451)
        for name in ("filter_convs", "gate_convs", "residual_convs", "skip_convs", "gconv1", "gconv2", "norm"):
            setattr(self, name, nn.ModuleList())
        self.start_conv = nn.Conv2d(dim_in, R, kernel_size=(1, 1))
        self.gc = GraphConstructor(self.num_nodes, self.subgraph_size, self.node_dim, alpha=self.tanhalpha)
        for j in range(self.layers):
            self.filter_convs.append(DilatedInception(R, C, dilations[j]))
            self.gate_convs.append(DilatedInception(R, C, dilations[j]))
            self.residual_convs.append(nn.Conv2d(C, R, kernel_size=(1, 1)))                 # built and, with gcn_true, never used
            self.skip_convs.append(nn.Conv2d(C, S, kernel_size=(1, self.frames[j + 1])))
            if self.gcn_true:
                self.gconv1.append(MixProp(C, R, self.gcn_depth, self.propalpha))
                self.gconv2.append(MixProp(C, R, self.gcn_depth, self.propalpha))
            self.norm.append(LayerNorm((R, self.num_nodes, self.frames[j + 1]), elementwise_affine=self.layer_norm_affline))
        self.end_conv_1 = nn.Conv2d(S, self.end_channels, kernel_size=(1, 1))
        self.end_conv_2 = nn.Conv2d(self.end_channels, self.output_window, kernel_size=(1, 1))
        self.skip0 = nn.Conv2d(dim_in, S, kernel_size=(1, self.total_window))
        self.skipE = nn.Conv2d(R, S, kernel_size=(1, self.frames[-1] - dim_out + 1))

    def _keep(self, tag, like):
        """the dropout multiplier of one site (0 or 1 / (1 - p), shaped like ``like``), or None where dropout is off.  ``tag`` names the
        site: "in" for the padded input, "l<i>" for layer i's gated output.  ``x * _keep(..)`` is what ``F.dropout(x)`` computes, drawn
        from the same random stream."""
        if not self.training or self.dropout == 0:
            return None
        return F.dropout(torch.ones_like(like), self.dropout, True)

    def _drop(self, tag, x):
        keep = self._keep(tag, x)
        return x if keep is None else x * keep

    def adjacency(self):
        return self.gc(self.idx) if self.buildA_true else self.predefined_A

    def forward(self, source):                                             # (B, input_window, N, dim_in)
        y = _backend.hip_forward(self, "mtgnn_hip", source)
        if y is not None:
            return y
        x = source.transpose(1, 3)                                         # (B, dim_in, N, T)
        assert x.shape[3] == self.input_window, "input sequence length not equal to preset sequence length"
        if self.input_window < self.receptive_field:
            x = F.pad(x, (self.receptive_field - self.input_window, 0, 0, 0))
        adp = self.adjacency() if self.gcn_true else None
        skip = self.skip0(self._drop("in", x))                             # T = 1
        x = self.start_conv(x)
        for i in range(self.layers):
            residual = x
            x = self._drop("l%d" % i, torch.tanh(self.filter_convs[i](x)) * torch.sigmoid(self.gate_convs[i](x)))
            skip = self.skip_convs[i](x) + skip
            x = self.gconv1[i](x, adp) + self.gconv2[i](x, adp.transpose(1, 0)) if self.gcn_true else self.residual_convs[i](x)
            x = self.norm[i](x + residual[..., -x.shape[3]:])
        skip = self.skipE(x) + skip                                        # T = output_dim + T = 1: broadcasts at output_dim 2
        return self.end_conv_2(F.relu(self.end_conv_1(F.relu(skip))))     # (B, output_window, N, output_dim)
