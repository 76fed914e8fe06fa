"""ASTGCN predictor (Guo et al., AAAI 2019) as the reference wires it behind the enhanced embedding: ``-mode eval -model ASTGCN``
(reference model/ASTGCN/ASTGCN.py:217-312).  Restated with the SAME parameter tree, key for key and in the same order — so a reference
checkpoint loads with ``load_state_dict`` — and the same arithmetic.  Layout inside the torch modules: the reference's (B, N, F, T).

    block:   E = temporal attention of x  ->  x_TAt = x E  ->  S = spatial attention of x_TAt
             ->  relu(sum_k (T_k * S_b)^T x theta_k)  ->  (1, 3) time conv  + 1x1 residual conv of x  ->  relu  ->  LayerNorm over channels
    head:    final_conv contracts (T, F) to num_for_predict * dim_out

The reference's quirks are kept: both attention softmaxes run over dim=1; the spatial attention sees the time-attended x_TAt while the Chebyshev
convolution runs on the plain x; the masked polynomial is applied transposed; ``final_conv`` has int(len_input / time_strides) input channels.
The reference's per-time-step Python loop of the graph convolution (T * K small batched matmuls, each materialising the (B, N, N) Hadamard
product) is one contraction per k here.  The polynomials are buffers outside the state dict (the reference keeps them as plain attributes).

Initialisation: as in the reference, the attention parameters (U1 U2 U3 be Ve, W1 W2 W3 bs Vs) and every Theta are allocated with ``torch.empty``
and NOT initialised here — no random numbers are drawn for them — because the reference relies on the xavier pass of its Run.py (``xavier`` is
True in all four ASTGCN confs) to fill them; Run.py's eval branch does the same and refuses ``-model ASTGCN`` with xavier off.  A seeded
construction therefore consumes the random stream exactly as the reference does: per block the time conv, the residual conv and the LayerNorm,
then ``final_conv``.

``ASTGCN(..., backend="hip")`` runs the same parameter tree on the project's kernels (predictors/astgcn_hip.py, csrc/astgcn.hip) wherever those
serve the call; elsewhere the forward takes the torch modules.  ``backend_used`` records which of the two the last forward took.  As for the
other predictors, in eval mode the HIP path runs under ``no_grad`` and keeps nothing for a backward.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _backend


class _TemporalAttention(nn.Module):
    """E (B, T, T) = softmax over dim 1 of Ve sigmoid(((x^T U1) U2)(U3 x) + be)   (ASTGCN.py:134-163)"""

    def __init__(self, c_in, n, t):
        super().__init__()
        self.U1 = nn.Parameter(torch.empty(n))
        self.U2 = nn.Parameter(torch.empty(c_in, n))
        self.U3 = nn.Parameter(torch.empty(c_in))
        self.be = nn.Parameter(torch.empty(1, t, t))
        self.Ve = nn.Parameter(torch.empty(t, t))

    def forward(self, x):                                                  # x (B, N, F, T)
        lhs = torch.matmul(torch.matmul(x.permute(0, 3, 2, 1), self.U1), self.U2)      # (B, T, N)
        rhs = torch.matmul(self.U3, x)                                     # (B, N, T)
        e = torch.matmul(self.Ve, torch.sigmoid(torch.matmul(lhs, rhs) + self.be))
        return F.softmax(e, dim=1)


class _SpatialAttention(nn.Module):
    """S (B, N, N) = softmax over dim 1 of Vs sigmoid(((x W1) W2)(W3 x)^T + bs)   (ASTGCN.py:49-78)"""

    def __init__(self, c_in, n, t):
        super().__init__()
        self.W1 = nn.Parameter(torch.empty(t))
        self.W2 = nn.Parameter(torch.empty(c_in, t))
        self.W3 = nn.Parameter(torch.empty(c_in))
        self.bs = nn.Parameter(torch.empty(1, n, n))
        self.Vs = nn.Parameter(torch.empty(n, n))

    def forward(self, x):                                                  # x (B, N, F, T)
        lhs = torch.matmul(torch.matmul(x, self.W1), self.W2)              # (B, N, T)
        rhs = torch.matmul(self.W3, x).transpose(-1, -2)                   # (B, T, N)
        s = torch.matmul(self.Vs, torch.sigmoid(torch.matmul(lhs, rhs) + self.bs))
        return F.softmax(s, dim=1)


class _ChebConvSAt(nn.Module):
    """relu(sum_k (T_k * S_b)^T x theta_k) per time step   (ASTGCN.py:81-131)"""

    def __init__(self, k, c_in, c_out):
        super().__init__()
        self.Theta = nn.ParameterList([nn.Parameter(torch.empty(c_in, c_out)) for _ in range(k)])

    def forward(self, x, s, cheb):                                         # x (B, N, F, T), s (B, N, N), cheb (K, N, N)
        out = None
        for k, theta in enumerate(self.Theta):
            z = torch.einsum("bmn,bmft->bnft", cheb[k] * s, x)             # the masked polynomial, transposed, for all T at once
            y = torch.einsum("bnft,fo->bnot", z, theta)
            out = y if out is None else out + y
        return torch.relu(out)


class _Block(nn.Module):
    def __init__(self, c_in, k, c_cheb, c_time, time_strides, n, t):
        super().__init__()
        self.TAt = _TemporalAttention(c_in, n, t)
        self.SAt = _SpatialAttention(c_in, n, t)
        self.cheb_conv_SAt = _ChebConvSAt(k, c_in, c_cheb)
        self.time_conv = nn.Conv2d(c_cheb, c_time, kernel_size=(1, 3), stride=(1, time_strides), padding=(0, 1))
        self.residual_conv = nn.Conv2d(c_in, c_time, kernel_size=(1, 1), stride=(1, time_strides))
        self.ln = nn.LayerNorm(c_time)

    def forward(self, x, cheb):                                            # x (B, N, F, T)
        b, n, f, t = x.shape
        e = self.TAt(x)
        x_tat = torch.matmul(x.reshape(b, -1, t), e).reshape(b, n, f, t)
        s = self.SAt(x_tat)
        g = self.cheb_conv_SAt(x, s, cheb)                                 # on the plain x
        y = self.time_conv(g.permute(0, 2, 1, 3)) + self.residual_conv(x.permute(0, 2, 1, 3))      # (B, F, N, T)
        return self.ln(F.relu(y).permute(0, 3, 2, 1)).permute(0, 2, 3, 1)                          # LayerNorm over F; back to (B, N, F, T)


class ASTGCN(nn.Module):
    """``args``: nb_block, K, nb_chev_filter, nb_time_filter, time_strides, len_input, num_for_predict, num_nodes and G, the (K, N, N) Chebyshev
    polynomials of the scaled Laplacian (gptst_amd.graph.astgcn_graph) — the fields of reference ASTGCN.py:272-286.

    Takes (B, T, N, dim_in), returns (B, num_for_predict, N, dim_out).  The attention and Theta parameters are left uninitialised: see the
    module docstring."""

    def __init__(self, args, device, dim_in, dim_out, backend="torch"):
        super().__init__()
        self.backend, self.backend_used = _backend.check("ASTGCN", backend), None
        a = args
        self.num_for_predict, self.dim_out, self.time_strides = a.num_for_predict, dim_out, a.time_strides
        self.register_buffer("cheb", a.G[:a.K].to(torch.float32), persistent=False)
        t_out = a.len_input // a.time_strides
        self.BlockList = nn.ModuleList([_Block(dim_in, a.K, a.nb_chev_filter, a.nb_time_filter, a.time_strides, a.num_nodes, a.len_input)])
        self.BlockList.extend([_Block(a.nb_time_filter, a.K, a.nb_chev_filter, a.nb_time_filter, 1, a.num_nodes, t_out)
                               for _ in range(a.nb_block - 1)])
        self.final_conv = nn.Conv2d(int(a.len_input / a.time_strides), a.num_for_predict * dim_out, kernel_size=(1, a.nb_time_filter))
        self.to(device)

    def head(self, h):
        """h (B, T', N, F) -> (B, num_for_predict, N, dim_out): the reference's reshape and transpose (ASTGCN.py:309-311)"""
        return self.final_conv(h).reshape(h.shape[0], self.num_for_predict, self.dim_out, -1).transpose(-1, -2)

    def forward(self, x):                                                  # x (B, T, N, dim_in)
        y = _backend.hip_forward(self, "astgcn_hip", x)
        if y is not None:
            return y
        h = x.permute(0, 2, 3, 1)
        for blk in self.BlockList:
            h = blk(h, self.cheb)
        return self.head(h.permute(0, 3, 1, 2))
