"""What the ST-MGCN tests and the golden generator share (test_predictor_stmgcn.py, test_stmgcn_hip_cpu.py, test_gpu_stmgcn_hip.py,
golden/make_golden_stmgcn.py): the two random graphs, the argument set, the move away from the initialisation, and the explicit per-step
formulas of the two LSTM launches of csrc/stmgcn.hip (any dtype; the tests call them in float64).

At the default initialisation (uniform in +-1/8 at H = 64) the gates stay near 1/2 and exchanging two of them moves the output little;
``perturb_`` multiplies every 2-D LSTM weight by 3, which spreads the four gates apart, and moves the biases of the graph convolutions (0 at
the initialisation) and of the Linears so that no gradient is small by construction."""
from types import SimpleNamespace

import numpy as np
import torch

SEED = 13


def graphs(N, seed=SEED):
    """-> (dis, pcc) (N, N) fp32.  dis: symmetric, non-negative, node N - 1 isolated (row sum 0: the inf of ``rowsum ** -0.5``); pcc:
    symmetric with entries in (-1, 1), unit diagonal, node 0 with a negative row sum (the NaN of it)"""
    rng = np.random.RandomState(seed)
    d = rng.rand(N, N) * (rng.rand(N, N) < 0.4)
    d = np.maximum(d, d.T)
    d[np.arange(N - 1), (np.arange(N - 1) + 1) % (N - 1)] = 0.5                # a ring over the first N - 1 nodes: none of them is isolated
    d = np.maximum(d, d.T)
    np.fill_diagonal(d, 0.0)
    d[N - 1, :] = 0.0
    d[:, N - 1] = 0.0
    p = rng.rand(N, N) * 0.8 - 0.1
    p = (p + p.T) / 2
    p[0, 1:] = -np.abs(p[0, 1:]) - 0.2
    p[1:, 0] = p[0, 1:]
    np.fill_diagonal(p, 1.0)
    d, p = d.astype(np.float32), p.astype(np.float32)
    assert d[N - 1].sum() == 0 and (d[:N - 1].sum(1) > 0).all() and p[0].sum() < 0 and (p[1:].sum(1) > 0).all()
    return d, p


def model_args(N, dis, pcc, T=12, H=64, L=3, G=64, bias=True):
    """dis, pcc: the (3, N, N) support stacks"""
    return SimpleNamespace(seq_len=T, M=2, n_nodes=N, lstm_hidden_dim=H, lstm_num_layers=L, gcn_hidden_dim=G, gconv_use_bias=bias,
                           gconv_activation="nn.ReLU", dis_graph=dis, pcc_graph=pcc)


def perturb_(model):
    """every 2-D LSTM weight times 3; the GCN biases and the biases of every ``fc`` drawn from 0.1 N(0, 1), from torch's global generator
    in the order of the modules (works on the reference's model too: the attribute names are the same)"""
    with torch.no_grad():
        for m in range(len(model.rnn_list)):
            r = model.rnn_list[m]
            for k, p in r.lstm.named_parameters():
                if p.dim() == 2:
                    p.mul_(3.0)
            for b in (r.gconv_temporal_feats.b, r.fc.bias, model.gcn_list[m].b):
                b.copy_(0.1 * torch.randn(b.shape))
        model.fc.bias.copy_(0.1 * torch.randn(model.fc.bias.shape))
    return model


# ---- the two launches, step by step -----------------------------------------------------------------------------------------------------
# Gx0 (T, rows, 4H) = the input half of layer 0 with both of its biases;  W[0] = W_hh0 (4H, H), W[l] = [W_ih_l | W_hh_l] (4H, 2H);
# b[l] (4H) = b_ih_l + b_hh_l (b[0] is not read: it is inside Gx0).  Gate blocks in torch's order i, f, g, o.
def lstm_fwd(Gx0, W, b, order=(0, 1, 2, 3)):
    """-> (top (T, rows, H), gates (L, T, rows, 4H) activated, c (L, T, rows, H), h (L, T + 1, rows, H) with slot 0 the zero state).
    ``order``: which block of the pre-activation plays i, f, g, o — anything but (0, 1, 2, 3) is a deliberately wrong kernel"""
    T, rows, H4 = Gx0.shape
    H, L = H4 // 4, len(W)
    gates, cs, hs = Gx0.new_zeros(L, T, rows, H4), Gx0.new_zeros(L, T, rows, H), Gx0.new_zeros(L, T + 1, rows, H)
    for t in range(T):
        for l in range(L):
            if l == 0:
                pre = hs[0, t] @ W[0].t() + Gx0[t]
            else:
                pre = torch.cat([hs[l - 1, t + 1], hs[l, t]], dim=1) @ W[l].t() + b[l]
            blk = [pre[:, k * H:(k + 1) * H] for k in order]
            i, f, g, o = torch.sigmoid(blk[0]), torch.sigmoid(blk[1]), torch.tanh(blk[2]), torch.sigmoid(blk[3])
            c = f * (cs[l, t - 1] if t else 0) + i * g
            gates[l, t], cs[l, t], hs[l, t + 1] = torch.cat([i, f, g, o], dim=1), c, o * torch.tanh(c)
    return hs[L - 1, 1:], gates, cs, hs


def lstm_bwd(dTop, W, gates, cs):
    """dTop (T, rows, H): the gradient of every step of the top ring -> dG (L, T, rows, 4H), the gradient of every pre-activation
    (dG[0] is dGx0)"""
    L, T, rows, H4 = gates.shape
    H = H4 // 4
    dG = torch.zeros_like(gates)
    dh_carry, dc_carry = [dTop.new_zeros(rows, H) for _ in range(L)], [dTop.new_zeros(rows, H) for _ in range(L)]
    for t in reversed(range(T)):
        dx = None
        for l in reversed(range(L)):
            dh = (dTop[t] if l == L - 1 else dx) + dh_carry[l]
            i, f, g, o = (gates[l, t][:, k * H:(k + 1) * H] for k in range(4))
            tc = torch.tanh(cs[l, t])
            dc = dh * o * (1 - tc * tc) + dc_carry[l]
            cp = cs[l, t - 1] if t else torch.zeros_like(tc)
            dG[l, t] = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], dim=1)
            dc_carry[l] = dc * f
            back = dG[l, t] @ W[l]                                         # [dx | dh_prev] (layer 0: dh_prev alone)
            if l:
                dx, dh_carry[l] = back[:, :H], back[:, H:]
            else:
                dh_carry[l] = back
    return dG


def lstm_operands(lstm):
    """(W, b) of an ``nn.LSTM`` in the form above, and (W_ih0, b_0) of the hoisted input half"""
    L = lstm.num_layers
    g = lambda n, l: getattr(lstm, "%s_l%d" % (n, l))                      # noqa: E731
    W = [g("weight_hh", 0)] + [torch.cat([g("weight_ih", l), g("weight_hh", l)], dim=1) for l in range(1, L)]
    b = [g("bias_ih", l) + g("bias_hh", l) for l in range(L)]
    return W, b, g("weight_ih", 0)


# ---- the inputs of the GPU launch tests (rows, T, L, H); test_stmgcn_hip_cpu.py shows that they tell a wrong kernel from a right one ------------
LAUNCH_CASES = [(40, 2, 1, 64), (111, 12, 3, 64), (16, 1, 2, 16), (48, 3, 3, 48), (33, 2, 2, 128), (64, 32, 1, 32), (32, 2, 4, 64)]


def launch_inputs(rows, T, L, H, dtype=torch.float64, last_only=False):
    """-> (Gx0, W list, b list, dTop): an LSTM of ``nn.LSTM``'s own initialisation with its 2-D weights times 3, unit-normal input rows"""
    g = torch.Generator().manual_seed(rows * 1000 + T * 100 + L * 10 + H)
    k = 3.0 / H ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k      # noqa: E731
    W = [u(4 * H, H)] + [u(4 * H, 2 * H) for _ in range(1, L)]
    b = [u(4 * H) / 3 * 2 for _ in range(L)]
    Gx0 = torch.randn(T, rows, 4 * H, generator=g, dtype=torch.float64)
    dTop = torch.randn(T, rows, H, generator=g, dtype=torch.float64)
    if last_only:
        dTop[:T - 1] = 0
    return Gx0.to(dtype), [w.to(dtype) for w in W], [v.to(dtype) for v in b], dTop.to(dtype)
