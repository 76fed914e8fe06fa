"""What the DMVSTNET tests and the golden generator share (test_predictor_dmvstnet.py, test_dmvstnet_hip_cpu.py, test_gpu_dmvstnet_hip.py,
golden/make_golden_dmvstnet.py): the random graph, the argument set, the move away from the initialisation, and the explicit formulas of
the restated model (any dtype; the tests call them in float64): the LSTM with the head's columns applied to every step's h, and the
semantic view as a per-node thin projection, forward and backward — the two launches of csrc/dmvstnet.hip.  The LSTM's backward step is
stmgcn_util's, at one layer: the HIP backend runs ST-MGCN's launches there.

At the default initialisation the gates stay near 1/2 and exchanging two of them moves the output little; ``perturb_`` multiplies the two
LSTM matrices by 3, which spreads the four gates apart, and draws every Linear's bias anew so that no gradient is small by construction."""
from types import SimpleNamespace

import numpy as np
import torch

import stmgcn_util as su

SEED = 17


def adjacency(N, seed=SEED):
    """(N, N) fp32: dense, random, non-negative, not symmetric, row N - 1 all zero (a node that hears nobody); scaled so a row sums to about 1"""
    rng = np.random.RandomState(seed)
    a = rng.rand(N, N) * (2.0 / N)
    a[N - 1, :] = 0.0
    a = a.astype(np.float32)
    assert a[N - 1].sum() == 0 and (a[:N - 1] > 0).all()
    return a


def model_args(N, adj, T=12, hidden=32, topo=16):
    return SimpleNamespace(num_nodes=N, hidden_dim=hidden, topo_embedded_dim=topo, input_window=T, output_window=T, adj_mx=torch.as_tensor(adj))


def perturb_(model):
    """the two LSTM matrices times 3; the bias of every Linear that the forward reads and the four of the LSTM's drawn from 0.1 N(0, 1), from
    torch's global generator in a fixed order (works on the reference's model too: the attribute names are the same)"""
    with torch.no_grad():
        for k, p in model.lstm.named_parameters():
            if p.dim() == 2:
                p.mul_(3.0)
            else:
                p.copy_(0.1 * torch.randn(p.shape))
        for lin in (model.Lin_in_spa, model.Lin_in_tem, model.Lin_in_sen, model.Local_GNN1.lin, model.Lin_spa, model.output):
            lin.bias.copy_(0.1 * torch.randn(lin.bias.shape))
    return model


NO_GRAD_KEYS = ["Local_GNN2.lin.weight", "Local_GNN2.lin.bias", "Local_GNN3.lin.weight", "Local_GNN3.lin.bias"]


# ---- the LSTM with the thin head ------------------------------------------------------------------------------------------------------------
# Gx0 (T, rows, 4H) with both biases inside; Whh (4H, H); Wa (O, H).  Gate blocks in torch's order i, f, g, o.
def lstm_head_fwd(Gx0, Whh, Wa, order=(0, 1, 2, 3)):
    """-> (y (T, rows, O) = h_t Wa^T, gates (T, rows, 4H), c (T, rows, H), h (T + 1, rows, H) with slot 0 the zero state)"""
    T, rows, H4 = Gx0.shape
    H = H4 // 4
    gates, cs, hs = [], [], [Gx0.new_zeros(rows, H)]                       # (lists, then stacked: autograd can run through this one)
    for t in range(T):
        pre = hs[t] @ Whh.t() + Gx0[t]
        blk = [pre[:, k * H:(k + 1) * H] for k in order]
        i, f, g, o = torch.sigmoid(blk[0]), torch.sigmoid(blk[1]), torch.tanh(blk[2]), torch.sigmoid(blk[3])
        c = f * cs[t - 1] + i * g if t else i * g
        gates.append(torch.cat([i, f, g, o], dim=1))
        cs.append(c)
        hs.append(o * torch.tanh(c))
    hs = torch.stack(hs)
    return hs[1:] @ Wa.t(), torch.stack(gates), torch.stack(cs), hs


def lstm_head_bwd(dy, Whh, Wa, gates, cs):
    """dy (T, rows, O) -> dG (T, rows, 4H): dh_t = dy[t] Wa where the plain LSTM takes the gradient of its top ring"""
    return su.lstm_bwd(dy @ Wa, [Whh], gates[None], cs[None])[0]


def head_output(y, last=True):
    """top[t] = y_t + y_{T-1};  last = False drops the second term (a deliberately wrong model)"""
    return y + y[-1:] if last else y


# ---- the semantic view ------------------------------------------------------------------------------------------------------------------------
def sen_fwd(x, V, c, N):
    """x (units N, C), V (N, C, O), c (N, O) -> z (units N, O) = x[r] V[r mod N] + c[r mod N]"""
    xu = x.view(-1, N, x.shape[1])
    return (torch.einsum("unc,nco->uno", xu, V) + c).reshape(x.shape[0], -1)


def sen_bwd(x, V, dz, N):
    """-> (dx, dV, dc)"""
    xu, du = x.view(-1, N, x.shape[1]), dz.view(-1, N, dz.shape[1])
    return torch.einsum("uno,nco->unc", du, V).reshape(x.shape), torch.einsum("unc,uno->nco", xu, du), du.sum(0)


def sen_pack(model):
    """(V (N, C, O), c (N, O)) of a DMVSTNET module, written out the long way: the (N, h, h) generated weight first, as the model forms it"""
    Wn = torch.einsum("nd,dio->nio", model.node_embeddings, model.w)
    Wb = model.output.weight[:, model.lstm_dim:]
    V = torch.einsum("ic,nio,po->ncp", model.Lin_in_sen.weight, Wn, Wb)
    return V, torch.einsum("i,nio,po->np", model.Lin_in_sen.bias, Wn, Wb)


def restated(model, x, order=(0, 1, 2, 3), last=True):
    """the module's forward through the formulas above, time-major as the HIP backend runs it -> (out (B, T, N, O), parts)"""
    B, T, N, C = x.shape
    H = model.lstm_dim
    X = x.permute(1, 0, 2, 3).reshape(T * B * N, C)
    spa, tem = model.Lin_in_spa(X), model.Lin_in_tem(X)
    mixed = torch.einsum("vn,unc->uvc", model.adj_mx.to(x.dtype), spa.view(T * B, N, -1)).reshape(spa.shape)
    S = model.Lin_spa(torch.relu(model.Local_GNN1.lin(mixed))) + spa
    lstm = model.lstm
    Gx0 = (torch.cat([S, tem], 1) @ lstm.weight_ih_l0.t() + lstm.bias_ih_l0 + lstm.bias_hh_l0).view(T, B * N, 4 * H)
    y, gates, cs, hs = lstm_head_fwd(Gx0, lstm.weight_hh_l0, model.output.weight[:, :H], order)
    V, c = sen_pack(model)
    z = sen_fwd(X, V, c, N)
    out = head_output(y, last) + z.view(T, B * N, -1) + model.output.bias
    return out.view(T, B, N, -1).permute(1, 0, 2, 3), dict(Gx0=Gx0, y=y, gates=gates, c=cs, h=hs, V=V, cvec=c, z=z, X=X)


# ---- the inputs of the GPU launch tests ------------------------------------------------------------------------------------------------------
# (units, N, C): below one node tile; a tile plus one node; and one whose reduction loops all run more than once: 130 units are 44 splits of 3
# units (the sum over the splits, and the loop over a split's units, both longer than one), at C = 128 both 64-channel chunks are live
SEN_CASES = [(1, 5, 64), (3, 17, 16), (130, 17, 128)]
SEN_O = 2


def sen_inputs(units, N, C, O=SEN_O, dtype=torch.float64):
    """-> (x (units N, C), V (N, C, O), c (N, O), dz (units N, O))"""
    g = torch.Generator().manual_seed(units * 1000 + N * 10 + C)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                      # noqa: E731
    return r(units * N, C).to(dtype), (r(N, C, O) / C ** 0.5).to(dtype), r(N, O).to(dtype), r(units * N, O).to(dtype)
