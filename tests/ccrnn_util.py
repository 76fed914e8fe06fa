"""What the CCRNN tests and the golden generator share (test_predictor_ccrnn.py, test_ccrnn_hip_cpu.py, test_gpu_ccrnn_hip.py,
golden/make_golden_ccrnn.py): the support, the argument set, the move away from the initialisation, the series the support test is made from,
and the explicit formulas of the step launches of csrc/ccrnn.hip (any dtype; the tests call them in float64).

At the initialisation ``w1, w2`` are the identity and ``b1, b2`` zero, so the three graphs coincide, every graph-conv bias is small and the
``attlinear`` logits nearly agree; ``perturb_`` moves all of them so that no gradient is small by construction."""
from types import SimpleNamespace

import numpy as np
import torch

SEED = 17
TF_SEED = 3                      # ``random.seed`` of the teacher-forced golden runs
LAYERS = [(1, 1), (2, 1), (1, 3)]            # (n_rnn_layers, n_gconv_layers) of the golden cases; the last is the torch-only attention path


def support(N, seed=SEED):
    """-> (N, N) fp32: a random-walk matrix (rows sum to 1, zero diagonal) of a dense positive graph, the kind graph.ccrnn_support returns"""
    rng = np.random.RandomState(seed + N)
    a = rng.rand(N, N) ** 3 + 0.01
    np.fill_diagonal(a, 0.0)
    return (a / a.sum(1, keepdims=True)).astype(np.float32)


def model_args(N, sup, H=25, n_dim=10, k_hop=3, rnn=1, gconv=1, P=12, n_supports=1):
    return SimpleNamespace(num_predict=P, hidden_size=H, num_nodes=N, n_dim=n_dim, n_supports=n_supports, k_hop=k_hop, n_rnn_layers=rnn,
                           n_gconv_layers=gconv, cl_decay_steps=300, support=torch.as_tensor(sup, dtype=torch.float32))


def perturb_(model, vec=0.05):
    """in ``named_parameters`` order, from torch's global generator: the node vectors plus ``vec`` N(0, 1), w1, w2 plus 0.05 N(0, 1); b1, b2 0.02 N(0, 1), every bias
    0.1 N(0, 1); every graph-conv weight times 2; every attlinear weight 0.1 N(0, 1).  Works on the reference's model too: same names.
    ``vec``: the noise n1 n2 on graph0 has entries of size vec^2 sqrt(n_dim) whose positive half survives the leaky ReLU, a row sum of about
    0.4 vec^2 sqrt(n_dim) N on top of the support's 1: 0.06 at the golden N = 20, n_dim = 10, but 1.9 at N = 266, n_dim = 50, where T_3 of
    a spectral radius near 3 is 99 and 24 steps of it are chaotic (the fp32 torch backend itself then differs from fp64 by more than 1).
    The tests at the shipped sizes pass vec = 0.004: 0.012 on the row sum"""
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k in ("nodevec1", "nodevec2", "w1", "w2"):
                p.add_((vec if k.startswith("nodevec") else 0.05) * torch.randn(p.shape))
            elif k in ("b1", "b2"):                                        # (small: b b^T enters every entry of graph1 and graph2, whose powers the cells take)
                p.copy_(0.02 * torch.randn(p.shape))
            elif k.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape))
            elif "attlinear" in k:
                p.copy_(0.1 * torch.randn(p.shape))
            else:
                p.mul_(2.0)
    return model


def tag(rnn, gconv):
    return "L%d%d" % (rnn, gconv)


def series(T=60, N=20, seed=SEED):
    """-> (pick, drop) (T, N) fp64 counts-like arrays for the support test: a few latent daily profiles mixed per node, plus noise"""
    rng = np.random.RandomState(seed)
    t = np.arange(T)[:, None]
    base = np.stack([np.sin(2 * np.pi * t[:, 0] / p) + 1.2 for p in (12, 7, 30)], 1)          # (T, 3)
    mix = rng.rand(2, 3, N)
    out = [np.floor(20 * base @ mix[c] + 3 * rng.rand(T, N)) for c in range(2)]
    return out[0], out[1]


SUPPORT_CASE = dict(hidden_size_data=6, holdout=10)


# ---- the cell of csrc/ccrnn.hip, step by step ---------------------------------------------------------------------------------------------
# P (k, N, N) = [T_1(S) .. T_k(S)];  z (B, N, C) -> [z | P_1 z | .. | P_k z] (B, N, (k + 1) C), matrix-major: the kernels' column order
def poly_stack(S, k):
    """[T_1(S), .., T_k(S)] by the recursion T_j = 2 S T_{j-1} - T_{j-2} on matrices"""
    eye = torch.eye(S.shape[0], dtype=S.dtype, device=S.device)
    Ts = [eye, S]
    for _ in range(2, k + 1):
        Ts.append(2 * S @ Ts[-1] - Ts[-2])
    return torch.stack(Ts[1:k + 1], 0)


def mix(P, z):
    return torch.cat([z] + [torch.einsum("vw,bwc->bvc", Pj, z) for Pj in P], dim=-1)


def cell_fwd(P, Wru, bru, Wc, bc, x, h):
    """one DCGRUCell with matrix-major weights: Wru (2H, (k + 1)(C + H)), Wc (H, (k + 1)(C + H)) over mix([x, h]) -> (h', r, u, c)"""
    H = h.shape[-1]
    ru = torch.sigmoid(mix(P, torch.cat([x, h], -1)) @ Wru.t() + bru)
    r, u = ru[..., :H], ru[..., H:]
    c = torch.tanh(mix(P, torch.cat([x, r * h], -1)) @ Wc.t() + bc)
    return u * h + (1 - u) * c, r, u, c


def matrix_major(W, C, M):
    """a GraphConv Linear weight (out, C * M), columns c * M + m -> columns m * C + c"""
    return W.reshape(W.shape[0], C, M).transpose(1, 2).reshape(W.shape[0], M * C)


# ---- the launches of predictors/ccrnn_hip.py restated in torch, with the signatures of their ``ops`` wrappers (any device, any dtype) -----------
# test_ccrnn_hip_cpu.py runs the whole HIP path's Python on them in float64; test_gpu_ccrnn_hip.py holds every real launch to them.
def _mixed(P, zz, B, N):
    """zz (B N, Ks) -> [zz | P_j zz]_j (B N, (k + 1) Ks); P (k, Np, Np) zero-padded"""
    z3 = zz.view(B, N, -1)
    return torch.cat([z3] + [torch.einsum("vw,bwc->bvc", Pj[:N, :N], z3) for Pj in P], dim=-1).reshape(B * N, -1)


def _at(seq, t, B, T, N):
    """the (B N, width) rows of step t of a seq tensor (a view)"""
    return seq.view(B, T, N, -1)[:, t]


def ref_fwd_gates(P, W0, h, g, t, u, q, B, T, N, inp=None, fb=None, inp_out=None, r=None, z=None, tiles=0):
    Hp = h.shape[1]
    if fb is not None:
        inp = fb[0] @ fb[1].t() + fb[2]
        inp_out.copy_(inp)
    M = _mixed(P, h if inp is None else torch.cat([h, inp], 1), B, N)
    s = torch.sigmoid(M @ W0.t() + (_at(g, t, B, T, N).reshape(B * N, -1) if g.dim() == 2 else g))
    u.copy_(s[:, Hp:])
    q.copy_(s[:, :Hp] * h)
    if r is not None:
        r.copy_(s[:, :Hp])
    if z is not None:
        _at(z, t, B, T, N).copy_(M.view(B, N, -1))


def ref_fwd_state(P, W1, q, g, t, u, h, h_out, B, T, N, inp=None, c=None, z=None, tiles=0):
    M = _mixed(P, q if inp is None else torch.cat([q, inp], 1), B, N)
    cc = torch.tanh(M @ W1.t() + (_at(g, t, B, T, N).reshape(B * N, -1) if g.dim() == 2 else g))
    h_out.copy_(u * h + (1 - u) * cc)
    if c is not None:
        c.copy_(cc)
    if z is not None:
        _at(z, t, B, T, N).copy_(M.view(B, N, -1))


def ref_bwd_cand(PT, W1T, dh, u, c, r, h, t, dpre1, dpre0, dh_part, B, T, N, dh2=None, dinp=None, tiles=0):
    Hp = h.shape[1]
    d = dh if dh2 is None else dh + dh2
    d1 = d * (1 - u) * (1 - c * c)
    _at(dpre1, t, B, T, N).copy_(d1.view(B, N, -1))
    out = _mixed(PT, d1, B, N) @ W1T.t()
    dq = out[:, :Hp]
    _at(dpre0, t, B, T, N).copy_(torch.cat([dq * h * r * (1 - r), d * (h - c) * u * (1 - u)], 1).view(B, N, -1))
    dh_part.copy_(d * u + dq * r)
    if dinp is not None:
        dinp.copy_(out[:, Hp:])


def ref_bwd_state(PT, W0T, dpre0, dh_part, t, dh_out, B, T, N, dinp=None, tiles=0):
    Hp = dh_part.shape[1]
    out = _mixed(PT, _at(dpre0, t, B, T, N).reshape(B * N, -1), B, N) @ W0T.t()
    dh_out.copy_(dh_part + out[:, :Hp])
    if dinp is not None:
        dinp.add_(out[:, Hp:])


def ref_nodemix(Lp, In, N, c, reduce, res=None):
    x = In.view(-1, N, In.shape[1])
    L = Lp[:, :N, :N]
    if not reduce:
        return torch.cat([torch.einsum("vw,uwc->uvc", Lk, x) for Lk in L], -1).reshape(In.shape[0], -1)
    out = sum(torch.einsum("vw,uwc->uvc", Lk, x[..., k * c:(k + 1) * c]) for k, Lk in enumerate(L)).reshape(In.shape[0], c)
    return out if res is None else out + res


def ref_tapgemm(X, W, bias, taps, act, T, N, res=None, res_w=0, keep=False):
    assert tuple(taps) == (0,) and act == 0 and not keep
    Y = X @ W.t()
    if bias is not None:
        Y = Y + bias
    if res is not None and res_w:
        Y[:, :res_w] += res[:, :res_w]
    return Y


def ref_wgrad(D, X, taps, T, N, want_bias=True):
    assert tuple(taps) == (0,)
    return D.t() @ X, (D.sum(0) if want_bias else None)


def ref_graphgrad(D, X, N, c, ks, dcol0=0):
    d, x = D.view(-1, N, D.shape[1]), X[:, :c].reshape(-1, N, c)                # (X may be wider than c: its first c columns)
    return torch.stack([torch.einsum("uvc,uwc->vw", d[..., dcol0 + k * c:dcol0 + (k + 1) * c], x) for k in range(ks)], 0)


REF_OPS = dict(ccrnn_fwd_gates=ref_fwd_gates, ccrnn_fwd_state=ref_fwd_state, ccrnn_bwd_cand=ref_bwd_cand, ccrnn_bwd_state=ref_bwd_state,
               stgcn_nodemix=ref_nodemix, stgcn_tapgemm=ref_tapgemm, stgcn_wgrad=ref_wgrad, mtgnn_graphgrad=ref_graphgrad)
