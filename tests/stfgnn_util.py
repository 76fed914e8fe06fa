"""Shared by the STFGNN golden generator and the STFGNN tests: the graphs and argument set the vectors are made with, the block algebra of the
fusion graph in plain torch (what predictors/stfgnn_hip.py computes, launch by launch), and the recording of a layer's max candidates.  The
near-tie condition is stsgcn_util's (GAP, ambiguous)."""
import contextlib
import types

import numpy as np
import torch

import stsgcn_util as su
from stsgcn_util import GAP, ambiguous                                     # noqa: F401
from gptst_amd import graph


def graphs(n, seed=11):
    """(S, D): two different non-symmetric row-normalised graphs; S with a zero diagonal (the fusion graph forces it to 1), D with a unit
    diagonal, as ``graph.dtw_graph`` always gives (D itself is symmetric there; the form ``graph.stfgnn_blocks`` recognises does not need it)"""
    S, D = su.adjacency(n, seed), su.adjacency(n, seed + 100).copy()
    np.fill_diagonal(D, 1.0)
    assert np.abs(S - S.T).max() > 1e-2 and np.abs(D - D.T).max() > 1e-2 and np.abs(S - D).max() > 1e-2
    return S, D


def model_args(n, adj=None, T=9, P=3, width=16, layers=2, activation="GLU", hidden_dims=None, **kw):
    d = dict(num_nodes=n, window=T, horizon=P, hidden_dims=[[width] * 3 for _ in range(layers)] if hidden_dims is None else hidden_dims,
             first_layer_embedding_size=width, out_layer_dim=32, output_dim=1, strides=4, temporal_emb=True, spatial_emb=True, use_mask=False,
             activation=activation, adj=graph.stfgnn_fusion_graph(*graphs(n)) if adj is None else adj)
    d.update(kw)
    return types.SimpleNamespace(**d)


def randomize_embeddings_(model, scale=0.3):
    """the position embeddings are drawn with gain 0.0003: that small they hide an omitted add"""
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("temporal_embedding") or k.endswith("spatial_embedding"):
                p.copy_(torch.randn(p.shape, dtype=p.dtype) * scale)


# ---- the block algebra on blocks (..., 4, N, C):  mix(X)_0 = mix(X)_3 = D (X_0 + X_3) + X_1 + X_2,  mix(X)_k = S^ X_k + the other three, k = 1, 2 ----
def mix_expanded(S, D, X):
    tot = X.sum(-3)
    outer = D @ (X[..., 0, :, :] + X[..., 3, :, :]) + X[..., 1, :, :] + X[..., 2, :, :]
    return torch.stack([outer, S @ X[..., 1, :, :] + tot - X[..., 1, :, :], S @ X[..., 2, :, :] + tot - X[..., 2, :, :], outer], -3)


def mix_middle(S, X):
    return S @ X[..., 1, :, :] + X[..., 0, :, :] + X[..., 2, :, :] + X[..., 3, :, :]


def expand(H):
    """frames (B, T, N, C) -> window-expanded (B, W, 4, N, C): block (w, k) is frame w + k"""
    return torch.stack([H[:, w:w + 4] for w in range(H.shape[1] - 3)], 1)


def fold(G):
    """the adjoint of ``expand``: (B, W, 4, N, C) -> (B, W + 3, N, C)"""
    B, W = G.shape[:2]
    out = G.new_zeros(B, W + 3, *G.shape[3:])
    for k in range(4):
        out[:, k:k + W] += G[:, :, k]
    return out


def mix_f2e(S, D, H):
    return mix_expanded(S, D, expand(H))


def mix_m2e(St, g):
    """the adjoint of ``mix_middle``, St = S^^T: block 1 = S^T g, blocks 0, 2 and 3 = g unmixed"""
    return torch.stack([g, St @ g, g, g], -3)


# frame t takes block (t - s, k) unmixed, in this order (csrc/stfgnn.hip keeps the same one)
E2F_IDENTITY = ((0, 1), (3, 1), (0, 2), (3, 2), (1, 0), (1, 2), (1, 3), (2, 0), (2, 1), (2, 3))          # (k, s)


def mix_e2f(St, Dt, G):
    """the adjoint of ``mix_f2e`` as csrc/stfgnn.hip forms it: frame t gathers the blocks (t - 1, 1), (t - 2, 2) before the product with S^T,
    the blocks (t, 0), (t, 3), (t - 3, 0), (t - 3, 3) before the product with D^T, and takes up to ten blocks unmixed"""
    B, W = G.shape[:2]
    gs, gd = G.new_zeros(B, W + 3, *G.shape[3:]), G.new_zeros(B, W + 3, *G.shape[3:])
    gs[:, 1:1 + W] += G[:, :, 1]
    gs[:, 2:2 + W] += G[:, :, 2]
    for s in (0, 3):
        gd[:, s:s + W] += G[:, :, 0]
        gd[:, s:s + W] += G[:, :, 3]
    out = St @ gs + Dt @ gd
    for k, s in E2F_IDENTITY:
        out[:, s:s + W] += G[:, :, k]
    return out


def gate_weight(lay):
    """(W (2 co, 2 ci) tap-major, b (2 co)) of the gated branch as one tap GEMM with offsets (0, 3): conv2's rows (tanh), then conv1's (sigmoid)"""
    w = torch.cat([lay.conv2.weight, lay.conv1.weight])[:, :, 0, :].permute(0, 2, 1)
    return w.reshape(w.shape[0], -1), torch.cat([lay.conv2.bias, lay.conv1.bias])


def gate_manual(lay, H, dG):
    """the gated branch launch by launch: tap GEMM with offsets (0, 3), tanh(P) sigmoid(Q); backward: dPre, dW / db of the stacked weight, the
    mirrored tap GEMM -> (g, dH, dconv1.weight, dconv1.bias, dconv2.weight, dconv2.bias)"""
    Wg, bg = (t.detach() for t in gate_weight(lay))
    B, T, N, ci = H.shape
    co = Wg.shape[0] // 2
    X = torch.cat([H[:, :T - 3], H[:, 3:]], -1)                           # (B, T - 3, N, 2 ci): the two taps side by side
    pre = X @ Wg.t() + bg
    tn, s = torch.tanh(pre[..., :co]), torch.sigmoid(pre[..., co:])
    g = tn * s
    dPre = torch.cat([dG * s * (1 - tn * tn), dG * tn * s * (1 - s)], -1)
    dW = torch.einsum("btno,btni->oi", dPre, X).reshape(2 * co, 2, ci).permute(0, 2, 1)[:, :, None, :]        # (2 co, ci, 1, 2)
    db = dPre.sum((0, 1, 2))
    dX = dPre @ Wg
    dH = torch.zeros_like(H)
    dH[:, :T - 3] += dX[..., :ci]
    dH[:, 3:] += dX[..., ci:]
    return g, dH, dW[co:], db[co:], dW[:co], db[:co]


def layer_manual(lay, S, D, H, dBest):
    """the window branch of one layer (H: embeddings added) launch by launch as predictors/windows_hip.LayerFn runs it, forward and the
    hand-written backward -> (best, which, dH, [dW_j], [db_j]) with dW_j (W, cw, ci) per window"""
    J, saved = len(lay.out_dims), []
    cur, best, which = H, None, None
    for j, co in enumerate(lay.out_dims):
        wt, bs = (t.detach() for t in lay.stacked(j))
        last = j == J - 1
        Z = mix_f2e(S, D, cur) if j == 0 else mix_middle(S, cur) if last else mix_expanded(S, D, cur)
        pre = Z @ (wt if last else wt[:, None]).transpose(-1, -2) + (bs[:, None, :] if last else bs[:, None, None, :])
        A, Sg = pre[..., :co], torch.sigmoid(pre[..., co:])
        cur = A * Sg
        midv = cur if last else cur[:, :, 1]
        if j == 0:
            best, which = midv.clone(), torch.zeros_like(midv, dtype=torch.int32)
        else:
            win = midv > best                                              # an exact tie keeps the earlier operation
            best, which = torch.where(win, midv, best), torch.where(win, torch.full_like(which, j), which)
        saved.append((Z, Sg, A, wt))
    St, Dt, up, dWs, dbs = S.t(), D.t(), None, [None] * J, [None] * J
    for j in range(J - 1, -1, -1):
        Z, Sg, A, wt = saved[j]
        last = j == J - 1
        routed = dBest * (which == j)
        if last:
            g = routed
        else:
            g = up.clone()
            g[:, :, 1] += routed
        dPre = torch.cat([g * Sg, g * A * Sg * (1 - Sg)], -1)
        dWs[j] = torch.einsum("bw...o,bw...i->woi", dPre, Z)
        dbs[j] = dPre.sum(dim=(0, 2) if last else (0, 2, 3))
        dZ = dPre @ (wt if last else wt[:, None])
        up = mix_e2f(St, Dt, dZ) if j == 0 else mix_m2e(St, dZ) if last else mix_expanded(St, Dt, dZ)
    return best, which, up, dWs, dbs


def layer_blocks(lay, S, D, H):
    """one layer of the model on the block algebra, from its stacked weights -> (output (B, W, N, co), candidates (J, B, W, N, co))"""
    x = lay.embed(H)
    cur = expand(x)
    J, cands = len(lay.out_dims), []
    for j, co in enumerate(lay.out_dims):
        wt, bs = lay.stacked(j)                                           # (W, cw, ci)
        z = mix_middle(S, cur) if j == J - 1 else mix_expanded(S, D, cur)
        wt = wt if z.dim() == 4 else wt[:, None]
        bs = bs[:, None, :] if z.dim() == 4 else bs[:, None, None, :]
        pre = z @ wt.transpose(-1, -2) + bs
        cur = pre[..., :co] * torch.sigmoid(pre[..., co:])
        cands.append(cur if j == J - 1 else cur[:, :, 1])
    cands = torch.stack(cands)
    Wg, bg = gate_weight(lay)
    T = x.shape[1]
    pre = torch.cat([x[:, :T - 3], x[:, 3:]], -1) @ Wg.t() + bg
    co = Wg.shape[0] // 2
    return cands.max(0)[0] + torch.tanh(pre[..., :co]) * torch.sigmoid(pre[..., co:]), cands


def model_blocks(m, x):
    """the whole model on the block algebra: embedding, the layers above, the stacked heads"""
    h = torch.relu(m.First_FC(x))
    for lay in m.STSGCLS:
        h, _ = layer_blocks(lay, m.s_hat, m.d_hat, h)
    return m.head(h)


@contextlib.contextmanager
def recorded_candidates(model, into):
    """every layer's candidates (J, B, W, N, co) of the forwards inside are appended to ``into``: taken where the layer stacks the outputs of its
    operations (the torch backend runs the windows of a layer batched)"""
    real = {}
    for i, lay in enumerate(model.STSGCLS):
        real[i] = lay.candidates

        def spy(x, adj, f=real[i]):
            c = f(x, adj)
            into.append(c.detach())
            return c
        lay.candidates = spy
    try:
        yield into
    finally:
        for lay in model.STSGCLS:
            del lay.candidates
