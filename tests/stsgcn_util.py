"""Shared by the STSGCN golden generator and the STSGCN tests: the adjacency and argument set the vectors are made with, the block algebra of
the localized adjacency in plain torch (what predictors/stsgcn_hip.py computes, launch by launch), and the near-tie condition on the max."""
import contextlib
import types

import numpy as np
import torch


def adjacency(n, seed=11):
    """non-symmetric, zero diagonal, rows normalised to sum 1: with an un-normalised one the activations of a deep model blow up"""
    rng = np.random.RandomState(seed)
    A = (rng.rand(n, n) < 0.2).astype(np.float64) * rng.rand(n, n)
    np.fill_diagonal(A, 0)
    A[np.arange(n), (np.arange(n) + 1) % n] += 0.5                       # connected ring underneath
    A = A / A.sum(1, keepdims=True)
    assert not np.allclose(A, A.T) and np.all(np.diag(A) == 0)
    return A.astype(np.float32)


def model_args(n, A=None, T=6, P=3, width=16, layers=2, module_type="individual", activation="GLU", filter_list=None, **kw):
    d = dict(num_nodes=n, feature_dim=64, input_window=T, output_window=P, rho=1, module_type=module_type, activation=activation,
             temporal_emb=True, spatial_emb=True, use_mask=False, steps=3, first_layer_embedding_size=width,
             filter_list=[[width] * 3 for _ in range(layers)] if filter_list is None else filter_list, A=adjacency(n) if A is None else A)
    d.update(kw)
    return types.SimpleNamespace(**d)


def randomize_embeddings_(model, scale=0.3):
    """the position embeddings are zeros at construction: at zero they hide an omitted add"""
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("temporal_emb") or k.endswith("spatial_emb"):
                p.copy_(torch.randn(p.shape, dtype=p.dtype) * scale)


# ---- the block algebra: mix(S)_k = A^ S_k + [k >= 1] S_{k-1} + [k <= 1] S_{k+1} on blocks (..., 3, N, C) ----
def mix_expanded(a_hat, S):
    out = a_hat @ S
    out[..., 1:, :, :] += S[..., :-1, :, :]
    out[..., :-1, :, :] += S[..., 1:, :, :]
    return out


def mix_middle(a_hat, S):
    return a_hat @ S[..., 1, :, :] + S[..., 0, :, :] + S[..., 2, :, :]


def expand(H):
    """frames (B, T, N, C) -> window-expanded (B, W, 3, N, C): block (w, k) is frame w + k"""
    return torch.stack([H[:, w:w + 3] for w in range(H.shape[1] - 2)], 1)


def fold(G):
    """the adjoint of ``expand``: (B, W, 3, N, C) -> (B, W + 2, N, C), frame t sums the blocks with w + k = t in the order k = 0, 1, 2"""
    B, W = G.shape[:2]
    out = G.new_zeros(B, W + 2, *G.shape[3:])
    for k in range(3):
        out[:, k:k + W] += G[:, :, k]
    return out


def mix_f2e(a_hat, H):
    return mix_expanded(a_hat, expand(H))


def mix_m2e(a_t, g):
    """the adjoint of ``mix_middle``, a_t = A^^T: block 1 = A^T g, blocks 0 and 2 = g unmixed"""
    return torch.stack([g, a_t @ g, g], -3)


def mix_e2f(a_t, G):
    """the adjoint of ``mix_f2e`` as csrc/stsgcn.hip forms it: frame t gathers the blocks with w + k = t before the product with A^T, and
    takes its neighbour terms — the blocks (t, 1), (t - 1, 2), (t - 1, 0), (t - 2, 1) — after it"""
    W = G.shape[1]
    out = a_t @ fold(G)
    for k, dw in ((1, 0), (2, -1), (0, -1), (1, -2)):
        out[:, -dw:W - dw] += G[:, :, k]
    return out


def layer_manual(lay, a_hat, H, dBest):
    """one layer (H: embeddings added) launch by launch as predictors/windows_hip.LayerFn runs it, forward and the hand-written backward
    -> (best, which, dH, [dW_j], [db_j]) with dW_j (W, cw, ci) per window"""
    J, saved = len(lay.filters), []
    cur, best, which = H, None, None
    for j, co in enumerate(lay.filters):
        wt, bs = (t.detach() for t in lay.stacked(j))
        last = j == J - 1
        Z = mix_f2e(a_hat, cur) if j == 0 else mix_middle(a_hat, cur) if last else mix_expanded(a_hat, cur)
        pre = Z @ (wt if last else wt[:, None]).transpose(-1, -2) + (bs[:, None, :] if last else bs[:, None, None, :])
        A, S = pre[..., :co], torch.sigmoid(pre[..., co:])
        cur = A * S
        midv = cur if last else cur[:, :, 1]
        if j == 0:
            best, which = midv.clone(), torch.zeros_like(midv, dtype=torch.int32)
        else:
            win = midv > best                                              # an exact tie keeps the earlier operation
            best, which = torch.where(win, midv, best), torch.where(win, torch.full_like(which, j), which)
        saved.append((Z, S, A, wt))
    a_t, up, dWs, dbs = a_hat.t(), None, [None] * J, [None] * J
    for j in range(J - 1, -1, -1):
        Z, S, A, wt = saved[j]
        last = j == J - 1
        routed = dBest * (which == j)
        if last:
            g = routed
        else:
            g = up.clone()
            g[:, :, 1] += routed
        dPre = torch.cat([g * S, g * A * S * (1 - S)], -1)
        dWs[j] = torch.einsum("bw...o,bw...i->woi", dPre, Z)
        dbs[j] = dPre.sum(dim=(0, 2) if last else (0, 2, 3))
        dZ = dPre @ (wt if last else wt[:, None])
        up = mix_e2f(a_t, dZ) if j == 0 else mix_m2e(a_t, dZ) if last else mix_expanded(a_t, dZ)
    return best, which, up, dWs, dbs


def layer_blocks(lay, a_hat, H):
    """one layer of the model on the block algebra, from its stacked weights -> (best (B, W, N, co), candidates (J, B, W, N, co))"""
    cur = expand(lay.position_embedding(H))
    J, cands = len(lay.filters), []
    for j, co in enumerate(lay.filters):
        wt, bs = lay.stacked(j)                                           # (W | 1, cw, ci)
        z = mix_middle(a_hat, cur) if j == J - 1 else mix_expanded(a_hat, cur)
        wt = wt if z.dim() == 4 else wt[:, None]                          # batch dimension W (or 1: sharing) against (B, W[, 3])
        bs = bs[:, None, :] if z.dim() == 4 else bs[:, None, None, :]
        pre = z @ wt.transpose(-1, -2) + bs
        cur = pre[..., :co] * torch.sigmoid(pre[..., co:])
        cands.append(cur if j == J - 1 else cur[:, :, 1])
    cands = torch.stack(cands)
    return cands.max(0)[0], cands


def model_blocks(m, x):
    """the whole model on the block algebra: embedding, the layers above, the stacked heads"""
    h = torch.relu(m.first_layer_embedding(x))
    for lay in m.stsgcl_layers:
        h, _ = layer_blocks(lay.layer, m.a_hat, h)
    return m.head(h)


# ---- the max and near-ties ----
GAP = 1e-5        # an element is ambiguous if its top-two candidates are closer than this share of the largest candidate magnitude


@contextlib.contextmanager
def recorded_candidates(model, into):
    """every layer's candidates (J, B, W, N, co) of the forwards inside are appended to ``into``.  The torch backend runs the windows of a layer
    batched and never calls its GcnOperation modules one by one, so the record is taken where the layer stacks their outputs."""
    real = {}
    for i, lay in enumerate(model.stsgcl_layers):
        real[i] = lay.layer.candidates

        def spy(data, adj, f=real[i]):
            c = f(data, adj)
            into.append(c.detach())
            return c
        lay.layer.candidates = spy
    try:
        yield into
    finally:
        for i, lay in enumerate(model.stsgcl_layers):
            del lay.layer.candidates


def ambiguous(cands, gap=GAP):
    """-> (number of ambiguous elements, number of elements) of one layer's candidates (J, ...)"""
    top = cands.double().topk(2, dim=0)[0]
    return int(((top[0] - top[1]) < gap * float(cands.abs().max())).sum()), top[0].numel()
