"""Shared by the STGODE golden generator and the STGODE tests: the graphs and argument set the vectors are made with, the xavier-style redraw,
and the transcription in plain torch of what predictors/stgode_hip.py computes launch by launch — the fused Euler step with its hand-written
backward (the detached x0 makes it another function than the derivative of the forward), the dalpha / dW / dW2 reductions, the batch norm
over the node channel and the running max over the branches.  The near-tie condition is stsgcn_util's GAP."""
import types

import numpy as np
import torch

import stsgcn_util as su
from stsgcn_util import GAP                                                # noqa: F401

SEED = 2468
DEAD = (".temporal1.", ".temporal2.")                                      # the keys of the convolutions that never run


def graphs(n, seed=11):
    """(A_sp, A_se) float32 tensors: two different NON-symmetric graphs with the scale of the reference's 0.4 (I + normalised)"""
    eye = np.eye(n, dtype=np.float32)
    a, b = 0.4 * (eye + su.adjacency(n, seed)), 0.4 * (eye + su.adjacency(n, seed + 100))
    assert np.abs(a - a.T).max() > 1e-2 and np.abs(b - b.T).max() > 1e-2 and np.abs(a - b).max() > 1e-2
    return torch.from_numpy(a), torch.from_numpy(b)


def model_args(n, T=5, P=3, n_layers=3, out_channels=(64, 32, 64), in_channels=64, g=None):
    sp, se = graphs(n) if g is None else g
    return types.SimpleNamespace(num_nodes=n, num_timesteps_input=T, num_timesteps_output=P, in_channels=in_channels,
                                 out_channels=list(out_channels), n_layers=n_layers, A_sp_wave=sp, A_se_wave=se)


def xavier_redraw_(model):
    """the redraw of enhance.xavier_downstream_ (reference Run.py:79-85) over a bare predictor: xavier_uniform_ for dim > 1, else uniform_"""
    for _, p in model.named_parameters():
        torch.nn.init.xavier_uniform_(p) if p.dim() > 1 else torch.nn.init.uniform_(p)
    return model


def is_dead(key):
    return any(d in key for d in DEAD)


# ---- one block, launch by launch ------------------------------------------------------------------------------------------------------------
def step_fwd(X, A, alpha, W, W2):
    """X (B, T, N, C) the block's input, alpha = sigmoid(alpha) (N) -> (z, At): t = relu(X),
    z = relu(3 alpha_n (A t)[n] + 6 t W + 6 sum_k W2[k, tau] t[k] - 11 t)"""
    t = torch.relu(X)
    At = torch.einsum("ij,btjc->btic", A, t)
    pre = 3 * alpha[:, None] * At + 6 * (t @ W) + 6 * torch.einsum("km,bknc->bmnc", W2, t) - 11 * t
    return torch.relu(pre), At, pre


def step_bwd(g, X, A, alpha, W, W2):
    """g = dz [z > 0] -> dX: dt = 3 A^T (alpha . g) + 6 g W^T + 6 sum_m W2[tau, m] g[m] - 17 g, dX = dt [X > 0]"""
    dt = 3 * torch.einsum("ji,btjc->btic", A, alpha[:, None] * g) + 6 * (g @ W.t()) + 6 * torch.einsum("km,bmnc->bknc", W2, g) - 17 * g
    return dt * (X > 0)


def step_param_grads(g, X, At):
    """-> (dalpha (N) with respect to sigmoid(alpha), dW (C, C), dW2 (T, T))"""
    t = torch.relu(X)
    return (3 * (g * At).sum((0, 1, 3)), 6 * torch.einsum("btnc,btnd->cd", t, g), 6 * torch.einsum("bknc,bmnc->km", t, g))


def bn_fwd(z, gamma, beta, eps=1e-5):
    """batch norm with the NODE as the channel, batch statistics -> (y, mean, var biased, var unbiased)"""
    n = z.numel() // z.shape[2]
    mean = z.mean((0, 1, 3))
    var = ((z - mean[:, None]) ** 2).sum((0, 1, 3)) / n
    y = (z - mean[:, None]) / torch.sqrt(var[:, None] + eps) * gamma[:, None] + beta[:, None]
    return y, mean, var, var * n / max(n - 1, 1)


def bn_eval(z, gamma, beta, rmean, rvar, eps=1e-5):
    return (z - rmean[:, None]) / torch.sqrt(rvar[:, None] + eps) * gamma[:, None] + beta[:, None]


def bn_bwd(dy, z, gamma, mean, var, eps=1e-5):
    """-> (dz, dgamma, dbeta)"""
    n = z.numel() // z.shape[2]
    rstd = 1 / torch.sqrt(var + eps)
    xh = (z - mean[:, None]) * rstd[:, None]
    s1, s2 = dy.sum((0, 1, 3)), (dy * xh).sum((0, 1, 3))
    return (gamma * rstd)[:, None] * (dy - s1[:, None] / n - xh * s2[:, None] / n), s2, s1


def running_max(outs):
    """[y_i] -> (best, which int32): a later branch replaces where STRICTLY greater, so an exact tie stays with the lowest index"""
    best, which = outs[0].clone(), torch.zeros_like(outs[0], dtype=torch.int32)
    for i, y in enumerate(outs[1:], 1):
        win = y > best
        best, which = torch.where(win, y, best), torch.where(win, torch.full_like(which, i), which)
    return best, which


def model_manual(model, x, dy_head=None):
    """the whole module on the functions above, forward and (with ``dy_head`` = the gradient of the max's output) the hand-written backward
    -> dict(best, which, records per block, dx, grads {key: tensor} of alpha (through the sigmoid), W, W2 effective matrices' sources)"""
    recs, outs = [], []
    for bi, (seq, A) in enumerate(model.branches()):
        h = x
        for blk in seq:
            f = blk.odeg.odeblock.odefunc
            alpha, W, W2 = (m.detach() for m in f.mats())
            z, At, pre = step_fwd(h, A, alpha, W, W2)
            bn = blk.batch_norm
            y, mean, var, varu = bn_fwd(z, bn.weight.detach(), bn.bias.detach(), bn.eps)
            recs.append(dict(branch=bi, blk=blk, A=A, X=h, z=z, At=At, pre=pre, mean=mean, var=var, varu=varu, y=y, alpha=alpha, W=W, W2=W2))
            h = y
        outs.append(h)
    best, which = running_max(outs)
    res = dict(best=best, which=which, recs=recs, outs=outs)
    if dy_head is None:
        return res
    dx = torch.zeros_like(x)
    for bi in range(len(outs)):
        up = dy_head * (which == bi)
        for r in reversed([r for r in recs if r["branch"] == bi]):
            bn = r["blk"].batch_norm
            dz, r["dgamma"], r["dbeta"] = bn_bwd(up, r["z"], bn.weight.detach(), r["mean"], r["var"], bn.eps)
            g = dz * (r["z"] > 0)
            r["dalpha"], r["dW"], r["dW2"] = step_param_grads(g, r["X"], r["At"])
            up = step_bwd(g, r["X"], r["A"], r["alpha"], r["W"], r["W2"])
        dx += up
    res["dx"] = dx
    return res


def unambiguous(res, x, gap=GAP):
    """on an fp64 ``model_manual`` record: (max gaps <= g, step pre-activations within g of zero, block inputs within g of zero), each a count;
    g = gap times the largest magnitude of the tensor in question"""
    cands = torch.stack(res["outs"]).double()
    top = cands.topk(2, dim=0)[0]
    ties = int(((top[0] - top[1]) <= gap * float(cands.abs().max())).sum()) if cands.shape[0] > 1 else 0
    pre0 = sum(int((r["pre"].abs() <= gap * float(r["pre"].abs().max())).sum()) for r in res["recs"])
    in0 = sum(int((r["X"].abs() <= gap * float(r["X"].abs().max())).sum()) for r in res["recs"])
    return ties, pre0, in0
