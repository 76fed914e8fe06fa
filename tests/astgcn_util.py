"""Shared by the ASTGCN golden generator and the ASTGCN tests: the parameter set the vectors are made with, and the condition on the inputs
that makes a comparison of gradients mean something (a saturated sigmoid passes no gradient: a wrong one behind it would go unseen)."""
import contextlib
import types

import numpy as np
import torch


def nonsymmetric_adjacency(n, seed=11):
    rng = np.random.RandomState(seed)
    A = (rng.rand(n, n) < 0.2).astype(np.float32)
    np.fill_diagonal(A, 0)
    A[np.arange(n), (np.arange(n) + 1) % n] = 1                          # connected ring underneath
    assert not np.array_equal(A, A.T)
    return A


def model_args(n, G, K=3, nb_block=2, width=64, time_strides=1, T=12):
    return types.SimpleNamespace(nb_block=nb_block, K=K, nb_chev_filter=width, nb_time_filter=width, time_strides=time_strides, len_input=T,
                                 num_for_predict=12, num_nodes=n, G=G)


def xavier_pass_(model):
    """the reference Run.py's pass: xavier_uniform_ for dim > 1, else uniform_, in parameter order"""
    for p in model.parameters():
        if p.requires_grad:
            torch.nn.init.xavier_uniform_(p) if p.dim() > 1 else torch.nn.init.uniform_(p)


def move_score_vectors_(model):
    """U1, U3, W1, W3 <- 0.25 (p - 0.5) in every block: the plain pass leaves them in [0, 1), which saturates the second block's sigmoids"""
    with torch.no_grad():
        for blk in model.BlockList:
            for p in (blk.TAt.U1, blk.TAt.U3, blk.SAt.W1, blk.SAt.W3):
                p.copy_(0.25 * (p - 0.5))


def scale_u1_(model, n):
    """after move_score_vectors_: TAt.U1 <- min(1, 64 / n) min(1, 64 / f) U1 in every block, f the block's input width.  The temporal score sums
    U1 over the n nodes and U2, U3 over the f features, so the temporal sigmoid's input grows with both: with the pass above alone the first one
    saturates from 250 nodes on (0.44 of its inputs inside |z| < 4 at 250, 0.36 at 266 and 320), and the second block's at 112 features (0.39)"""
    with torch.no_grad():
        for blk in model.BlockList:
            blk.TAt.U1.mul_(min(1.0, 64.0 / n) * min(1.0, 64.0 / blk.TAt.U3.shape[0]))


def tap(x4, W, b, taps):
    """the definition of ops.stgcn_tapgemm on (B, T, N, ci): sum_j x[t + taps[j]] W_j + b, zero outside [0, T); W (co, len(taps) ci) tap-major"""
    T = x4.shape[1]
    cols = []
    for dt in taps:
        s = torch.zeros_like(x4)
        lo, hi = max(0, -dt), min(T, T - dt)
        s[:, lo:hi] = x4[:, lo + dt:hi + dt]
        cols.append(s)
    y = torch.cat(cols, -1) @ W.t()
    return y if b is None else y + b


@contextlib.contextmanager
def recorded_sigmoids(into):
    """every input torch.sigmoid sees inside the block is appended to `into` (the model calls it once per attention layer)"""
    real = torch.sigmoid

    def spy(z):
        into.append(z.detach())
        return real(z)

    torch.sigmoid = spy
    try:
        yield into
    finally:
        torch.sigmoid = real


def assert_condition(zs, grads, n_sigmoids=4):
    """a condition on the INPUTS, not a tolerance: in each sigmoid at least half the inputs lie in |z| < 4, and no parameter's gradient is
    identically zero.  -> the fractions"""
    assert len(zs) == n_sigmoids, len(zs)
    frac = [float((z.abs() < 4).double().mean()) for z in zs]
    assert all(f >= 0.5 for f in frac), frac
    dead = [k for k, g in grads.items() if g is None or not bool((torch.as_tensor(g) != 0).any())]
    assert not dead, dead
    return frac
