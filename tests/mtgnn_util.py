"""Inputs for the MTGNN tests whose learned graph has no tie at a top-k cut (used by tests/golden/make_golden_mtgnn.py and the GPU tests).

The graph constructor keeps the ``subgraph_size`` largest entries of every row of relu(tanh(alpha a)).  Where the k-th and the (k+1)-th value of
a row are equal or a rounding error apart, which of them a top-k keeps depends on the device and the precision, and a comparison of two
implementations would compare two different graphs.  Two things make such ties with the default N(0, 1) embeddings: tanh(3 a) saturates to
exactly 1.0 in more than k entries of a row, and among ~N/2 positive values per row some pair is always close.  A cut at which the
(k+1)-th value is 0 is no tie that matters: entries that are 0 stay 0 under the mask, and relu passes them no gradient."""
import torch


def dense_graph(gc):
    """relu(tanh(alpha (n1 n2^T - n2 n1^T))) of a graph constructor, before its top-k (this project's module or the reference's)"""
    n1 = torch.tanh(gc.alpha * gc.lin1(gc.emb1.weight))
    n2 = torch.tanh(gc.alpha * gc.lin2(gc.emb2.weight))
    return torch.relu(torch.tanh(gc.alpha * (n1 @ n2.t() - n2 @ n1.t())))


def cut_gaps(gc, k):
    """-> (smallest k-th minus (k+1)-th value over the rows that cut among positive values, number of such rows)"""
    with torch.no_grad():
        top = dense_graph(gc).sort(1, descending=True)[0]
    if k >= top.shape[1]:
        return float("inf"), 0
    cut = top[:, k] > 0
    return (float((top[:, k - 1] - top[:, k])[cut].min()) if bool(cut.any()) else float("inf")), int(cut.sum())


def clear_topk_cuts(gc, k, min_gap=2e-3, seed=0, rounds=2000):
    """shrink the node embeddings until no entry of the graph is above 0.99 (no saturation), then nudge the embeddings of every node whose row
    cuts closer than ``min_gap`` until no row does.  Deterministic for a given module and seed.  -> the smallest gap left"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        while float(dense_graph(gc).max()) > 0.99:
            gc.emb1.weight.mul_(0.8)
            gc.emb2.weight.mul_(0.8)
        step = 0.05 * float(gc.emb1.weight.std())
        for _ in range(rounds):
            top = dense_graph(gc).sort(1, descending=True)[0]
            if k >= top.shape[1]:
                break
            bad = ((top[:, k] > 0) & (top[:, k - 1] - top[:, k] < min_gap)).nonzero().flatten()
            if bad.numel() == 0:
                break
            for e in (gc.emb1.weight, gc.emb2.weight):
                e[bad] += step * torch.randn(bad.numel(), e.shape[1], generator=g).to(e.dtype)
    gap, _ = cut_gaps(gc, k)
    assert gap >= min_gap, gap
    return gap


def same_support(a, b):
    """two adjacencies keep the same entries"""
    return bool(((a > 0) == (b.to(a.device) > 0)).all())
