"""Predefined-graph helpers the downstream predictors need (reference model/STGCN/args.py:7-49, lib/predifineGraph.py:6-60,
model/TGCN/TGCN.py:8-25): scaled graph Laplacian and its Chebyshev polynomials (STGCN), the normalised adjacency (TGCN), the adjacency of the
PEMS distance csv, and a synthetic sensor graph for runs without the (non-redistributable) data files."""
import csv

import numpy as np
import torch


def scaled_laplacian(W):
    """2 L / lambda_max - I with L = D - W normalised by sqrt(d_i d_j) where both degrees are positive (args.py:7-26)."""
    W = np.asarray(W, dtype=np.float64)
    n = W.shape[0]
    d = W.sum(axis=1)
    L = -W.copy()
    L[np.arange(n), np.arange(n)] = d
    pos = d > 0
    scale = np.ones((n, n))
    scale[np.ix_(pos, pos)] = np.sqrt(np.outer(d[pos], d[pos]))
    L = L / scale
    lam = np.linalg.eigvals(L).max().real
    return 2 * L / lam - np.identity(n)


def cheb_polynomials(L, Ks):
    """T_0 = I, T_1 = L, T_k = 2 L T_{k-1} - T_{k-2}  ->  (Ks, n, n)   (args.py:29-49)."""
    n = L.shape[0]
    if Ks < 1:
        raise ValueError("the spatial kernel size must be >= 1, got %r" % (Ks,))
    out = [np.identity(n)]
    if Ks > 1:
        out.append(np.array(L, dtype=np.float64))
    for _ in range(Ks - 2):
        out.append(2 * L @ out[-1] - out[-2])
    return np.stack(out, axis=0)


def adjacency_from_distance_csv(path, num_nodes):
    """Directed 0/1 adjacency from rows ``from,to,distance`` (header skipped), as lib/predifineGraph.py:46-60."""
    A = np.zeros((num_nodes, num_nodes), dtype=np.float32)
    with open(path) as f:
        f.readline()
        for row in csv.reader(f):
            if len(row) == 3:
                A[int(row[0]), int(row[1])] = 1
    return A


def synthetic_adjacency(num_nodes, seed=0, degree=3):
    """A connected sensor-like graph: a ring plus a few random chords (stand-in when the dataset's csv is absent)."""
    rng = np.random.RandomState(seed)
    A = np.zeros((num_nodes, num_nodes), dtype=np.float32)
    for i in range(num_nodes):
        A[i, (i + 1) % num_nodes] = 1
        for j in rng.choice(num_nodes, size=max(degree - 1, 0), replace=False):
            if j != i:
                A[i, j] = 1
    return A


def stgcn_graph(A, Ks=3):
    """The ``args_predictor.G`` tensor of the reference (args.py:86-88; the reference hard-codes 3 polynomials there)."""
    return torch.tensor(cheb_polynomials(scaled_laplacian(A), Ks), dtype=torch.float32)


def astgcn_graph(A, K):
    """The (K, N, N) fp32 Chebyshev polynomials ``predictors.ASTGCN`` masks with its spatial attention (reference ASTGCN.py:8-47,284-286).  The
    reference takes lambda_max from ARPACK (scipy ``eigs(k=1, which='LR')``), this project from the dense eigenvalues: the two agree to ARPACK's
    stopping tolerance (tests/golden/make_golden_astgcn.py prints the difference it measures)."""
    return torch.tensor(cheb_polynomials(scaled_laplacian(A), K), dtype=torch.float32)


def stsgcn_graph(A):
    """A^ (N, N) fp32 = A with every diagonal entry 1: the diagonal block of the reference's ``construct_adj`` (STSGCN.py:237-253), whose
    (3N, 3N) localized adjacency is A^ on the three diagonal blocks and the identity on the blocks of adjacent steps.  ``predictors.STSGCN``
    builds that matrix for its torch backend (``stsgcn.window_adjacency``); the HIP backend multiplies by A^ alone."""
    a = np.array(A, dtype=np.float64)
    np.fill_diagonal(a, 1.0)
    return torch.tensor(a, dtype=torch.float32)


def normalized_adjacency(A):
    """TGCN's graph (reference TGCN.py:8-25, ``calculate_normalized_laplacian``): with A~ = A + I and D = diag(row sums of A~), the reference's
    operand order (A~ D^-1/2)^T D^-1/2 = D^-1/2 A~^T D^-1/2 — for a non-symmetric A the TRANSPOSE of the textbook D^-1/2 A~ D^-1/2."""
    At = np.asarray(A, dtype=np.float64) + np.identity(len(A))
    d = At.sum(axis=1)
    with np.errstate(divide="ignore"):
        dis = np.power(d, -0.5)
    dis[np.isinf(dis)] = 0.0
    return (At * dis[None, :]).T * dis[None, :]


def tgcn_graph(A):
    """The dense fp32 (N, N) graph of ``predictors.TGCN`` (the reference builds it inside the cell and casts it with ``.float()``, TGCN.py:37,116)."""
    return torch.tensor(normalized_adjacency(A), dtype=torch.float32)
