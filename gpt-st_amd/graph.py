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


# ---- MSDR: the fixed supports of a GMSDR cell (reference model/MSDR/args.py:9-50, gmsdr_cell.py:80-91) ----------------------------------------
def msdr_supports(A, filter_type):
    """The (S, N, N) fp32 fixed supports ``predictors.MSDR`` multiplies by, dense where the reference keeps them sparse, from the raw
    adjacency in fp32 as the reference holds it:

        "dual_random_walk"   S = 2: (D^-1 A)^T and (D_T^-1 A^T)^T, D and D_T the row sums of A and A^T
        "random_walk"        S = 1: (D^-1 A)^T
        "laplacian"          S = 1: 2 L / lambda_max - I, L the normalised Laplacian of max(A, A^T); lambda_max from the dense eigenvalues
                             (the reference asks ARPACK for the largest one)
        anything else        S = 1: the same with lambda_max = 2, i.e. L - I.  The reference's default lands here: its ``--filter_type``
                             takes its default from the conf's ``cl_decay_steps`` ("2000"), so the confs' own value is never read."""
    a = np.asarray(A, dtype=np.float32)
    n = len(a)

    def random_walk(m):
        d = m.sum(axis=1)
        with np.errstate(divide="ignore"):
            inv = np.power(d, -1)
        inv[np.isinf(inv)] = 0.0
        return inv[:, None] * m

    def scaled_laplacian(lambda_max):
        m = np.maximum(a, a.T)
        d = m.sum(axis=1)
        with np.errstate(divide="ignore"):
            dis = np.power(d, -0.5)
        dis[np.isinf(dis)] = 0.0
        lap = np.identity(n) - (m * dis[None, :]).T * dis[None, :]             # the reference's operand order: (A D^-1/2)^T D^-1/2
        if lambda_max is None:
            lambda_max = float(np.abs(np.linalg.eigvalsh(lap)).max())          # ARPACK's 'LM': the largest magnitude
        return (2.0 / lambda_max) * lap - np.identity(n)

    if filter_type == "laplacian":
        sup = [scaled_laplacian(None)]
    elif filter_type == "random_walk":
        sup = [random_walk(a).T]
    elif filter_type == "dual_random_walk":
        sup = [random_walk(a).T, random_walk(a.T).T]
    else:
        sup = [scaled_laplacian(2.0)]
    return torch.tensor(np.stack([np.asarray(s, dtype=np.float32) for s in sup]), dtype=torch.float32)


# ---- STFGNN: the spatial-temporal fusion graph (reference model/STFGNN/args.py:10-151) ---------------------------------------------------
def stfgnn_fusion_graph(A, A_dtw, steps=4):
    """The (steps N, steps N) fp32 fusion matrix of ``construct_adj_fusion`` (args.py:101-151), from the spatial adjacency A and the temporal
    (DTW) graph A_dtw.  With "1" the identity block and X^ = X with a unit diagonal (every diagonal entry is forced to 1 last):

        [ D^ 1  1  D ]
        [ 1  S^ 1  1 ]
        [ 1  1  S^ 1 ]
        [ D  1  1  D^]

    The reference writes the blocks by index 3N..4N whatever ``steps`` is; every conf has 4, and nothing else is built here."""
    if steps != 4:
        raise ValueError("the STFGNN fusion graph is defined for 4 steps (reference args.py:139-145 index block 3), got %r" % (steps,))
    A, D = np.asarray(A, dtype=np.float64), np.asarray(A_dtw, dtype=np.float64)
    n = len(A)
    adj = np.zeros((n * steps, n * steps))
    eye = np.identity(n)
    blk = lambda i, j: (slice(i * n, (i + 1) * n), slice(j * n, (j + 1) * n))      # noqa: E731
    for i in range(steps):
        adj[blk(i, i)] = A if i in (1, 2) else D
    for k in range(steps - 1):                                                       # adjacent steps: the node's own row, both ways
        np.fill_diagonal(adj[blk(k, k + 1)], 1.0)
        np.fill_diagonal(adj[blk(k + 1, k)], 1.0)
    adj[blk(3, 0)] = D
    adj[blk(0, 3)] = D
    for i, j in ((2, 0), (0, 2), (1, 3), (3, 1)):
        adj[blk(i, j)] = adj[blk(0, 1)]
    assert np.array_equal(adj[blk(0, 1)], eye)
    np.fill_diagonal(adj, 1.0)
    return torch.tensor(adj, dtype=torch.float32)


def stfgnn_blocks(adj):
    """(S^, D) — both (N, N) fp32 — when ``adj`` (4N, 4N) has exactly the form ``stfgnn_fusion_graph`` gives for a D with a unit diagonal
    (``dtw_graph`` always gives one): the ten identity blocks exact, block(0,0) = block(3,3) = block(0,3) = block(3,0) = D, block(1,1) =
    block(2,2) = S^.  None for any other matrix: the HIP backend of ``predictors.STFGNN`` multiplies by the two blocks alone and serves no other."""
    adj = torch.as_tensor(adj)
    if adj.dim() != 2 or adj.shape[0] != adj.shape[1] or adj.shape[0] % 4 or adj.shape[0] == 0:
        return None
    n = adj.shape[0] // 4
    b = adj.reshape(4, n, 4, n).permute(0, 2, 1, 3)                                  # b[i, j] = block (i, j)
    eye = torch.eye(n, dtype=adj.dtype, device=adj.device)
    for i, j in ((0, 1), (0, 2), (1, 0), (1, 2), (1, 3), (2, 0), (2, 1), (2, 3), (3, 1), (3, 2)):
        if not torch.equal(b[i, j], eye):
            return None
    D, S = b[0, 3], b[1, 1]
    if not (torch.equal(b[3, 0], D) and torch.equal(b[0, 0], D) and torch.equal(b[3, 3], D) and torch.equal(b[2, 2], S)):
        return None
    return S.float().contiguous(), D.float().contiguous()


def _dtw_series(series, dataset, slots, day_slots, train_share, total_steps=None):
    """(days, slots, N) float64: the first channel, the first ``train_share`` of the days (construct_dtw + gen_data, args.py:10-24,59-67).
    ``total_steps``: the length of the whole series where ``series`` is only its head (the training split): the day count comes from it, and a
    last part-day of the head is dropped"""
    data = torch.as_tensor(series)
    if data.dim() == 3:
        data = data[:, :, 0]
    data = data.double()
    if day_slots is None:
        day_slots = 96 if dataset == "SZ_TAXI" else 288                              # the reference counts days of 288 slots for the NYC sets too
    if slots is None:
        slots = 96 if dataset == "SZ_TAXI" else 48 if dataset in ("NYC_TAXI", "NYC_BIKE") else 288
    tr_day = int((data.shape[0] if total_steps is None else total_steps) / day_slots * train_share)
    n = data.shape[1]
    full = data.shape[0] // slots * slots
    if full != data.shape[0] and total_steps is None:
        raise ValueError("the series has %d steps, no whole number of days of %d slots" % (data.shape[0], slots))
    if full < tr_day * slots:
        raise ValueError("the series has %d whole days, the DTW graph reads %d" % (full // slots, tr_day))
    return data[:full].reshape(-1, slots, n)[:tr_day]


def dtw_distances(x, band=12, chunk=2048, normalise=True):
    """x (days, slots, N) -> (N, N) float64, upper triangle: the banded DTW distance of ``compute_dtw`` (args.py:26-57, order 1) between the
    series of nodes i < j.  Every day's row is normalised on its own; the local cost of slots (p of j, q of i) is the sum over the days of
    |a[day, q] - b[day, p]|; the recurrence runs over the band |p - q| <= band, whose edges drop the neighbour outside it.  Vectorised over the
    node pairs (the reference loops over them in Python), ``chunk`` pairs at a time on x's device; the band's cells of one row depend on their
    left neighbour, so the recurrence itself is a loop of slots * (2 band + 1) steps.  ``band >= slots - 1`` is the unconstrained, exact DTW;
    ``normalise=False`` takes the series as they are (STGODE: ``stgode_dtw_distances``)."""
    x = x.double()
    days, T0, n = x.shape
    z = (x - x.mean(1, keepdim=True)) / x.std(1, unbiased=False, keepdim=True) if normalise else x
    z = z.permute(2, 0, 1).contiguous()                                              # (N, days, slots)
    iu, ju = torch.triu_indices(n, n, 1, device=x.device)
    out = torch.zeros(n, n, dtype=torch.float64, device=x.device)
    inf = float("inf")
    for c0 in range(0, iu.numel(), chunk):
        a, b = z[iu[c0:c0 + chunk]], z[ju[c0:c0 + chunk]]                            # a: node i (columns q), b: node j (rows p)
        P = a.shape[0]
        prev = None
        for p in range(T0):
            lo, hi = max(0, p - band), min(T0, p + band + 1)
            cost = (a[:, :, lo:hi] - b[:, :, p:p + 1]).abs().sum(1)                  # (P, hi - lo)
            row = torch.full((P, T0), inf, dtype=torch.float64, device=x.device)     # cells outside the band are never the minimum
            for q in range(lo, hi):
                if p == 0 and q == 0:
                    best = torch.zeros(P, dtype=torch.float64, device=x.device)
                elif p == 0:
                    best = row[:, q - 1]
                elif q == 0:
                    best = prev[:, 0]
                else:
                    best = torch.minimum(torch.minimum(prev[:, q - 1], prev[:, q]), row[:, q - 1])
                row[:, q] = cost[:, q - lo] + best
            prev = row
        out[iu[c0:c0 + chunk], ju[c0:c0 + chunk]] = prev[:, T0 - 1]
    return out


def dtw_graph(series, dataset="PEMS08", band=12, adj_percent=0.01, train_share=0.6, slots=None, day_slots=None, chunk=2048,
              return_distances=False, total_steps=None):
    """The 0/1 temporal graph of ``construct_dtw`` (args.py:59-99) as (N, N) float64 numpy: the banded DTW distance between every two nodes'
    training series (``dtw_distances``), for each node its ``int(N * adj_percent)`` nearest (itself, at distance 0, among them), made
    symmetric by taking an edge that either side has, and a unit diagonal.  ``series`` (L, N[, F]): the first channel is used, on the
    series' device.  Quirks kept: the day count is L / 288 for every dataset but SZ_TAXI, also where a day has 48 slots (so the NYC sets use a
    tenth of their days); ``slots`` / ``day_slots`` override the two for series of another shape.  ``total_steps``: see ``_dtw_series``."""
    x = _dtw_series(series, dataset, slots, day_slots, train_share, total_steps)
    d = dtw_distances(x, band, chunk)
    dtw = (d + d.t()).cpu().numpy()
    n = dtw.shape[0]
    w = np.zeros((n, n))
    top = int(n * adj_percent)
    for i in range(n):
        w[i, dtw[i].argsort()[:top]] = 1
    w = np.maximum(w, w.T)
    np.fill_diagonal(w, 1.0)
    return (w, d.cpu().numpy()) if return_distances else w


# ---- STGODE: the spatial and the semantic (DTW) graph (reference model/STGODE/args.py:10-144) ---------------------------------------------
def stgode_normalized_adj(A):
    """``get_normalized_adj`` (args.py:133-144): 0.4 (I + D^-1/2 A D^-1/2) with D the row sums, floored at 1e-4 -> (N, N) float32 tensor"""
    A = np.asarray(A, dtype=np.float64)
    deg = A.sum(1)
    deg[deg <= 10e-5] = 10e-5
    dinv = 1.0 / np.sqrt(deg)
    return torch.from_numpy((0.8 / 2 * (np.eye(A.shape[0]) + dinv[:, None] * A * dinv[None, :])).astype(np.float32))


def stgode_adjacencies(sp_dist, dtw_dist, sigma1, sigma2, thres1, thres2):
    """the thresholding of ``read_data`` (args.py:57-65, 118-125) -> (sp_matrix, dtw_matrix), float64 numpy.  Semantic: the DTW distances
    z-scored over all entries, exp(-z^2 / sigma1^2), 1 where above thres1 and 0 elsewhere.  Spatial: the distances z-scored over their
    finite entries, exp(-z^2 / sigma2^2) (0 at an infinite distance), kept where at least thres2."""
    d = np.asarray(dtw_dist, dtype=np.float64)
    d = (d - d.mean()) / d.std()
    dtw = (np.exp(-d ** 2 / sigma1 ** 2) > thres1).astype(np.float64)
    s = np.asarray(sp_dist, dtype=np.float64)
    fin = s[s != np.inf]
    s = (s - fin.mean()) / fin.std()
    sp = np.exp(-s ** 2 / sigma2 ** 2)
    sp[sp < thres2] = 0
    return sp, dtw


def stgode_graphs(sp_dist, dtw_dist, sigma1, sigma2, thres1, thres2):
    """(A_sp_wave, A_se_wave) of reference args.py:176-177: ``stgode_normalized_adj`` of the two thresholded matrices"""
    sp, dtw = stgode_adjacencies(sp_dist, dtw_dist, sigma1, sigma2, thres1, thres2)
    return stgode_normalized_adj(sp), stgode_normalized_adj(dtw)


def stgode_spatial_distance(A):
    """the spatial distances where only an adjacency exists — the reference's rule for the NYC sets (args.py:92-94), used for the synthetic
    graph too: (1 - adj) 1000"""
    return (1.0 - np.asarray(A, dtype=np.float32)) * 1000


def stgode_spatial_distance_csv(path, dataset, num_nodes):
    """the spatial distances from the dataset's csv by the reference's per-dataset rules (args.py:82-108): a matrix file read as it is
    (METR_LA, PEMS07M), a 0/1 matrix turned into 1000 / 5 (SZ_TAXI) or (1 - adj) 1000 (the NYC sets), else rows ``from,to,distance`` under a
    header, entered symmetrically into a matrix of infinities"""
    if dataset in ("PEMS07M", "METR_LA", "SZ_TAXI", "NYC_TAXI", "NYC_BIKE"):
        m = np.loadtxt(path, delimiter=",", dtype=np.float64, ndmin=2)
        if dataset == "SZ_TAXI":
            m = np.where(m == 0, 1000.0, np.where(m == 1, 5.0, m)).astype(np.float32)
        elif dataset in ("NYC_TAXI", "NYC_BIKE"):
            m = stgode_spatial_distance(m)
        return m
    d = np.full((num_nodes, num_nodes), np.inf)
    with open(path) as f:
        f.readline()
        for row in csv.reader(f):
            if len(row) >= 3:
                i, j = int(row[0]), int(row[1])
                d[i, j] = d[j, i] = float(row[2])
    return d


def stgode_dtw_distances(series, day_slots=288, chunk=16384):
    """(N, N) float64 symmetric: the DTW distance (local cost |a - b|) between the day-mean profiles of every two nodes (args.py:45-54).
    ``series`` (L, N[, F]) as the reference has it there, z-scored; the first channel, whole days of ``day_slots``.  The recurrence is the
    project's own (``dtw_distances`` with the band opened to the whole day and no per-row normalisation): the exact distance, where the
    reference's ``fastdtw(radius=6)`` approximates it."""
    data = torch.as_tensor(series)
    if data.dim() == 3:
        data = data[:, :, 0]
    days = data.shape[0] // day_slots
    if days < 1:
        raise ValueError("the series has %d steps: not one whole day of %d slots" % (data.shape[0], day_slots))
    prof = data[:days * day_slots].double().reshape(days, day_slots, -1).mean(0)
    d = dtw_distances(prof[None], band=day_slots, chunk=chunk, normalise=False)
    return (d + d.t()).cpu().numpy()


def stmgcn_supports(adj):
    """The (3, N, N) fp32 Chebyshev supports [I, L~, 2 L~^2 - I] ``predictors.STMGCN`` multiplies by, from one raw graph as the reference
    builds them (model/STMGCN_demand/GCN.py ``Adj_Preprocessor('chebyshev', K=2)``, args.py:43-51), in fp32 torch ops as there:

        A_norm = D^-1/2 A D^-1/2 with D the row sums;  L = I - A_norm;  L~ = (2 / lambda_max) L - I with lambda_max = 2

    lambda_max is 2 always: the reference asks ``torch.eig`` for it inside a bare ``except``, a call every torch this project runs on
    refuses, so its fallback is what runs (the line it prints there is dropped).  ``rowsum ** -0.5`` is taken as it comes: a zero row sum
    gives inf, a negative one (a correlation graph has them) NaN, both spread through the products, and ``nan_to_num`` at the very end turns
    what is left of them into fp32's largest value and 0."""
    a = torch.as_tensor(np.asarray(adj, dtype=np.float32))
    eye = torch.eye(a.shape[0])
    d = torch.diag(torch.pow(a.sum(dim=1), -0.5))
    lap = eye - torch.mm(torch.mm(d, a), d)
    lt = (2 / 2) * lap - eye
    return torch.nan_to_num(torch.stack([eye, lt, 2 * torch.mm(lt, lt) - eye], dim=0))


def stmgcn_correlation(series):
    """(N, N) fp32 Pearson correlation between the nodes of a (L, N) series, the diagonal zeroed; a constant node correlates 0 with all"""
    s = np.asarray(series, dtype=np.float64)
    s = s - s.mean(0, keepdims=True)
    sd = np.sqrt((s * s).sum(0))
    c = (s.T @ s) / np.maximum(np.outer(sd, sd), 1e-30)
    np.fill_diagonal(c, 0.0)
    return c.astype(np.float32)


def ccrnn_support(series, hidden_size_data, normalized_category="randomwalk", holdout=1700):
    """The (N, N) float64 support ``predictors.CCRNN`` takes its node vectors from, as the reference builds it (model/CCRNN_demand/args.py:33-76
    ``preprocessing_for_metric``, ``random_walk_matrix``; normalization.py ``Standard``), in numpy as there.  series (T, N, 2): the pick-up and
    drop-off channels.

        z = (series - mean) / std over the whole array;  as (T, 2, N), the last ``holdout`` frames dropped, rows (t, channel)
        u, s, v = svd(rows);  w = (diag(s[:h]) v[:h]).T            (N, h): every node's coordinates on the first h right singular vectors
        d = pairwise Euclidean distances of w;  support = exp(-d / std(d)^2) - I;  'randomwalk': D^-1 support (an empty row stays 0)

    A sign flip of a right singular vector flips a column of w, which the distances do not see.  ``'laplacian'`` is refused: the reference's
    ``normalized_laplacian`` multiplies the identity by the SHAPE TUPLE of the degree vector, not by its inverse square roots, so what it
    returns is I - N^2 support; no shipped conf selects it and the slip is not reproduced.  Any other category leaves the matrix as it is,
    as the reference does."""
    if normalized_category == "laplacian":
        raise ValueError("ccrnn_support: normalized_category 'laplacian' is not built: the reference's normalized_laplacian scales by the shape of "
                         "the degree vector instead of its inverse square roots (args.py:17-23); use 'randomwalk'")
    x = np.asarray(series, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 2:
        raise ValueError("ccrnn_support: series must be (T, N, 2), got %r" % (x.shape,))
    if not 0 <= holdout < x.shape[0]:                                          # (0: nothing is held out — the reference's own slice cannot say that)
        raise ValueError("ccrnn_support: holdout %r leaves nothing of %d frames" % (holdout, x.shape[0]))
    z = (1. * (x - np.mean(x)) / np.std(x)).transpose(0, 2, 1)[:x.shape[0] - holdout]
    rows = z.reshape(-1, z.shape[2])
    _, s, v = np.linalg.svd(rows, full_matrices=False)
    h = int(hidden_size_data)
    w = np.diag(s[:h]).dot(v[:h, :]).T
    d = np.sqrt(((w[:, None, :] - w[None, :, :]) ** 2).sum(-1))
    support = np.exp(d * -1 / np.std(d) ** 2) - np.identity(d.shape[0])
    if normalized_category == "randomwalk":
        deg = support.sum(1)
        with np.errstate(divide="ignore"):
            d_inv = np.power(deg, -1)
        d_inv[np.isinf(d_inv)] = 0.
        support = (np.eye(d_inv.shape[0]) * d_inv).dot(support)
    return support


def dmvstnet_adjacency(path, num_nodes):
    """The (N, N) fp32 graph ``predictors.DMVSTNET`` multiplies by: the header-less, comma-separated N x N matrix of ``path`` as it is — the
    reference (model/DMVSTNET_demand/args.py:32-33) neither normalises nor thresholds it.  Any other shape is refused."""
    a = np.loadtxt(path, delimiter=",", dtype=np.float32, ndmin=2)
    if a.shape != (num_nodes, num_nodes):
        raise ValueError("DMVSTNET reads a header-less %d x %d matrix, %s holds %r" % (num_nodes, num_nodes, path, a.shape))
    return a
