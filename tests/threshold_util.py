"""Reference side of the threshold-cell tests (tests/test_threshold_cells_cpu.py, tests/test_gpu_threshold_cells.py): plain torch on the CPU,
nothing from the kernels' side.

The pretraining loss and every reported metric keep a cell by `y > thresh`, y the de-normalised label.  The rule is the reference's fp32 torch
arithmetic, `label * std + mean`: a rounded multiply, then a rounded add (inverse32).  A raw zero is stored as fl32((0 - mean) / std); with the
synthetic scaler (230, 146) inverse32 returns exactly 0.0 for it, while ONE fused multiply-add (inverse_fused: what fp64 returns as well) leaves
+7.153e-6.  At threshold 0 the rule drops such a cell and the fused form keeps it, so labels with planted stored zeros (plant_zeros) under a
mask separate the two; labels drawn with randn never do.

The inputs of the GPU file are built here too (metric_inputs, loss_inputs, tail_inputs, step_inputs), so that the CPU file can hold every one
of them to the condition that makes the GPU assertions mean something."""
import torch

from gptst_amd import synth

SIGMA, MU = synth.SCALER_STD, synth.SCALER_MEAN
SHARE = 0.1                                    # share of the flow cells that hold a stored raw zero


def stored_zero():
    """fl32(scaler.transform(0)) as a python float"""
    return float(torch.tensor(synth.scaler_zeros(), dtype=torch.float32))


def inverse32(x, sigma=SIGMA, mu=MU):
    """StandardScaler.inverse_transform as fp32 torch forms it — two ops, two roundings.  THE RULE."""
    t = x.float() * sigma
    return t + mu


def inverse_fused(x, sigma=SIGMA, mu=MU):
    """the same value from one rounding: computed in fp64 (the product of an fp32 value and the scaler is exact there) and rounded to fp32 — what
    a fused multiply-add returns.  Only used to show, on the reference alone, that an input separates the two rules."""
    return (x.double() * sigma + mu).float()


def plant_zeros(src, base, share=SHARE, seed=0):
    """set `share` of the flow cells src[..., :base] to the stored raw zero, in place -> the boolean plant (shape of src[..., :base])"""
    g = torch.Generator().manual_seed(seed)
    plant = torch.rand(src[..., :base].shape, generator=g) < share
    src[..., :base][plant] = stored_zero()
    return plant


def visibility(shape, seed):
    """1 = visible, as tests/test_gpu_kernels.py::test_loss_and_kl draws it"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) > 0.25).float()


def kept(y, thresh):
    return torch.ones_like(y, dtype=torch.bool) if thresh is None else y > thresh


# ---- metrics (csrc/metrics.hip) -------------------------------------------------------------------------------------------------------------
def metric_py(out, src, vis, sigma, mu, D):
    """(p, y) as Trainer.test forms them in pretrain mode, fp32: inverse(out * m), inverse(label * m), m = 1 - vis (all ones without vis)"""
    label = src[..., :D].float()
    out = out.reshape(label.shape).float()
    m = torch.ones_like(label) if vis is None else 1.0 - vis.reshape(label.shape).float()
    return inverse32(out * m, sigma, mu), inverse32(label * m, sigma, mu)


def metric_sums(out, src, lda, vis, sigma, mu, mae_t, mape_t, T, N, D, absolute=False):
    """The tables of csrc/metrics.hip's header comment over out (B*T*N, D), src (B, T, N, lda), vis (B*T*N*D) or None ->
    (T, 5) [n1, sum|e|, sum e^2, n2, sum|e/y|] and (T, N, 6) [K, sum p, sum y, sum p^2, sum y^2, sum p y], float64.
    p, y, e = y - p and e / y are fp32 torch values; every sum is taken in fp64.  absolute=True: the sums of the ABSOLUTE terms (what an
    accumulation-order bound is relative to)."""
    assert src.shape[1:] == (T, N, lda)
    p, y = metric_py(out, src, vis, sigma, mu, D)
    e = y - p
    k1, k2 = kept(y, mae_t), y > mape_t
    q = (e / y).abs()
    dd = lambda v: v.double()                                                    # noqa: E731
    st = torch.stack([dd(k1).sum((0, 2, 3)), (dd(e.abs()) * k1).sum((0, 2, 3)), (dd(e) ** 2 * k1).sum((0, 2, 3)),
                      dd(k2).sum((0, 2, 3)), torch.where(k2, dd(q), torch.zeros((), dtype=torch.float64)).sum((0, 2, 3))], -1)
    ab = (lambda v: v.abs()) if absolute else (lambda v: v)                      # noqa: E731
    sn = torch.stack([torch.ones_like(dd(p)).sum((0, 3)), ab(dd(p)).sum((0, 3)), ab(dd(y)).sum((0, 3)), (dd(p) ** 2).sum((0, 3)),
                      (dd(y) ** 2).sum((0, 3)), ab(dd(p) * dd(y)).sum((0, 3))], -1)
    return st, sn


# (B, T, N, D): 20 nodes; 266 nodes (NYC_TAXI) — a second pass of the kernel's 256-node loop with 10 live threads; 513 — a third with one
METRIC_SHAPES = [(3, 12, 20, 1), (2, 12, 266, 2), (1, 3, 513, 1)]
# (mae_thresh, mape_thresh) of the shipped confs: PEMS08, METR_LA, NYC
THRESHOLDS = [(None, 0.0), (0.0, 0.0), (None, 0.001)]
NODE_VISIBLE, NODE_PLANTED = 0, 1              # with vis: truth mu at every cell of node 0; truth 0.0 (the rule) at every cell of node 1


def metric_inputs(shape, with_vis):
    """-> dict(calls=[(B_i, out_i (B_i*T*N, D), src_i (B_i, T, N, lda), vis_i or None)], out, src, vis, plant, lda): the two accumulating calls
    of a case and their concatenation.  A batch of B >= 2 samples is fed as its halves; the B = 1 shape as two batches of one sample, so that
    every launch has that shape's grid.  Node 1 is wholly planted (and, with vis, masked); with vis node 0 is wholly visible."""
    B, T, N, D = shape
    Bt = B if B >= 2 else 2
    lda = D + 2 if with_vis else D
    full = synth.make_batch(Bt, T, N, D, seed=31 + N)
    plant = plant_zeros(full, D, SHARE, seed=32 + N)
    full[:, :, NODE_PLANTED, :D] = stored_zero()
    plant[:, :, NODE_PLANTED] = True
    g = torch.Generator().manual_seed(33 + N)
    out = full[..., :D] + 0.1 * torch.randn(Bt, T, N, D, generator=g)
    vis = None
    if with_vis:
        vis = visibility((Bt, T, N, D), seed=34 + N)
        vis[:, :, NODE_VISIBLE] = 1.0
        vis[:, :, NODE_PLANTED] = 0.0
    src = full if with_vis else full[..., :D].contiguous()
    h = Bt // 2
    calls = [(hi - lo, out[lo:hi].reshape(-1, D).contiguous(), src[lo:hi].contiguous(), None if vis is None else vis[lo:hi].reshape(-1).contiguous())
             for lo, hi in ((0, h), (h, Bt))]
    return dict(calls=calls, out=out, src=src, vis=vis, plant=plant, lda=lda)


# ---- masked MAE: mae_fwd / mae_bwd (csrc/loss_adam.hip), the MAE tails (csrc/tails.hip, csrc/kl_guest.h) ---------------------------------------
def loss_ref(out, label, vis, sigma, mu, thresh):
    """oracle.gptst_oracle.mae_loss, term by term: p = inverse32(out) * M, y = inverse32(label) * M, M = 1 - vis, keep = y > thresh ->
    dict(keep, count, total = sum_keep |y - p| (fp64 sum of fp32 terms), a = d total / d out = sign(p - y) M sigma on the kept cells (fp64))"""
    M = 1.0 - vis.reshape(label.shape).float()
    p, y = inverse32(out.reshape(label.shape), sigma, mu) * M, inverse32(label, sigma, mu) * M
    keep = y > thresh
    a = (torch.sign(p - y) * M * sigma).double() * keep
    return dict(keep=keep, count=int(keep.sum()), total=float((y - p).abs().double()[keep].sum()), a=a, p=p, y=y)


def fused_count(label, vis, sigma, mu, thresh):
    """cells ONE fused multiply-add would keep (the count the rule must not return)"""
    M = 1.0 - vis.reshape(label.shape).float()
    return int((inverse_fused(label, sigma, mu) * M > thresh).sum())


LOSS_SHAPE = (3, 12, 20)                       # B, T, N of test_loss_and_kl
LOSS_CASES = [(1, 0.0), (2, 0.0), (1, 0.001), (2, 0.001)]      # (base, thresh)


def loss_inputs(base):
    """-> (out (B,T,N,base), src (B,T,N,base+2), vis (B,T,N,base), plant)"""
    B, T, N = LOSS_SHAPE
    src = synth.make_batch(B, T, N, base, seed=3)
    plant = plant_zeros(src, base, SHARE, seed=40 + base)
    g = torch.Generator().manual_seed(41 + base)
    out = torch.randn(B, T, N, base, generator=g)
    return out, src, visibility((B, T, N, base), seed=42 + base), plant


# (J, C, rows): the tail's two bodies are chosen by a library switch, not by shape (TAIL_BODIES); every case runs on both
TAIL_CASES = [(1, 64, 1000), (2, 64, 1000), (1, 128, 1000), (1, 64, 37), (2, 64, 37), (1, 128, 37)]
TAIL_THRESH = 0.0


def tail_inputs(J, C, rows):
    """-> (dec (rows,C), W (J,C), b (J), src (rows,J+2), vis (rows*J), plant (rows,J))"""
    src = synth.make_batch(1, 1, rows, J, seed=50 + rows + J).reshape(rows, J + 2).contiguous()
    plant = plant_zeros(src, J, SHARE, seed=51 + rows + J)
    g = torch.Generator().manual_seed(52 + rows + J + C)
    dec, W, b = torch.randn(rows, C, generator=g), 0.2 * torch.randn(J, C, generator=g), torch.randn(J, generator=g)
    return dec, W, b, src, visibility((rows * J,), seed=53 + rows + J), plant


def tail_ref(dec, W, b, src, vis, J, sigma, mu, thresh):
    """loss_ref on out = dec W^T + b (fp64 product, rounded to fp32), and the tail's gradients of the SUM loss in fp64:
    d_dec = a W, gW = a^T dec, gb = column sums of a"""
    out = (dec.double() @ W.double().t() + b.double()).float()
    r = loss_ref(out, src[:, :J], vis, sigma, mu, thresh)
    a = r["a"]
    r.update(out=out, d_dec=a @ W.double(), gW=a.t() @ dec.double(), gb=a.sum(0))
    return r


# ---- one fused step ---------------------------------------------------------------------------------------------------------------------
STEP_CASES = ("small_rand", "small_ada")


def step_inputs(name):
    """-> (args, B, epoch, state dict, planted src, injected mask noise, plant) of a case of step_grad_util.CASES"""
    import step_grad_util as U
    from oracle import gptst_oracle as O
    c = U.CASES[name]
    args = U.case_args(name)
    src = U.make_src(args, c["B"])
    plant = plant_zeros(src, args.input_base_dim, SHARE, seed=60)
    return args, c["B"], c["epoch"], O.init_state_dict(args, U.SD_SEED), src, U.noise_inject(args, c["B"], c["epoch"]), plant
