"""The MTGNN predictor on HIP (``MTGNN(..., backend="hip")``, csrc/mtgnn.hip, predictors/mtgnn_hip.py) on the GPU.  The reference of every
comparison is fp64 torch on the CPU: ``F.conv2d`` and autograd for the tap GEMM family, ``einsum`` for the graph gradient, the torch MTGNN module
(pinned to the reference implementation's vectors by tests/test_predictor_mtgnn.py) for the whole model.  The bound is the project's element-wise
one, 1e-4 of the reference tensor's largest magnitude, for every output, dX and parameter gradient.  The shapes are the smallest at which a
kernel can still go wrong (odd N, N of exactly one tile, several workgroups, K beyond one LDS chunk), not the workload's; the cases with a PLANS
entry, ``test_graphgrad_several_steps`` and the shipped configurations are the smallest at which the launch plans take the paths of a real
batch (two tiles per wave, several chunks or units per split, a second grid-stride pass), and each asserts that it is on its path first."""
import functools
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gptst_amd import _C, graph, ops, synth
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import MTGNN, mtgnn_hip as H
from golden_util import load
from mtgnn_util import clear_topk_cuts, same_support
from downstream_util import _check, _err
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _g(t):
    return None if t is None else t.float().to(DEV).contiguous()


def _guarded(rows, width):
    """a (rows, width) block inside a buffer of 7.0: what a launch writes outside its block shows"""
    big = torch.full((rows + 32, width), 7.0, device=DEV)
    return big, big[16:16 + rows]


def _intact(big):
    return bool((big[:16] == 7).all()) and bool((big[-16:] == 7).all())


# ---- 1. the tap GEMM between two frames, its data backward, weight gradient and gate backward -----------------------------------------------
#            B  Tsrc Tdst N  ci  co  offs                gated  zero pattern  keep   accumulate  operand mask
TAP_CASES = {
    "inception":      (2, 19, 13, 20, 32, 32, tuple(range(7)), True, True, False, False, False),
    "inception_keep": (2, 19, 13, 20, 32, 32, tuple(range(7)), True, True, True, False, False),
    "dilated":        (1, 13, 7, 16, 16, 16, (0, 2, 4, 6), True, False, False, False, False),
    "skip":           (3, 13, 1, 37, 32, 64, tuple(range(13)), False, False, False, True, False),
    "skip0":          (2, 20, 1, 20, 64, 64, tuple(range(20)), False, False, False, False, False),
    "skip0_dropout":  (2, 20, 1, 20, 64, 64, tuple(range(20)), False, False, False, False, True),
    "one_tap":        (2, 2, 2, 37, 32, 64, (0,), False, False, False, False, False),
    # two row tiles per wave (mt_tapgemm_kernel<2>), several 64-row chunks per split of the weight gradient, a second grid-stride pass of the
    # gate backward: what every real batch takes.  N = 461 and 253 are no multiples of 16
    "wide_tpw2":      (3, 13, 12, 461, 16, 128, (0, 1), True, False, False, False, False),
    "wide_tpw2_b6":   (6, 13, 12, 461, 16, 128, (0, 1), True, False, False, False, False),
    "inception_tpw2": (20, 19, 13, 253, 32, 32, tuple(range(7)), True, True, True, False, False),       # the workload's layer 0 at B = 20
    "wgrad_cw256":    (2, 19, 13, 193, 32, 128, tuple(range(7)), True, False, False, False, False),    # 79 chunks, 40 splits, the last of one
}
# what the launch plans must make of a case (absent: one iteration everywhere, as in the cases above the comment): tiles per wave of the
# forward and of the mirrored data backward, chunks per split of the weight gradient at least, and whether the gate backward makes a second pass
PLANS = {
    "wide_tpw2":      dict(fwd=2, bwd=1, cps=2, gate2=False),
    "wide_tpw2_b6":   dict(fwd=2, bwd=1, cps=3, gate2=True),
    "inception_tpw2": dict(fwd=2, bwd=2, cps=5, gate2=False),
    "wgrad_cw256":    dict(fwd=1, bwd=1, cps=2, gate2=False),
}
ONE_PASS = dict(fwd=1, bwd=1, cps=1, gate2=False)


def _plan(c):
    """the same four figures from the library: the plan query of include/gptst_hip_testing.h, the split rule, the grid of the gate backward"""
    v = _C.lib().value
    ns = v("gptst_stgcn_wgrad_nsplit", c.rows, c.cw, c.ntap * c.ci)
    nchunks = -(-c.rows // 64)
    return dict(fwd=v("gptst_mtgnn_tapgemm_tpw", c.rows, c.co, int(c.gated)), bwd=v("gptst_mtgnn_tapgemm_tpw", c.srows, c.ci, 0),
                cps=-(-nchunks // ns), gate2=c.gated and c.rows * c.co // 4 > 4096 * 256)


@functools.lru_cache(maxsize=None)
def _tap_case(name):
    """the case's operands and its fp64 results: Y by F.conv2d, dX / dW / db of sum(Y G) by autograd.  Computed once, shared, never written to"""
    B, Tsrc, Tdst, N, ci, co, offs, gated, pattern, keep, accum, xmask = TAP_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)          # noqa: E731
    ntap, cw = len(offs), (2 * co if gated else co)
    W = rn(cw, ntap, ci) / (ntap * ci) ** 0.5 * (2.0 if gated else 1.0)
    if pattern:                                                                  # the four inception kernels, right-aligned: 2, 3, 6, 7 taps
        for half in (0, co):
            for q, kern in enumerate((2, 3, 6, 7)):
                W[half + q * co // 4:half + (q + 1) * co // 4, :ntap - kern] = 0
    c = SimpleNamespace(B=B, Tsrc=Tsrc, Tdst=Tdst, N=N, ci=ci, co=co, offs=offs, gated=gated, ntap=ntap, cw=cw, accum=accum,
                        rows=B * Tdst * N, srows=B * Tsrc * N)
    c.X, c.b, c.G = rn(c.srows, ci), rn(cw), rn(c.rows, co)
    c.W = W.reshape(cw, ntap * ci)
    c.OM = (torch.rand(c.rows, co, dtype=torch.float64, generator=g) > 0.3).double() / 0.7 if keep else None
    c.XM = (torch.rand(c.srows, ci, dtype=torch.float64, generator=g) > 0.3).double() / 0.7 if xmask else None
    c.Y0 = rn(c.rows, co) if accum else None
    c.Rg = rn(c.rows, ci)                                                        # a second gradient for the data backward's epilogue
    X, Wl, b = c.X.clone().requires_grad_(True), c.W.clone().requires_grad_(True), c.b.clone().requires_grad_(True)
    xin = (X if c.XM is None else X * c.XM).view(B, Tsrc, N, ci).permute(0, 3, 2, 1)               # (B, ci, N, Tsrc)
    d = offs[1] - offs[0] if ntap > 1 else 1
    assert offs == tuple(d * j for j in range(ntap))
    pre = F.conv2d(xin, Wl.view(cw, ntap, ci).permute(0, 2, 1).unsqueeze(2), b, dilation=(1, d))   # (B, cw, N, Tdst)
    assert pre.shape[3] == Tdst
    pre = pre.permute(0, 3, 2, 1).reshape(c.rows, cw)
    if gated:
        c.tn, c.s = torch.tanh(pre[:, :co]).detach(), torch.sigmoid(pre[:, co:]).detach()
        Y = torch.tanh(pre[:, :co]) * torch.sigmoid(pre[:, co:])
        Y = Y if c.OM is None else Y * c.OM
    else:
        Y = pre if c.Y0 is None else pre + c.Y0
    (Y * c.G).sum().backward()
    c.Y, c.dX, c.dW, c.db = Y.detach(), X.grad, Wl.grad, b.grad
    return c


@pytest.mark.parametrize("name", list(TAP_CASES))
def test_tapgemm_forward(name, parity):
    c = _tap_case(name)
    assert _plan(c) == PLANS.get(name, ONE_PASS), _plan(c)
    big, Y = _guarded(c.rows, c.co)
    args = (_g(c.X), _g(c.W), _g(c.b), c.offs, c.B, c.Tsrc, c.Tdst, c.N)
    if c.gated:
        _, tn, s = ops.mtgnn_tapgemm(*args, gated=True, omask=_g(c.OM), out=Y, keep=True)
        _check(parity, {"y": _err(Y, c.Y), "tanh": _err(tn, c.tn), "sigmoid": _err(s, c.s)})
        Y2 = ops.mtgnn_tapgemm(*args, gated=True, omask=_g(c.OM))                 # nothing kept: the same bits
        assert torch.equal(Y2, Y)
    else:
        if c.accum:
            Y.copy_(_g(c.Y0))                                                     # accumulation onto a non-zero Y, in place
        ops.mtgnn_tapgemm(*args, xmask=_g(c.XM), res=Y if c.accum else None, out=Y)
        _check(parity, {"y": _err(Y, c.Y)})
    assert _intact(big)


@pytest.mark.parametrize("name", list(TAP_CASES))
def test_tapgemm_backward(name, parity):
    """dPre (the gate's backward from the kept tanh and sigmoid), dW of every tap (the zero-pattern taps too) and db, dX with a second
    gradient added in the epilogue at the residual's offset; a second run gives the same bits"""
    c = _tap_case(name)
    assert _plan(c) == PLANS.get(name, ONE_PASS), _plan(c)
    X, W, XM = _g(c.X), _g(c.W), _g(c.XM)

    def run():
        dPre = ops.mtgnn_gate_bwd(_g(c.G), _g(c.tn), _g(c.s), _g(c.OM)) if c.gated else _g(c.G)
        dW, db = ops.mtgnn_wgrad(dPre, X, c.offs, c.B, c.Tsrc, c.Tdst, c.N, xmask=XM)
        big, dX = _guarded(c.srows, c.ci)
        ops.mtgnn_tapgemm(dPre, H._mirror(W, c.ntap), None, tuple(-o for o in c.offs), c.B, c.Tdst, c.Tsrc, c.N, omask=XM,
                          res=None if XM is not None else _g(c.Rg), res_frame=c.Tdst, res_off=c.Tdst - c.Tsrc, out=dX)
        assert _intact(big)
        return dW, db, dX
    dW, db, dX = run()
    want = c.dX
    if c.XM is None:                                                              # + Rg at the last Tdst steps of the source frame
        want = want + F.pad(c.Rg.view(c.B, c.Tdst, c.N * c.ci), (0, 0, c.Tsrc - c.Tdst, 0)).reshape(c.srows, c.ci)
    errs = {"dX": _err(dX, want), "db": _err(db, c.db)}
    for j in range(c.ntap):
        wj = c.dW.view(c.cw, c.ntap, c.ci)[:, j]
        if float(wj.abs().max()) > 0:
            errs["dW%d" % j] = _err(dW.view(c.cw, c.ntap, c.ci)[:, j], wj)
    _check(parity, errs)
    assert all(torch.equal(a, b) for a, b in zip(run(), (dW, db, dX)))


# ---- 2. the gradient of the node mix with respect to its graphs -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,unit_list", [(16, (1, 5, 26)), (20, (1, 5, 26)), (37, (1, 5, 26)), (170, (1,))])
def test_graphgrad(N, unit_list, parity):
    """random non-symmetric data: a transposed result or a read into the neighbouring unit's rows (N is no multiple of 16) shows"""
    g = torch.Generator().manual_seed(N)
    errs = {}
    for units in unit_list:
        for c in (16, 32):
            for ks in (1, 4):
                D = torch.randn(units * N, 16 + ks * c, dtype=torch.float64, generator=g)
                X = torch.randn(units * N, c, dtype=torch.float64, generator=g)
                want = torch.einsum("uvkc,uwc->kvw", D[:, 16:].view(units, N, ks, c), X.view(units, N, c))
                got = ops.mtgnn_graphgrad(_g(D), _g(X), N, c, ks, dcol0=16)
                assert got.shape == (ks, N, N)
                errs["u%d c%d ks%d" % (units, c, ks)] = _err(got, want)
                assert torch.equal(ops.mtgnn_graphgrad(_g(D), _g(X), N, c, ks, dcol0=16), got)
    _check(parity, errs)


#            N  units ks  c   units per split, and whether the last split is shorter
GG_STEPS = [(170, 57, 4, 32, 3, False), (170, 58, 4, 32, 3, True), (37, 600, 4, 16, 3, False), (37, 1, 4, 64, 1, False)]


@pytest.mark.parametrize("N,units,ks,c,ups,ragged", GG_STEPS)
def test_graphgrad_several_steps(N, units, ks, c, ups, ragged, parity):
    """a workgroup's register-prefetch pipeline (the next stage's loads beside this stage's MFMAs) over two stages and more: several units per
    split (36 and 4 tiles of 64 x 64 per split against 1024 workgroups), or the two 32-channel groups of c = 64 alone.  Every case above
    this one has one unit per split and c <= 32, so one stage"""
    ns = _C.lib().value("gptst_mtgnn_graphgrad_nsplit", units, N, ks)
    got_ups = -(-units // ns)
    steps = got_ups * (-(-c // 32))
    assert got_ups == ups and steps >= 2 and (units - (ns - 1) * ups < ups) == ragged, (ns, got_ups, steps)
    g = torch.Generator().manual_seed(N + units)
    D = torch.randn(units * N, 16 + ks * c, dtype=torch.float64, generator=g)
    X = torch.randn(units * N, c, dtype=torch.float64, generator=g)
    want = torch.einsum("uvkc,uwc->kvw", D[:, 16:].view(units, N, ks, c), X.view(units, N, c))
    got = ops.mtgnn_graphgrad(_g(D), _g(X), N, c, ks, dcol0=16)
    assert got.shape == (ks, N, N)
    _check(parity, {"u%d c%d ks%d" % (units, c, ks): _err(got, want)})
    assert torch.equal(ops.mtgnn_graphgrad(_g(D), _g(X), N, c, ks, dcol0=16), got)


# ---- 3. the whole model ----------------------------------------------------------------------------------------------------------------------
CONF = dict(input_window=12, output_window=12, gcn_true=True, buildA_true=True, gcn_depth=2, node_dim=40, dilation_exponential=1,
            conv_channels=32, residual_channels=32, skip_channels=64, end_channels=128, layers=3, propalpha=0.05, tanhalpha=3,
            layer_norm_affline=True, use_curriculum_learning=True, task_level=0, adj_mx=None)


def _ap(N, out=1, k=20, p=0.3, **kw):
    return SimpleNamespace(num_nodes=N, output_dim=out, subgraph_size=min(k, N), dropout=p, **{**CONF, **kw})


def _run(m, x, w):
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    y = m(xi)
    (y * w).sum().backward()
    return y.detach(), xi.grad, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def _masks(m, B, p, seed):
    """one dropout multiplier per site in the rows' layout (B, T, N, C), fp64 on the CPU; None when p = 0"""
    if p == 0:
        return None
    g = torch.Generator().manual_seed(seed)
    shapes = {"in": (B, m.total_window, m.num_nodes, m.feature_dim)}
    shapes.update({"l%d" % i: (B, m.frames[i + 1], m.num_nodes, m.conv_channels) for i in range(m.layers)})
    return {k: (torch.rand(s, dtype=torch.float64, generator=g) >= p).double() / (1 - p) for k, s in shapes.items()}


def _inject(m, masks, rows_layout):
    """replace the module's dropout hook: the same masks for both modules, permuted into the torch module's (B, C, N, T)"""
    if masks is None:
        m._keep = lambda tag, like: None
    elif rows_layout:
        dev = {k: _g(v) for k, v in masks.items()}
        m._keep = lambda tag, like: dev[tag]
    else:
        m._keep = lambda tag, like: masks[tag].permute(0, 3, 2, 1)


@functools.lru_cache(maxsize=None)
def _model_pair(B, N, out, k, p, C=64, ds=None):
    """the torch module in fp64 on the CPU (default init; biases and LayerNorm weights moved off 0 / 1; no tie at a top-k cut), its HIP twin, a
    batch, and the fp64 results.  ds: the predictor's arguments are those of conf/MTGNN/<ds>.conf (and N, out, k, p must be its values)"""
    torch.manual_seed(7 + N + out)
    ap = _ap(N, out, k, p)
    if ds is not None:
        ap = SimpleNamespace(**vars(predictor_args(ds, "MTGNN")), adj_mx=np.asarray(graph.synthetic_adjacency(N, 2), dtype=np.float32))
        assert (ap.num_nodes, ap.output_dim, ap.subgraph_size, ap.dropout) == (N, out, k, p)
    m64 = MTGNN(ap, "cpu", C, out).double().train()
    with torch.no_grad():
        for name, q in m64.named_parameters():
            if name.startswith("norm.") or name.endswith(".bias"):
                q.add_(0.2 * torch.randn_like(q))
    if k < N:
        clear_topk_cuts(m64.gc, k)
    x64, w64 = torch.randn(B, 12, N, C, dtype=torch.float64), torch.randn(B, 12, N, out, dtype=torch.float64)
    masks = _masks(m64, B, p, N)
    _inject(m64, masks, False)
    ref = _run(m64, x64, w64)
    m = MTGNN(ap, DEV, C, out, backend="hip").to(DEV).train()
    m.load_state_dict({n: v.float() for n, v in m64.state_dict().items()}, strict=True)
    _inject(m, masks, True)
    return m, m64, _g(x64), _g(w64), ref


def _errs(got, ref):
    errs = {"y": _err(got[0], ref[0]), "dx": _err(got[1], ref[1])}
    assert set(got[2]) == set(ref[2]) and len(ref[2]) == 94 - 6 and not any(k.startswith("residual_convs.") for k in got[2])
    for k, g in ref[2].items():
        errs[k] = _err(got[2][k], g)
    return errs


CASES = [(2, 20, 1, 20), (3, 37, 2, 37), (2, 37, 1, 8), (1, 170, 1, 20)]


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("B,N,out,k", CASES)
def test_whole_model_against_fp64_torch(B, N, out, k, p, parity):
    m, m64, x, w, ref = _model_pair(B, N, out, k, p)
    if k < N:                                            # a precondition on the input: both precisions keep the same top-k set
        with torch.no_grad():
            assert same_support(m.adjacency(), m64.adjacency())
    got = _run(m, x, w)
    assert m.backend_used == "hip" and got[0].shape == (B, 12, N, out)
    _check(parity, _errs(got, ref))


@pytest.mark.parametrize("ds,N,out,k", [("METR_LA", 207, 1, 20), ("NYC_BIKE", 250, 2, 40), ("NYC_TAXI", 266, 2, 20)])
def test_shipped_mtgnn_configuration_against_fp64_torch(ds, N, out, k, parity):
    """the predictor as ``-mode eval -model MTGNN`` builds it from conf/MTGNN/<dataset>.conf (NYC_BIKE: subgraph_size 40, end_channels 64) over
    a synthetic adjacency, one batch element of the 64-wide embedding, the conf's dropout 0.3 with injected masks"""
    m, m64, x, w, ref = _model_pair(1, N, out, k, 0.3, 64, ds)
    assert (m.end_conv_1.out_channels == 64) == (ds == "NYC_BIKE")
    with torch.no_grad():                                # a precondition on the input: both precisions keep the same top-k set
        assert same_support(m.adjacency(), m64.adjacency())
    got = _run(m, x, w)
    assert m.backend_used == "hip" and got[0].shape == (1, 12, N, out)
    _check(parity, _errs(got, ref))


@pytest.mark.parametrize("mode", ["eval_vectors", "train_vectors"])
def test_whole_model_against_the_reference_vectors(mode, parity):
    """tests/golden/mtgnn_small.npz: the eval-mode vectors (dropout off; the HIP path needs train() for a backward, so its hook returns no
    mask) and the training-mode vectors, whose masks are what the seeded CPU stream gives for the reference's tensors, in its order"""
    G = load("mtgnn_small.npz")
    cfg = dict(conv_channels=16, residual_channels=16, skip_channels=16, end_channels=32, adj_mx=G["A"])
    m = MTGNN(_ap(20, 2, 8, 0.3, **cfg), DEV, 16, 2, backend="hip").to(DEV).train()
    sd = {k[3:]: torch.tensor(G[k]) for k in G.files if k.startswith("sd.")}
    m.load_state_dict(sd, strict=True)
    cpu = MTGNN(_ap(20, 2, 8, 0.3, **cfg), "cpu", 16, 2)
    cpu.load_state_dict(sd, strict=True)
    with torch.no_grad():
        assert same_support(m.adjacency(), cpu.adjacency())
    tag = ""
    if mode == "eval_vectors":
        m._keep = lambda tag, like: None
    else:
        tag = "train."
        torch.manual_seed(int(G["train_seed"]))
        shapes = [("in", (2, 16, 20, 20))] + [("l%d" % i, (2, 16, 20, t)) for i, t in enumerate((14, 8, 2))]
        masks = {k: F.dropout(torch.ones(s), 0.3, True).permute(0, 3, 2, 1).contiguous().to(DEV) for k, s in shapes}
        m._keep = lambda tag, like: masks[tag]
    got = _run(m, torch.tensor(G["x"], device=DEV), torch.tensor(G["w"], device=DEV))
    assert m.backend_used == "hip"
    ref = (torch.tensor(G[tag + "y"]), torch.tensor(G[tag + "dx"]), {k: torch.tensor(G[tag + "grad." + k]) for k in got[2]})
    _check(parity, _errs(got, ref))


# ---- 4. repeatability, modes, frozen parameters, the fallback ---------------------------------------------------------------------------------
LAUNCHES = ("mtgnn_tapgemm", "mtgnn_gate_bwd", "mtgnn_wgrad", "mtgnn_graphgrad", "stgcn_nodemix", "stgcn_tapgemm", "stgcn_wgrad",
            "stgcn_ln_fwd", "stgcn_ln_bwd", "stgcn_ln_bwd_param")
FWD = ["mtgnn_tapgemm"] * 2 + ["mtgnn_tapgemm", "stgcn_nodemix", "mtgnn_tapgemm", "mtgnn_tapgemm", "stgcn_ln_fwd"] * 3 + ["mtgnn_tapgemm"]


def _spy(monkeypatch):
    """every launch wrapper the backend calls, in order, and whether a launch was asked to keep something for a backward"""
    seen = {"calls": [], "kept": []}

    def wrap(name):
        fn = getattr(ops, name)

        def f(*a, **kw):
            seen["calls"].append(name)
            if kw.get("keep"):
                seen["kept"].append(name)
            return fn(*a, **kw)
        monkeypatch.setattr(ops, name, f)
    for n in LAUNCHES:
        wrap(n)
    return seen


def test_repeatability_and_modes(monkeypatch):
    torch.manual_seed(3)
    B, N = 2, 37
    m = MTGNN(_ap(N, 2, 8), DEV, 64, 2, backend="hip").to(DEV).train()
    masks = _masks(m, B, 0.3, 1)
    _inject(m, masks, True)
    x, w = torch.randn(B, 12, N, 64, device=DEV), torch.randn(B, 12, N, 2, device=DEV)
    seen = _spy(monkeypatch)
    y1, dx1, g1 = _run(m, x, w)
    assert m.backend_used == "hip" and seen["calls"][:len(FWD)] == FWD, seen["calls"]
    assert seen["kept"] == ["mtgnn_tapgemm", "stgcn_ln_fwd"] * 3
    for name in ("mtgnn_gate_bwd", "mtgnn_wgrad", "mtgnn_graphgrad", "stgcn_wgrad", "stgcn_ln_bwd", "stgcn_ln_bwd_param"):
        assert name in seen["calls"][len(FWD):], name
    # a second backward of the same batch: bit for bit
    y2, dx2, g2 = _run(m, x, w)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    # no_grad (the same masks), and eval mode with gradients enabled (dropout off): the forward's launches only, nothing kept, no graph
    seen["calls"].clear(), seen["kept"].clear()
    with torch.no_grad():
        y3 = m(x)
    assert torch.equal(y3, y1) and seen["calls"] == FWD and not seen["kept"] and not y3.requires_grad
    _inject(m, None, True)
    y4 = _run(m, x, w)[0]                                                          # training mode without masks: what eval mode computes
    m.eval()
    del m._keep                                                                    # the module's own hook: no mask in eval mode
    seen["calls"].clear(), seen["kept"].clear()
    y5 = m(x.clone().requires_grad_(True))
    assert torch.equal(y5, y4) and m.backend_used == "hip" and seen["calls"] == FWD and not seen["kept"]
    assert not y5.requires_grad and y5.grad_fn is None


def test_default_hook_draws_dropout_on_the_hip_path():
    """training mode with the module's own hook: masks are drawn (two passes differ), the scale is 1 / (1 - p), and the pass is repeatable
    from a seed"""
    torch.manual_seed(5)
    m = MTGNN(_ap(20, 1, 20), DEV, 64, 1, backend="hip").to(DEV).train()
    x = torch.randn(2, 12, 20, 64, device=DEV)
    keep = m._keep("l0", x.new_empty(2, 13, 20, 32))
    vals = keep.unique().tolist()
    assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] - 1 / 0.7) < 1e-6 and 0.6 < float((keep > 0).float().mean()) < 0.8
    torch.manual_seed(9)
    ya = m(x)
    yb = m(x)
    torch.manual_seed(9)
    yc = m(x)
    assert m.backend_used == "hip" and not torch.equal(ya, yb) and torch.equal(ya, yc)


def test_frozen_predictor_skips_the_parameter_gradients(monkeypatch):
    """parameters that take no gradient: the input's gradient is the same, bit for bit, and no weight-gradient or graph-gradient kernel runs"""
    torch.manual_seed(3)
    m = MTGNN(_ap(20, 1, 8, 0.0), DEV, 64, 1, backend="hip").to(DEV).train()
    x, w = torch.randn(2, 12, 20, 64, device=DEV), torch.randn(2, 12, 20, 1, device=DEV)
    want = _run(m, x, w)[1]
    for p in m.parameters():
        p.requires_grad_(False)
    seen = _spy(monkeypatch)
    xi = x.clone().requires_grad_(True)
    (m(xi) * w).sum().backward()
    assert m.backend_used == "hip" and torch.equal(xi.grad, want)
    assert not {"mtgnn_wgrad", "stgcn_wgrad", "mtgnn_graphgrad", "stgcn_ln_bwd_param"} & set(seen["calls"]), seen["calls"]


def test_unsupported_width_takes_the_torch_path():
    torch.manual_seed(4)
    mh, mt = MTGNN(_ap(20), DEV, 24, 1, backend="hip").to(DEV), MTGNN(_ap(20), DEV, 24, 1).to(DEV)
    mt.load_state_dict(mh.state_dict(), strict=True)
    x = torch.randn(2, 12, 20, 24, device=DEV)
    assert not H.supported(mh, x)
    torch.manual_seed(6)
    yh = mh(x)
    torch.manual_seed(6)
    yt = mt(x)
    assert mh.backend_used == "torch" and mt.backend_used == "torch" and torch.equal(yh, yt)


# ---- 5. the chain ----------------------------------------------------------------------------------------------------------------------------
def _front_end(tmp_path, backend, finetune, sd, p):
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    N = 20
    args = make_args("PEMS08", mode="eval", num_nodes=N, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros(), batch_size=8, epochs=3,
                     early_stop=False, log_dir=str(tmp_path), debug=True, model="MTGNN_test", mtgnn_backend=backend)
    sd = O.init_state_dict(args, 4) if sd is None else sd
    torch.manual_seed(0)
    pred = MTGNN(_ap(N, args.output_dim, 8, p), DEV, args.hidden_dim, args.output_dim, backend=args.mtgnn_backend)
    model = EnhanceFrontEnd(args, predictor=pred, finetune_encoder=finetune).to(DEV)
    model.load_pretrained_model(sd)
    return args, sd, model, EvalTrainer


@pytest.mark.parametrize("finetune", [False, True])
def test_chain_one_step_agrees_with_the_torch_backend(tmp_path, finetune, parity):
    """(dropout 0: the two backends draw their masks from different streams)"""
    args, sd, mh, ET = _front_end(tmp_path, "hip", finetune, None, 0.0)
    _, _, mt, _ = _front_end(tmp_path, "torch", finetune, sd, 0.0)
    mt.load_state_dict(mh.state_dict(), strict=True)
    src = synth.make_batch(2, 12, 20, 1, interval=args.interval, seed=21).to(DEV)
    tgt = synth.make_batch(2, 12, 20, 1, interval=args.interval, seed=22, start_slot=12).to(DEV)
    res = {}
    for name, model in (("hip", mh), ("torch", mt)):
        tr = ET(model, args, None, None, None, synth.SCALER_MEAN, synth.SCALER_STD)
        tr.logger.setLevel(logging.WARNING)
        model.train()
        loss = tr._loss(model(src, tgt)[0], tgt)
        loss.backward()
        assert model.predictor.backend_used == name
        res[name] = (float(loss.detach()), {k: p.grad for k, p in model.named_parameters() if p.requires_grad and p.grad is not None})
    assert set(res["hip"][1]) == set(res["torch"][1])
    assert any(k.startswith("pretrain_model.") for k in res["hip"][1]) == finetune
    errs = {"loss": abs(res["hip"][0] - res["torch"][0]) / abs(res["torch"][0])}
    for k, g in res["torch"][1].items():
        errs[k] = _err(res["hip"][1][k], g)
    _check(parity, errs)


def test_eval_trainer_learns_on_the_hip_backend(tmp_path):
    """three epochs with ``-mtgnn_backend hip`` and the conf's dropout 0.3 active"""
    from gptst_amd import data as gdata
    args, sd, model, ET = _front_end(tmp_path, "hip", False, None, 0.3)
    raw = synth.make_series(20, 3, days=6, seed=3)
    train, val, test, scaler, _, _ = gdata.get_dataloader(args, device=DEV, raw=raw, generator=torch.Generator().manual_seed(1))
    tr = ET(model, args, train, val, test, float(scaler.mean), float(scaler.std))
    tr.logger.setLevel(logging.WARNING)
    losses = [tr.train_epoch(e) for e in (1, 2, 3)]
    assert model.predictor.backend_used == "hip"
    assert losses[2] < losses[0] and all(np.isfinite(losses)), losses
    rows = tr.test(test)
    assert model.predictor.backend_used == "hip"
    assert rows.shape == (13, 4) and bool(torch.isfinite(rows[:, :3]).all())
