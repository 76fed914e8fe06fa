"""The MSDR predictor on HIP (``MSDR(..., backend="hip")``, csrc/msdr.hip, predictors/msdr_hip.py) on the GPU.  The reference of every
comparison is the torch MSDR module (pinned to the reference implementation's vectors by tests/test_predictor_msdr.py) or the step's formula,
in fp64 on the CPU; the bound is the project's element-wise one, 1e-4 of the reference tensor's largest magnitude, for every output, dX and
parameter gradient.  Measured on the reference itself, fp32 against fp64 on the CPU with the inputs used here, that error stays below 4.2e-6
at (B, N, out) = (2, 20, 1), (3, 37, 2), (1, 170, 1), (1, 266, 2): the bound leaves room for another summation order, not for an error.

The gradient of ``attlinear.bias`` is identically zero (a constant added to every logit of a softmax) — fp64 autograd leaves 1e-17, fp32 1e-8 —
so a relative error on it means nothing: those gradients (one per cell) are held to |g| <= 1e-6 max|gradient of that cell's attlinear.weight|
instead (the fp32 reference stays below 6.1e-7 of it; the HIP backend returns exactly 0).

Every comparison first moves W, b and R off their zero initialisation (msdr_util.perturb_): at the initialisation every hidden state is 0.

Step shapes: padded widths Hp 16 (one column tile: three waves skip the mix, K below one k-block), 32, 48, 64, 112 and 128 (two full slabs, K
up to 512), each under every variant of kept states, supports and row tiles; the launch's own choice of row tiles (tiles = 0) is crossed at its
boundary, 37 nodes at B = 128 (3 workgroups a sample) and 129 (2), where it must be bit-equal to the forced count it names.  Every launch
is run twice and must repeat bit for bit."""
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import msdr_util as gu
from gptst_amd import _C, graph, ops, synth
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import MSDR, msdr_hip as H
from golden_util import load
from downstream_util import _check, _err
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0


def _g(t):
    return t.float().to(DEV).contiguous()


# ---- 1. the three step launches, each alone, against their formulas ---------------------------------------------------------------------------
# (1, 266, 64): 272 padded nodes, a slab of 73 984 bytes: the forward and the second backward launch ask for more than the 64 KB of dynamic LDS
# a launch gets by default.  (2, 37, 112): Hp above 64, so a second 64-column slab pass whose last wave has no column tile, zero fill at
# col >= Hp, and a partial k-block in the second GEMM.  (1, 16, 16): one column tile, so three of the four waves skip the mix, and the second
# GEMM's K = 16 is less than one 64-wide k-block; (3, 37, 48): three column tiles, one wave idle, K = 96 .. 192; (2, 37, 128): two full
# 64-column slabs, K up to 512 — with two fixed supports and two tiles forced, 96 000 bytes of LDS on a 48-node graph
STEP_SHAPES = [(1, 16, 32), (3, 37, 64), (2, 170, 64), (1, 266, 64), (2, 37, 112), (1, 16, 16), (3, 37, 48), (2, 37, 128)]
VARIANTS = [(1, 1, 1), (4, 2, 2), (4, 1, 0), (1, 2, 2)]          # (kept states K, fixed supports, row tiles per workgroup: 0 = the kernel's choice)
T2, T1 = 2, 1                # two steps in the seq tensors, the launch works on the second: a wrong (t, b) row offset shows


def test_step_shapes_reach_beyond_64_kb_of_lds():
    v = _C.lib().value
    assert v("gptst_msdr_lds_bytes", 266, 64, 1, 2) == (272 * 68 + 16 * (3 * 64 + 4) + 16 * 68) * 4 > 73984 > 64 * 1024
    assert v("gptst_msdr_lds_bytes", 266, 64, 1, 3) > v("gptst_msdr_lds_bytes", 266, 64, 1, 2)
    assert all(v("gptst_msdr_lds_bytes", N, Hp, B, 3) <= 64 * 1024 for B, N, Hp in STEP_SHAPES[:2])
    assert v("gptst_msdr_lds_bytes", 170, 64, 2, 2) == 64768 <= 64 * 1024 < v("gptst_msdr_lds_bytes", 170, 64, 2, 3)      # two fixed supports: above, too
    assert v("gptst_msdr_groups", 266, 1, 0) == 17 and v("gptst_msdr_groups", 266, 1, 2) == 9 and v("gptst_msdr_groups", 16, 1, 2) == 1
    # the widest rows at a small graph: served, below 64 KB as the launch plans it (B = 2: one tile a workgroup) with one, two and three supports
    assert [v("gptst_msdr_lds_bytes", 37, 128, 2, ks) for ks in (1, 2, 3)] == [(48 * 68 + 16 * ((ks + 1) * 128 + 4) + 16 * 132) * 4 for ks in (1, 2, 3)]
    assert 0 < v("gptst_msdr_lds_bytes", 37, 128, 2, 3) == 54528 <= 64 * 1024 < (48 * 68 + 32 * (4 * 128 + 4) + 32 * 132) * 4 == 96000 <= H.LDS_MAX
    assert all(0 < v("gptst_msdr_lds_bytes", N, Hp, B, 3) <= 64 * 1024 for B, N, Hp in STEP_SHAPES[5:])


def _step_inputs(B, N, Hp, K, S, tiles, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)          # noqa: E731
    Np, ks = 16 * ((N + 15) // 16), S + 1
    L = rn(ks, N, N) / N ** 0.5                                                   # non-symmetric: a transposed graph shows
    Lp = torch.zeros(ks, Np, Np, dtype=torch.float64)
    Lp[:, :N, :N] = L
    G = ops.msdr_groups(N, B, tiles)
    return SimpleNamespace(L=L, Lp=_g(Lp), LpT=_g(Lp.transpose(1, 2)), ks=ks, G=G, rows=T2 * B * N, rn=rn, B=B, N=N, Hp=Hp, K=K,
                           seq=lambda x: x.view(T2, B * N, -1)[T1],                                      # the (T1, b) rows of a seq tensor
                           mixes=lambda x, Ls: torch.cat([x] + [torch.matmul(Lk, x.view(B, N, -1)).reshape(B * N, -1) for Lk in Ls], dim=1))


# each launch at one shape and variant -> (what it wrote, its errors against the fp64 formula); a repeated launch is bit-equal
def _fwd(B, N, Hp, K, S, tiles):
    s = _step_inputs(B, N, Hp, K, S, tiles, N + Hp + K)
    Wh, W2 = s.rn(Hp, (s.ks + 1) * Hp) / (3 * Hp) ** 0.5, s.rn(Hp, Hp) / Hp ** 0.5
    bvec, R, w, w2, wr = s.rn(N, Hp), s.rn(K, N, Hp), s.rn(N, Hp) / (N * Hp) ** 0.5, s.rn(N, Hp), s.rn(K)
    Gx, Hs, sig = s.rn(s.rows, Hp), s.rn(T2 + K, B * N, Hp), s.rn(T2 + K, B, s.G)
    e = sig[T1:T1 + K].sum(-1).t() + wr                                           # (B, K)
    a = torch.softmax(e, dim=1)
    xs = Hs[T1:T1 + K].view(K, B, N, Hp) + R[:, None]
    M = s.mixes(Hs[T1 + K - 1], s.L)
    c = F.leaky_relu(M @ Wh.t() + s.seq(Gx))
    o = (c @ W2.t()).view(B, N, Hp) + bvec + (a.t()[:, :, None, None] * xs).sum(0)

    def run():
        hs, sg, sg2 = _g(Hs), _g(sig), torch.full((T2 + K, B, s.G), SENT, device=DEV)
        hs[T1 + K], sg[T1 + K] = SENT, SENT
        cc, z, att = (torch.full(shape, SENT, device=DEV) for shape in ((s.rows, Hp), (s.rows, (s.ks + 1) * Hp), (T2, B, K)))
        ops.msdr_fwd_step(s.Lp, _g(Wh), _g(W2), _g(bvec), _g(R), _g(w), _g(wr), _g(Gx), hs, sg, T1, B, T2, N, w2=_g(w2), sig2=sg2, c=cc, z=z,
                          a=att, tiles=tiles)
        torch.cuda.synchronize()
        return hs, sg, sg2, cc, z, att
    (hs, sg, sg2, cc, z, att), again = run(), run()
    assert all(torch.equal(x, y) for x, y in zip((hs, sg, sg2, cc, z, att), again))
    errs = {"o": _err(hs[T1 + K], o.view(B * N, Hp)), "c": _err(s.seq(cc), c), "z": _err(s.seq(z), M), "a": _err(att[T1], a),
            "sigma": _err(sg[T1 + K].sum(-1), (o * w).sum((1, 2))), "sigma2": _err(sg2[T1 + K].sum(-1), (o * w2).sum((1, 2)))}
    keep = [i for i in range(T2 + K) if i != T1 + K]                              # nothing outside the step's own block is written
    assert torch.equal(hs[keep], _g(Hs)[keep]) and torch.equal(sg[keep], _g(sig)[keep]) and bool((sg2[keep] == SENT).all())
    assert all(bool((x.view(T2, -1)[0] == SENT).all()) for x in (cc, z, att))
    return (hs, sg, sg2, cc, z, att), errs


def _bwd_pre(B, N, Hp, K, S, tiles):
    s = _step_inputs(B, N, Hp, K, S, tiles, N + Hp + K + 1)
    W, R, Hs, dH, c = s.rn(Hp, Hp) / Hp ** 0.5, s.rn(K, N, Hp), s.rn(T2 + K, B * N, Hp), s.rn(T2 + K, B * N, Hp), s.rn(s.rows, Hp)
    dO = dH[K + T1]
    dpre = (dO @ W.t()) * torch.where(s.seq(c) > 0, 1.0, 0.01)
    xs = Hs[T1:T1 + K].view(K, B, N, Hp) + R[:, None]
    dA = (dO.view(1, B, N, Hp) * xs).sum((2, 3)).t()                              # (B, K)

    def run():
        dp, pa = torch.full((s.rows, Hp), SENT, device=DEV), torch.full((B, s.G, 8), SENT, device=DEV)
        ops.msdr_bwd_pre(_g(W), _g(R), _g(Hs), _g(dH), _g(c), dp, pa, T1, B, T2, N, tiles=tiles)
        torch.cuda.synchronize()
        return dp, pa
    (dp, pa), again = run(), run()
    assert torch.equal(dp, again[0]) and torch.equal(pa, again[1])
    assert bool((dp.view(T2, -1)[0] == SENT).all()) and bool((pa[:, :, K:] == SENT).all())
    return (dp, pa), {"dpre": _err(s.seq(dp), dpre), "dA": _err(pa[:, :, :K].sum(1), dA)}


def _bwd_state(B, N, Hp, K, S, tiles):
    s = _step_inputs(B, N, Hp, K, S, tiles, N + Hp + K + 2)
    WhT, w = s.rn(Hp, (s.ks + 1) * Hp) / (3 * Hp) ** 0.5, s.rn(N, Hp)
    a, pa, dpre, dH = torch.softmax(s.rn(T2, B, K), dim=-1), s.rn(B, s.G, 8), s.rn(s.rows, Hp), s.rn(T2 + K, B * N, Hp)
    dA = pa[:, :, :K].sum(1)
    de = a[T1] * (dA - (a[T1] * dA).sum(1, keepdim=True))                         # (B, K)
    dh = s.mixes(s.seq(dpre), s.L.transpose(1, 2)) @ WhT.t()
    want = dH.clone()
    dO = dH[K + T1].view(B, N, Hp)
    for k in range(K):
        want[T1 + k] += (a[T1][:, k, None, None] * dO + de[:, k, None, None] * w).view(B * N, Hp)
    want[T1 + K - 1] += dh

    def run():
        got, dev = _g(dH), torch.full((T2, B, K), SENT, device=DEV)
        ops.msdr_bwd_state(s.LpT, _g(WhT), _g(w), _g(a), _g(pa), _g(dpre), got, dev, T1, B, T2, N, tiles=tiles)
        torch.cuda.synchronize()
        return got, dev
    (got, dev), again = run(), run()
    assert torch.equal(got, again[0]) and torch.equal(dev, again[1])
    rest = [i for i in range(T2 + K) if not T1 <= i < T1 + K]
    assert torch.equal(got[rest], _g(dH)[rest]) and bool((dev[0] == SENT).all())
    return (got, dev), {"dH": _err(got[T1:T1 + K], want[T1:T1 + K]), "de": _err(dev[T1], de)}


@pytest.mark.parametrize("K,S,tiles", VARIANTS)
@pytest.mark.parametrize("B,N,Hp", STEP_SHAPES)
def test_step_fwd(B, N, Hp, K, S, tiles, parity):
    _check(parity, _fwd(B, N, Hp, K, S, tiles)[1])


@pytest.mark.parametrize("K,S,tiles", VARIANTS)
@pytest.mark.parametrize("B,N,Hp", STEP_SHAPES)
def test_step_bwd_pre(B, N, Hp, K, S, tiles, parity):
    _check(parity, _bwd_pre(B, N, Hp, K, S, tiles)[1])


@pytest.mark.parametrize("K,S,tiles", VARIANTS)
@pytest.mark.parametrize("B,N,Hp", STEP_SHAPES)
def test_step_bwd_state(B, N, Hp, K, S, tiles, parity):
    _check(parity, _bwd_state(B, N, Hp, K, S, tiles)[1])


@pytest.mark.parametrize("B,rule", [(128, 1), (129, 2)])
def test_the_kernel_s_own_tile_count_at_its_boundary(B, rule, parity):
    """tiles = 0 leaves the rows per workgroup to the launch: two 16-node tiles once B ceil(tiles / 2) exceeds 256.  37 nodes are 3 tiles, so
    B = 128 gives 256 (one tile a workgroup: 3 workgroups a sample) and B = 129 gives 258 (two: 2 workgroups).  Every launch of a step, left to
    the rule, writes bit for bit what it writes with that tile count forced — the partials have the rule's length — within TOL of fp64.  One
    kept state, one support, one column tile"""
    N, Hp, K, S = 37, 16, 1, 0
    assert ops.msdr_groups(N, 128, 0) == 3 and ops.msdr_groups(N, 129, 0) == 2
    assert ops.msdr_groups(N, B, 0) == ops.msdr_groups(N, B, rule) == 4 - rule != ops.msdr_groups(N, B, 3 - rule)
    for launch in (_fwd, _bwd_pre, _bwd_state):
        own, errs = launch(B, N, Hp, K, S, 0)
        forced, _ = launch(B, N, Hp, K, S, rule)
        assert all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(own, forced)), launch.__name__
        _check(parity, {launch.__name__[1:] + "." + k: v for k, v in errs.items()})


# ---- 2. whole models against fp64 torch ----------------------------------------------------------------------------------------------------
def _ap(N, ft="2000", seed=gu.SEED, **kw):
    return gu.model_args(N, graph.msdr_supports(gu.adjacency(N, seed), ft), **kw)


def _run(m, x, w):
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    y = m(xi)
    (y * w).sum().backward()
    return y.detach(), xi.grad, {k: p.grad for k, p in m.named_parameters() if not k.startswith("out.")}


def _pair(ap, C, seed, B):
    """the module on the GPU with the HIP backend, its fp64 twin on the CPU with the torch ops, a batch and a loss weight"""
    torch.manual_seed(seed)
    mh = gu.perturb_(MSDR(ap, "cpu", C, backend="hip")).to(DEV).train()
    mt = MSDR(ap, "cpu", C).double().train()
    mt.load_state_dict({k: v.detach().cpu().double() for k, v in mh.state_dict().items()}, strict=True)
    x = torch.randn(B, ap.seq_len, ap.num_nodes, C)
    w = torch.randn(B, ap.horizon, ap.num_nodes, ap.output_dim)
    return mh, mt, x, w


def _errs(got, ref):
    """y, dx and every gradient but attlinear.bias by the project's measure; those biases against their cell's weight gradient"""
    errs = {"y": _err(got[0], ref[0]), "dx": _err(got[1], ref[1])}
    assert set(got[2]) == set(ref[2])
    for k, g in ref[2].items():
        if k.endswith("attlinear.bias"):
            wmax = float(ref[2][k[:-4] + "weight"].abs().max())
            assert float(got[2][k].abs().max()) <= 1e-6 * wmax and float(g.abs().max()) <= 1e-6 * wmax, k
        else:
            assert float(g.abs().max()) > 0, k                                 # the comparison is not made where everything is zero
            errs[k] = _err(got[2][k], g)
    return errs


def _compare(mh, mt, x, w, parity):
    got = _run(mh, x.to(DEV), w.to(DEV))
    assert mh.backend_used == "hip"
    ref = _run(mt, x.double(), w.double())
    errs = _errs(got, ref)
    assert len(errs) == 2 + len(mh.cells()) * 8 + 4
    _check(parity, errs)


# (B, T, horizon, N, C, d, out, layers, K, filter_type): T < K in the last two, the last with a width that is padded (40 -> 48); one fixed
# support and two
CASES = [(2, 12, 12, 20, 64, 64, 1, 2, 4, "2000"), (3, 12, 5, 37, 64, 64, 2, 2, 4, "dual_random_walk"), (2, 3, 3, 16, 16, 32, 1, 1, 2, "dual_random_walk"),
         (1, 12, 12, 170, 64, 64, 1, 2, 4, "2000"), (2, 2, 2, 20, 64, 48, 1, 2, 4, "random_walk"),
         (2, 3, 2, 20, 32, 40, 2, 2, 4, "dual_random_walk")]


@pytest.mark.parametrize("B,T,P,N,C,d,out,layers,K,ft", CASES)
def test_whole_model_against_fp64_torch(B, T, P, N, C, d, out, layers, K, ft, parity):
    mh, mt, x, w = _pair(_ap(N, ft, T=T, horizon=P, d=d, layers=layers, K=K, out=out), C, N + T, B)
    _compare(mh, mt, x, w, parity)


@pytest.mark.parametrize("ds", ["PEMS08", "METR_LA", "NYC_BIKE", "NYC_TAXI"])
def test_shipped_msdr_configuration_against_fp64_torch(ds, parity):
    pa = predictor_args(ds, "MSDR")
    ap = SimpleNamespace(**vars(pa), supports=graph.msdr_supports(gu.adjacency(pa.num_nodes, 5, density=0.05), pa.filter_type))
    mh, mt, x, w = _pair(ap, 64, 9, 1)
    assert H.supported(mh, x.to(DEV))
    _compare(mh, mt, x, w, parity)


def test_whole_model_against_the_reference_vectors(parity):
    G = load("msdr_small.npz")
    m = MSDR(gu.model_args(20, graph.msdr_supports(G["A"], "2000")), "cpu", 64, backend="hip")
    m.load_state_dict({k[3:]: torch.tensor(G[k]) for k in G.files if k.startswith("sd.")}, strict=True)
    m = m.to(DEV).train()
    got = _run(m, torch.tensor(G["x"]).float().to(DEV), torch.tensor(G["w"]).float().to(DEV))
    assert m.backend_used == "hip"
    ref = (torch.tensor(G["y"]), torch.tensor(G["dx"]), {k[5:]: torch.tensor(G[k]) for k in G.files if k.startswith("grad.")})
    _check(parity, _errs(got, ref))


# ---- 3. the launch sequence, the padding, repeatability, the modes ------------------------------------------------------------------------------
STEP_OPS = ["msdr_fwd_step", "msdr_bwd_pre", "msdr_bwd_state"]
HOISTED = ["stgcn_tapgemm", "stgcn_wgrad", "stgcn_nodemix", "mtgnn_graphgrad"]


def _spy(monkeypatch):
    seen = {"calls": [], "kept": [], "Hs": []}

    def wrap(name):
        fn = getattr(ops, name)

        def f(*a, **kw):
            seen["calls"].append(name)
            if name == "msdr_fwd_step":
                seen["kept"].append((kw.get("c"), kw.get("z"), kw.get("a")))
                if not any(a[8] is h for h in seen["Hs"]):
                    seen["Hs"].append(a[8])
            return fn(*a, **kw)
        monkeypatch.setattr(ops, name, f)
    for n in STEP_OPS + HOISTED:
        wrap(n)
    return seen


def _sequence(T, P, layers):
    """the documented launch order of one training step: the mlp, then encoder and decoder layers bottom up; backward the other way round"""
    fwd = ["stgcn_tapgemm"]
    for steps in [T] * layers + [P] * layers:
        fwd += ["stgcn_nodemix", "stgcn_tapgemm"] + ["msdr_fwd_step"] * steps
    bwd = []
    for steps in [P] * layers + [T] * layers:
        bwd += ["msdr_bwd_pre", "msdr_bwd_state"] * steps + ["stgcn_wgrad"] * 3 + ["stgcn_tapgemm"] * 2 + ["stgcn_nodemix", "stgcn_tapgemm"]
        bwd += ["mtgnn_graphgrad"] * 2
    return fwd, bwd + ["stgcn_wgrad", "stgcn_tapgemm"]                          # (the mlp's weight and data gradient)


def test_padded_channels_repeatability_and_modes(monkeypatch):
    B, T, P, N, d = 2, 6, 4, 37, 40
    torch.manual_seed(3)
    m = gu.perturb_(MSDR(_ap(N, T=T, horizon=P, d=d), "cpu", 64, backend="hip")).to(DEV)
    x, w = torch.randn(B, T, N, 64, device=DEV), torch.randn(B, P, N, 1, device=DEV)
    seen = _spy(monkeypatch)
    m.train()
    y1, dx1, g1 = _run(m, x, w)
    fwd, bwd = _sequence(T, P, 2)
    assert m.backend_used == "hip" and seen["calls"] == fwd + bwd, seen["calls"]
    assert fwd.count("msdr_fwd_step") == 2 * (T + P) and bwd.count("msdr_bwd_pre") == bwd.count("msdr_bwd_state") == 2 * (T + P)
    assert len(seen["kept"]) == 2 * (T + P) and all(c is not None and z is not None and a is not None for c, z, a in seen["kept"])
    # every state ring: (steps + K, B N, 48) with the 8 padded channels exactly 0, the others not
    assert [h.shape[0] for h in seen["Hs"]] == [T + 4, T + 4, P + 4, P + 4] and all(h.shape[1:] == (B * N, 48) for h in seen["Hs"])
    assert all(bool((h[:, :, d:] == 0).all()) and bool((h[4:, :, :d] != 0).any()) for h in seen["Hs"])
    assert all(bool((g1[k] == 0).all()) for k in g1 if k.endswith("attlinear.bias"))
    # a second backward of the same batch: bit for bit
    y2, dx2, g2 = _run(m, x, w)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    # no_grad, and eval mode with gradients enabled: the same launches, the same output, nothing handed over to keep
    for mode in ("no_grad", "eval"):
        seen["calls"].clear(), seen["kept"].clear()
        if mode == "no_grad":
            with torch.no_grad():
                y3 = m(x)
        else:
            m.eval()
            y3 = m(x.clone().requires_grad_(True))
        assert torch.equal(y3, y1) and m.backend_used == "hip" and not y3.requires_grad and y3.grad_fn is None
        assert seen["calls"] == fwd and all(c is None and z is None and a is None for c, z, a in seen["kept"]), (mode, seen["calls"])


def test_frozen_predictor_skips_the_weight_gradients(monkeypatch):
    """parameters that take no gradient: the input's gradient is the same, bit for bit, no weight- or graph-gradient kernel is launched and the
    [h | L h] rows are not kept"""
    torch.manual_seed(3)
    m = gu.perturb_(MSDR(_ap(20, T=4, horizon=3), "cpu", 64, backend="hip")).to(DEV).train()
    x, w = torch.randn(2, 4, 20, 64, device=DEV), torch.randn(2, 3, 20, 1, device=DEV)
    want = _run(m, x, w)[1]
    for p in m.parameters():
        p.requires_grad_(False)
    seen = _spy(monkeypatch)
    xi = x.clone().requires_grad_(True)
    (m(xi) * w).sum().backward()
    assert m.backend_used == "hip" and "stgcn_wgrad" not in seen["calls"] and "mtgnn_graphgrad" not in seen["calls"] and torch.equal(xi.grad, want)
    assert seen["calls"].count("msdr_bwd_state") == 2 * 7 and all(c is not None and z is None and a is not None for c, z, a in seen["kept"])


@pytest.mark.parametrize("kw,C", [(dict(pre_v=2), 64), (dict(mds=2), 64), (dict(), 24)])
def test_unsupported_input_takes_the_torch_path(kw, C):
    torch.manual_seed(4)
    ap = _ap(20, T=3, horizon=3, **kw)
    mh = gu.perturb_(MSDR(ap, "cpu", C, backend="hip")).to(DEV)
    mt = MSDR(ap, "cpu", C).to(DEV)
    mt.load_state_dict(mh.state_dict(), strict=True)
    x = torch.randn(2, 3, 20, C, device=DEV)
    assert not H.supported(mh, x)
    yh, yt = mh(x), mt(x)
    assert mh.backend_used == "torch" and mt.backend_used == "torch" and torch.equal(yh, yt)


def test_lds_plan_depends_on_the_batch_and_the_module_serves_both(parity):
    """N = 500: one row tile per workgroup fits the 160 KB of LDS (156 160 bytes), the two tiles a batch of 17 would get do not: that batch takes
    the torch ops, bit-equal to a torch-backend twin, and the same module serves the next small batch on HIP again"""
    v = _C.lib().value
    assert 0 < v("gptst_msdr_lds_bytes", 500, 64, 1, 2) == 156160 <= H.LDS_MAX < v("gptst_msdr_lds_bytes", 500, 64, 17, 2)
    torch.manual_seed(6)
    ap = _ap(500, T=2, horizon=2, layers=1, K=2)
    mh = gu.perturb_(MSDR(ap, "cpu", 16, backend="hip")).to(DEV).train()
    mt = MSDR(ap, "cpu", 16).to(DEV).train()
    mt.load_state_dict(mh.state_dict(), strict=True)
    xb = torch.randn(17, 2, 500, 16, device=DEV)
    assert not H.supported(mh, xb) and H.supported(mh, xb[:1])
    yh, yt = mh(xb), mt(xb)
    assert mh.backend_used == "torch" and torch.equal(yh, yt)
    ys = mh(xb[:1])
    assert mh.backend_used == "hip"
    _check(parity, {"y": _err(ys, mt(xb[:1]))})


# ---- 4. the chain --------------------------------------------------------------------------------------------------------------------------
def _front_end(tmp_path, backend, finetune, sd):
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    N = 20
    args = make_args("PEMS08", mode="eval", num_nodes=N, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros(), batch_size=8, epochs=3,
                     early_stop=False, log_dir=str(tmp_path), debug=True, model="MSDR_test", msdr_backend=backend)
    sd = O.init_state_dict(args, 4) if sd is None else sd
    torch.manual_seed(0)
    pred = gu.perturb_(MSDR(_ap(N, out=args.output_dim), "cpu", args.hidden_dim, backend=args.msdr_backend))
    model = EnhanceFrontEnd(args, predictor=pred, finetune_encoder=finetune).to(DEV)
    model.load_pretrained_model(sd)
    return args, sd, model, EvalTrainer


@pytest.mark.parametrize("finetune", [False, True])
def test_chain_one_step_agrees_with_the_torch_backend(tmp_path, finetune, parity):
    args, sd, mh, ET = _front_end(tmp_path, "hip", finetune, None)
    _, _, mt, _ = _front_end(tmp_path, "torch", finetune, sd)
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
        if k.endswith("attlinear.bias"):
            wmax = float(res["torch"][1][k[:-4] + "weight"].abs().max())
            assert float(res["hip"][1][k].abs().max()) <= 1e-6 * wmax, k
        else:
            errs[k] = _err(res["hip"][1][k], g)
    _check(parity, errs)


def test_eval_trainer_learns_on_the_hip_backend(tmp_path):
    from gptst_amd import data as gdata
    args, sd, model, ET = _front_end(tmp_path, "hip", False, None)
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
