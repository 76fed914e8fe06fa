"""The ST-WA predictor on HIP (``STWA(..., backend="hip")``, csrc/stwa.hip, predictors/stwa_hip.py) on the GPU.  The reference of every
comparison is the torch STWA module (pinned to the reference implementation's vectors by tests/test_predictor_stwa.py) or a cut's formula
(stwa_util.cut_local / cut_spatial, shown to be the module's Layer by tests/test_stwa_hip_cpu.py), in fp64 on the CPU with the same noise; the
bound is the project's element-wise one, 1e-4 of the reference tensor's largest magnitude, for every output, dX and parameter gradient.
fp32 torch against fp64 torch stays below 7.5e-6 at every whole-model input used here, and every such input leaves the spatial softmax at
2.8 - 9.4 x 1 / N (tests/test_predictor_stwa.py::test_every_gpu_input_is_sharp_and_within_fp32_reach asserts both on the CPU).

21 gradients are identically zero (stwa_util.degenerate): they are held to |g| <= 1e-6 of the model's largest gradient magnitude (fp32
torch leaves at most 2.3e-8 of it at these inputs; the HIP path leaves the temporal key's bias generator and the spatial key's common bias
at exactly 0).

Every comparison starts from stwa_util.perturb_ (the generators' last Linears x 3).  Every launch is run twice and must repeat bit for bit."""
import logging

import numpy as np
import pytest
import torch

import stwa_util as su
from gptst_amd import _C, ops, synth
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import STWA, stwa_hip as H
from golden_util import load
from downstream_util import _check, _err
from oracle import gptst_oracle as O
from types import SimpleNamespace

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0


def _g(t):
    return t.detach().float().to(DEV).contiguous()


def _sent(*shape):
    return torch.full(shape, SENT, device=DEV)


# ---- 1. the five launches of a cut, each alone, against their formulas ---------------------------------------------------------------------
# (1, 16, 16): one tile; (3, 37, 16): a ragged last tile; (2, 170, 16); (1, 266, 16): 119 168 bytes of LDS, above the 64 KB a launch gets by
# default; (2, 37, 32): the other head width.  A layer of 3 cuts of 6 rows; (cut, T) picks the cut under test and its data rows r:
# cut 0 (nothing carried in) with r = 1, 2, 6 — a first cut always has a row — and cut 1 (out_0 carried in, a gradient carried back) with
# r = 0, 2, 6.
CUT_SHAPES = [(1, 16, 16), (3, 37, 16), (2, 170, 16), (1, 266, 16), (2, 37, 32)]
CUT_CASES = [(0, 1), (0, 2), (0, 9), (1, 6), (1, 8), (1, 12)]
CUTS, CS = 3, 6


def test_lds_plan():
    """the widest launch is the key / value backward, 16 N C + 192 N bytes: T and dS of both proxies and three statistics per (row, head)"""
    assert H.plan(170, 16) == 448 * 170 == 76160 > 64 * 1024 and H.plan(266, 16) == 448 * 266 == 119168
    assert H.plan(16, 16) == (6 * 128 * 16 + 9 * 32 * 16 + 2 * 384) * 4 == 70656          # a small graph: the local backward's tile arrays
    assert H.plan(365, 16) == 163520 <= H.LDS_MAX < H.plan(366, 16)                        # the first N refused at C = 16
    assert H.plan(232, 32) == 163840 == H.LDS_MAX < H.plan(233, 32) and H.plan(170, 24) < 0
    assert ops.stwa_slab_shape(3, 37, 16) == (9, 30 * 256 + 30 * 16)


def _cut_inputs(B, N, C, cut, T, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)          # noqa: E731
    d = SimpleNamespace(B=B, N=N, C=C, cut=cut, T=T, r=max(0, min(CS, T - cut * CS)), rn=rn)
    d.h, d.prox, d.Y = rn(B, T, N, C), rn(2 * CUTS, N, C), 0.7 * rn(B, CUTS, N, C)
    d.co, d.cb = rn(B, N, 4, 5).abs(), rn(B, N, 4, 5).abs()                        # what a ReLU leaves
    d.V, d.u = 0.5 * rn(4, 6, C, C) / C ** 0.5, 0.5 * rn(4, 6, C)
    d.Wl, d.bl = 1.5 * rn(6, C, C) / C ** 0.5, 0.3 * rn(6, C)
    d.V[0] *= 2.0                                                                  # sharper temporal scores: two keys alone (r = 0) are not a near tie
    for k in ("h", "prox", "co", "cb", "V", "u", "Wl", "bl"):
        getattr(d, k).requires_grad_(True)
    d.outprev = (d.Y[:, cut - 1].clone() if cut > 0 else torch.zeros(B, N, C, dtype=torch.float64)).requires_grad_(True)
    d.gpu = {k: _g(getattr(d, k)) for k in ("h", "prox", "Y", "co", "cb", "V", "u", "Wl", "bl")}
    d.gpu["WlT"] = d.gpu["Wl"].transpose(1, 2).contiguous()
    return d


def _local_ref(d):
    return su.cut_local(d.h[:, d.cut * CS:(d.cut + 1) * CS], d.prox[2 * d.cut:2 * d.cut + 2], d.outprev, d.co, d.cb, d.V, d.u, d.Wl, d.bl)


def _slab_parts(slab, C):
    s = slab.sum(0)
    nV, nu, nW = 24 * C * C, 24 * C, 6 * C * C
    return s[:nV].view(4, 6, C, C), s[nV:nV + nu].view(4, 6, C), s[nV + nu:nV + nu + nW].view(6, C, C), s[nV + nu + nW:].view(6, C)


@pytest.mark.parametrize("cut,T", CUT_CASES)
@pytest.mark.parametrize("B,N,C", CUT_SHAPES)
def test_local_launches_against_their_formula(B, N, C, cut, T, parity):
    d = _cut_inputs(B, N, C, cut, T, 100 * N + 10 * cut + T)
    q = d.gpu
    Tr, Kr, Vr, a = _local_ref(d)
    R2 = d.r + 2
    assert float(a.max(dim=2).values.mean()) * R2 >= 1.5                           # the temporal softmax is far from uniform
    out = [[_sent(B, 2, N, C) for _ in range(3)] for _ in range(2)]
    for o in out:
        ops.stwa_local_fwd(q["h"], q["prox"], q["Y"], q["co"], q["cb"], q["V"], q["u"], q["WlT"], q["bl"], *o, cut, CS)
    assert all(torch.equal(x, y) for x, y in zip(*out))
    errs = {"T": _err(out[0][0], Tr), "Ks": _err(out[0][1], Kr), "Vs": _err(out[0][2], Vr)}
    # backward: the gradient of <T, dT> + <Ks, dKs> + <Vs, dVs>
    dT, dK, dV = d.rn(B, 2, N, C), d.rn(B, 2, N, C), d.rn(B, 2, N, C)
    ((Tr * dT).sum() + (Kr * dK).sum() + (Vr * dV).sum()).backward()
    res = []
    for _ in range(2):
        dh, dPb, carry = _sent(B, T, N, C), _sent(B, 2 * CUTS, N, C), _sent(B, N, C)
        dco, dcb = torch.zeros(B, N, 4, 5, device=DEV), torch.zeros(B, N, 4, 5, device=DEV)
        slab = torch.zeros(ops.stwa_slab_shape(B, N, C), device=DEV)
        ops.stwa_local_bwd(q["h"], q["prox"], q["Y"], q["co"], q["cb"], q["V"], q["u"], q["Wl"], q["WlT"], q["bl"], _g(dT), _g(dK), _g(dV), dh, dPb,
                           carry if cut > 0 else None, dco, dcb, slab, cut, CS)
        res.append((dh, dPb, carry, dco, dcb, slab))
    assert all(torch.equal(x, y) for x, y in zip(*res))
    dh, dPb, carry, dco, dcb, slab = res[0]
    lo, hi = cut * CS, cut * CS + d.r
    assert bool((dh[:, :lo] == SENT).all()) and bool((dh[:, hi:] == SENT).all())             # only the cut's rows are written
    own = torch.zeros(2 * CUTS, dtype=torch.bool)
    own[2 * cut:2 * cut + 2] = True
    assert bool((dPb[:, ~own] == SENT).all()) and bool((carry == SENT).all()) == (cut == 0)
    if d.r:
        errs["dh"] = _err(dh[:, lo:hi], d.h.grad[:, lo:hi])
    errs["dprox"] = _err(dPb[:, own].sum(0), d.prox.grad[2 * cut:2 * cut + 2])
    if cut > 0:
        errs["carry"] = _err(carry, d.outprev.grad)
        assert _err(dPb[:, 2 * cut] + dPb[:, 2 * cut + 1], carry) < 1e-6
    errs["dco"] = _err(dco, d.co.grad)
    assert bool((dcb[:, :, 0] == 0).all()) and float(d.cb.grad[:, :, 0].abs().max()) < 1e-12 * float(d.cb.grad.abs().max())
    errs["dcb"] = _err(dcb[:, :, 1:], d.cb.grad[:, :, 1:])
    gV, gu, gW, gb = _slab_parts(slab, C)
    errs["dV"] = _err(gV, d.V.grad)
    assert bool((gu[0] == 0).all()) and float(d.u.grad[0].abs().max()) < 1e-12 * float(d.u.grad.abs().max())
    errs["du"] = _err(gu[1:], d.u.grad[1:])
    errs["dWl"], errs["dbl"] = _err(gW[:2], d.Wl.grad[:2]), _err(gb[:2], d.bl.grad[:2])
    assert bool((gW[2:] == 0).all()) and bool((gb[2:] == 0).all())                             # the other four Linears belong to the spatial backward
    # the accumulating outputs: a second launch onto the first's result doubles it exactly, and without a slab the rest is bit-equal
    ops.stwa_local_bwd(q["h"], q["prox"], q["Y"], q["co"], q["cb"], q["V"], q["u"], q["Wl"], q["WlT"], q["bl"], _g(dT), _g(dK), _g(dV), None, None,
                       None, dco, dcb, slab, cut, CS)
    assert torch.equal(dco, 2 * res[1][3]) and torch.equal(dcb, 2 * res[1][4]) and torch.equal(slab, 2 * res[1][5])
    dh2, dco2 = _sent(B, T, N, C), torch.zeros_like(dco)
    ops.stwa_local_bwd(q["h"], q["prox"], q["Y"], q["co"], q["cb"], q["V"], q["u"], q["Wl"], q["WlT"], q["bl"], _g(dT), _g(dK), _g(dV), dh2, None,
                       None, dco2, torch.zeros_like(dcb), None, cut, CS)
    assert torch.equal(dh2, res[1][0]) and torch.equal(dco2, res[1][3])
    _check(parity, errs)


@pytest.mark.parametrize("cut", [0, 1])
@pytest.mark.parametrize("B,N,C", CUT_SHAPES)
def test_spatial_launches_against_their_formula(B, N, C, cut, parity):
    d = _cut_inputs(B, N, C, cut, 12, 100 * N + cut + 1)
    q = d.gpu
    with torch.no_grad():
        T0, K0, V0, _ = _local_ref(d)
    Tl, Kl, Vl = (t.clone().requires_grad_(True) for t in (T0, K0, V0))
    out, S, mx, sm, a = su.cut_spatial(Tl, Kl, Vl, d.Wl, d.bl)
    S.retain_grad()
    assert float(a.max(dim=-1).values.mean()) * N >= 3.0                            # the spatial softmax is far from uniform
    res = []
    for _ in range(2):
        Y, Sg, mg, sg = _sent(B, CUTS, N, C), _sent(B, 2, N, C), _sent(B, 2, N, 8), _sent(B, 2, N, 8)
        ops.stwa_spatial_fwd(_g(T0), _g(K0), _g(V0), q["WlT"], q["bl"], Y, cut, S=Sg, mx=mg, sm=sg)
        res.append((Y, Sg, mg, sg))
    assert all(torch.equal(x, y) for x, y in zip(*res))
    Y, Sg, mg, sg = res[0]
    other = [i for i in range(CUTS) if i != cut]
    assert bool((Y[:, other] == SENT).all())
    errs = {"out": _err(Y[:, cut], out), "S": _err(Sg, S), "mx": _err(mg, mx), "sm": _err(sg, sm)}
    Y2 = _sent(B, CUTS, N, C)
    ops.stwa_spatial_fwd(_g(T0), _g(K0), _g(V0), q["WlT"], q["bl"], Y2, cut)          # nothing kept: the same output
    assert torch.equal(Y2, Y)
    # backward: the gradient of <out, dY[:, cut] + carry>
    dY, carry = d.rn(B, CUTS, N, C), d.rn(B, N, C)
    (out * (dY[:, cut] + (carry if cut == 0 else 0))).sum().backward()                # (cut 0 of 3 receives a carried gradient, the last one none)
    dYg = _sent(B, CUTS, N, C)
    dYg[:, cut] = _g(dY[:, cut])
    stats = (_g(S), _g(mx), _g(sm))
    res = []
    for _ in range(2):
        dS, Dq, dTq = _sent(B, 2, N, C), _sent(B, 2, N, 8), _sent(B, 2, N, C)
        slab = torch.zeros(ops.stwa_slab_shape(B, N, C), device=DEV)
        ops.stwa_spatial_bwd_q(_g(T0), _g(K0), _g(V0), *stats, q["Wl"], q["WlT"], q["bl"], dYg, _g(carry) if cut == 0 else None, dS, Dq, dTq, slab, cut)
        dKs, dVs = _sent(B, 2, N, C), _sent(B, 2, N, C)
        ops.stwa_spatial_bwd_kv(_g(T0), _g(K0), _g(V0), _g(S.grad), _g((S.grad * S).view(B, 2, N, 8, C // 8).sum(-1)), stats[1], stats[2], dKs, dVs)
        res.append((dS, Dq, dTq, slab, dKs, dVs))
    assert all(torch.equal(x, y) for x, y in zip(*res))
    dS, Dq, dTq, slab, dKs, dVs = res[0]
    errs.update({"dS": _err(dS, S.grad), "Dq": _err(Dq, (S.grad * S).view(B, 2, N, 8, C // 8).sum(-1)), "dT": _err(dTq, Tl.grad),
                 "dKs": _err(dKs, Kl.grad), "dVs": _err(dVs, Vl.grad)})
    gV, gu, gW, gb = _slab_parts(slab, C)
    errs["dWl"], errs["dbl"] = _err(gW[2:], d.Wl.grad[2:]), _err(gb[2:], d.bl.grad[2:])
    assert bool((gV == 0).all()) and bool((gu == 0).all()) and bool((gW[:2] == 0).all()) and bool((gb[:2] == 0).all())
    dS2, Dq2, dTq2 = _sent(B, 2, N, C), _sent(B, 2, N, 8), _sent(B, 2, N, C)
    ops.stwa_spatial_bwd_q(_g(T0), _g(K0), _g(V0), *stats, q["Wl"], q["WlT"], q["bl"], dYg, _g(carry) if cut == 0 else None, dS2, Dq2, dTq2, None, cut)
    assert torch.equal(dS2, dS) and torch.equal(Dq2, Dq) and torch.equal(dTq2, dTq)   # without a slab: the same input gradients
    _check(parity, errs)


# ---- 2. whole models against the fp64 torch module -----------------------------------------------------------------------------------------
def _errs(got, ref):
    (y, dx, g), (y64, dx64, g64) = got, ref
    errs = {"y": _err(y, y64), "dx": _err(dx, dx64)}
    gmax = max(float(torch.as_tensor(v).abs().max()) for v in g64.values())
    assert set(g) == set(g64) and len(g) in (213, 215)
    for k, v in g64.items():
        v = torch.as_tensor(v)
        if su.degenerate(k):
            assert float(g[k].abs().max()) <= su.ZERO * gmax and float(v.abs().max()) <= su.ZERO * gmax, k
        else:
            assert float(v.abs().max()) > 0, k
            errs[k] = _err(g[k], v)
    assert len(errs) == len(g) - 21 + 2
    return errs


def _model_case(B, lag, N, C, out, seed=su.SEED):
    """the inputs of test_predictor_stwa.py::_gpu_input, whose conditions that test asserts on the CPU"""
    torch.manual_seed(seed)
    m = su.perturb_(STWA(su.model_args(N, lag=lag, C=C, out=out), "cpu", 64, backend="hip")).train()
    g = torch.Generator().manual_seed(seed + 1)
    x, w = torch.randn(B, lag, N, 64, generator=g), torch.randn(B, 12, N, out, generator=g)
    return m, x, w, su.noise(B, N, 16, seed + 2)


def _against_fp64(m, x, w, nz, parity):
    ref = su.run(m.double(), x.double(), w.double(), su.cast(nz, torch.float64))
    assert m.backend_used == "torch"
    m = m.float().to(DEV)
    got = su.run(m, x.to(DEV), w.to(DEV), su.cast(nz, torch.float32, DEV))
    assert m.backend_used == "hip"
    _check(parity, _errs(got, ref))


@pytest.mark.parametrize("B,lag,N,C,out", [(2, 12, 20, 16, 1), (3, 8, 37, 16, 2), (1, 12, 170, 16, 1), (2, 5, 16, 32, 1)])
def test_whole_model_against_fp64_torch(B, lag, N, C, out, parity):
    _against_fp64(*_model_case(B, lag, N, C, out), parity)


@pytest.mark.parametrize("ds", ["PEMS08", "METR_LA", "NYC_BIKE", "NYC_TAXI"])
def test_shipped_configurations(ds, parity):
    pa = predictor_args(ds, "STWA")
    assert H.plan(pa.num_nodes, pa.channels) <= H.LDS_MAX
    _against_fp64(*_model_case(1, pa.lag, pa.num_nodes, pa.channels, pa.out_dim), parity)


@pytest.mark.parametrize("c,N,B,lag,out", [("A", 20, 2, 12, 1), ("B", 13, 3, 8, 2)])
def test_whole_model_against_the_reference_vectors(c, N, B, lag, out, parity):
    G = load("stwa_small.npz")
    m = STWA(su.model_args(N, lag=lag, out=out), "cpu", 64, backend="hip")
    keys = [str(k) for k in G[c + ".init.keys"]]
    m.load_state_dict({k: torch.tensor(G["%s.sd.%s" % (c, k)] if "%s.sd.%s" % (c, k) in G else G["%s.init.%s" % (c, k)]) for k in keys}, strict=True)
    m = m.to(DEV).train()
    nz = (_g(torch.tensor(G[c + ".eps_d"])), [_g(torch.tensor(G[c + ".eps_l%d" % i])) for i in range(3)])
    got = su.run(m, _g(torch.tensor(G[c + ".x"])), _g(torch.tensor(G[c + ".w"])), nz)
    assert m.backend_used == "hip"
    ref = (torch.tensor(G[c + ".y"]), torch.tensor(G[c + ".dx"]), {k: torch.tensor(G["%s.grad.%s" % (c, k)]) for k in keys})
    _check(parity, _errs(got, ref))


# ---- 3. the launch sequence, repeatability, the modes ----------------------------------------------------------------------------------------
FWD_OPS, BWD_OPS = ["stwa_local_fwd", "stwa_spatial_fwd"], ["stwa_spatial_bwd_q", "stwa_spatial_bwd_kv", "stwa_local_bwd"]


def _spy(monkeypatch):
    seen = {"calls": [], "kept": [], "slabs": []}

    def wrap(name):
        fn = getattr(ops, name)

        def f(*a, **kw):
            seen["calls"].append(name)
            if name == "stwa_spatial_fwd":
                seen["kept"].append((kw.get("S"), kw.get("mx"), kw.get("sm")))
            if name == "stwa_spatial_bwd_q":
                seen["slabs"].append(a[14])
            if name == "stwa_local_bwd":
                seen["slabs"].append(a[18])
            return fn(*a, **kw)
        monkeypatch.setattr(ops, name, f)
    for n in FWD_OPS + BWD_OPS:
        wrap(n)
    return seen


def _sequence():
    """the documented launch order of one training step: the layers bottom up, two launches a cut; backward top down, cuts in reverse, three"""
    return FWD_OPS * 12 + FWD_OPS * 3 + FWD_OPS * 1, BWD_OPS * 1 + BWD_OPS * 3 + BWD_OPS * 12


def test_launch_sequence_repeatability_and_modes(monkeypatch):
    m, x, w, nz = _model_case(2, 12, 37, 16, 2, seed=3)
    m, x, w, nz = m.to(DEV), x.to(DEV), w.to(DEV), su.cast(nz, torch.float32, DEV)
    seen = _spy(monkeypatch)
    y1, dx1, g1 = su.run(m, x, w, nz)
    fwd, bwd = _sequence()
    assert m.backend_used == "hip" and seen["calls"] == fwd + bwd, seen["calls"]
    assert len(fwd) == 32 and len(bwd) == 48
    assert len(seen["kept"]) == 16 and all(S is not None and a is not None and b is not None for S, a, b in seen["kept"])
    assert len(seen["slabs"]) == 32 and all(s is not None for s in seen["slabs"])
    assert all(bool((g1[k] == 0).all()) for k in g1 if su.degenerate(k))
    # a second step on the same batch: bit for bit
    y2, dx2, g2 = su.run(m, x, w, nz)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    # no_grad, and eval mode with gradients enabled: the same launches, the same output, nothing handed over to keep
    for mode in ("no_grad", "eval"):
        seen["calls"].clear(), seen["kept"].clear()
        if mode == "no_grad":
            with torch.no_grad():
                y3 = m(x, noise=nz)
        else:
            m.eval()
            y3 = m(x.clone().requires_grad_(True), noise=nz)
        assert torch.equal(y3, y1) and m.backend_used == "hip" and not y3.requires_grad and y3.grad_fn is None
        assert seen["calls"] == fwd and all(S is None and a is None and b is None for S, a, b in seen["kept"]), (mode, seen["calls"])
    # the noise is drawn in eval mode too, on both backends the same way
    torch.manual_seed(9)
    ya = m(x)
    torch.manual_seed(9)
    yb = m(x)
    assert torch.equal(ya, yb) and not torch.equal(ya, m(x))


def test_frozen_predictor_skips_the_weight_gradients(monkeypatch):
    """parameters that take no gradient: the input's gradient is the same, bit for bit, and no launch is given a slab to put weight
    gradients in"""
    m, x, w, nz = _model_case(2, 8, 20, 16, 1, seed=5)
    m, x, w, nz = m.to(DEV), x.to(DEV), w.to(DEV), su.cast(nz, torch.float32, DEV)
    want = su.run(m, x, w, nz)[1]
    for p in m.parameters():
        p.requires_grad_(False)
    seen = _spy(monkeypatch)
    xi = x.clone().requires_grad_(True)
    (m(xi, noise=nz) * w).sum().backward()
    assert m.backend_used == "hip" and seen["calls"] == sum(_sequence(), []) and torch.equal(xi.grad, want)
    assert len(seen["slabs"]) == 32 and all(s is None for s in seen["slabs"])


@pytest.mark.parametrize("N,lag,C", [(20, 3, 24), (366, 1, 16)])
def test_unsupported_input_takes_the_torch_path_and_the_module_serves_hip_again(N, lag, C, parity):
    """C = 24 is no kernel width; N = 366 is the first graph whose sample does not fit the LDS plan at C = 16"""
    torch.manual_seed(4)
    ap = su.model_args(N, lag=lag, C=C)
    mh = su.perturb_(STWA(ap, "cpu", 16, backend="hip")).to(DEV).train()
    mt = STWA(ap, "cpu", 16).to(DEV).train()
    mt.load_state_dict(mh.state_dict(), strict=True)
    x, w, nz = torch.randn(1, lag, N, 16, device=DEV), torch.randn(1, 12, N, 1, device=DEV), su.cast(su.noise(1, N, 16), torch.float32, DEV)
    assert not H.supported(mh, x)
    (yh, dxh, gh), (yt, dxt, gt) = su.run(mh, x, w, nz), su.run(mt, x, w, nz)
    assert mh.backend_used == "torch" and mt.backend_used == "torch"
    assert torch.equal(yh, yt) and torch.equal(dxh, dxt) and all(torch.equal(gh[k], gt[k]) for k in gh)
    if C == 16:                                                            # N = 365, the largest graph the plan admits, is served
        m2, x2, w2, nz2 = _model_case(1, lag, 365, 16, 1)
        m2, x2, nz2 = m2.to(DEV), x2.to(DEV), su.cast(nz2, torch.float32, DEV)
        with torch.no_grad():
            y2 = m2(x2, noise=nz2)
            assert m2.backend_used == "hip"
            m2.backend = "torch"
            yt2 = m2(x2, noise=nz2)
        assert m2.backend_used == "torch"
        _check(parity, {"y": _err(y2, yt2)})


def test_one_module_alternates_between_the_paths():
    """a module built for N = 20 serves a CUDA fp32 batch on HIP, an fp64 copy of it on torch, and the fp32 batch on HIP again"""
    m, x, w, nz = _model_case(2, 8, 20, 16, 1, seed=6)
    m, x = m.to(DEV), x.to(DEV)
    nz = su.cast(nz, torch.float32, DEV)
    with torch.no_grad():
        y1 = m(x, noise=nz)
        assert m.backend_used == "hip"
        m.double()
        y64 = m(x.double(), noise=su.cast(nz, torch.float64, DEV))
        assert m.backend_used == "torch"
        m.float()
        assert torch.equal(m(x, noise=nz), y1) and m.backend_used == "hip" and _err(y1, y64) < 1e-4


# ---- 4. the chain --------------------------------------------------------------------------------------------------------------------------
def _front_end(tmp_path, backend, finetune, sd):
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    N = 20
    args = make_args("PEMS08", mode="eval", num_nodes=N, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros(), batch_size=8, epochs=3,
                     early_stop=False, log_dir=str(tmp_path), debug=True, model="STWA_test", stwa_backend=backend)
    sd = O.init_state_dict(args, 4) if sd is None else sd
    torch.manual_seed(0)
    pred = su.perturb_(STWA(su.model_args(N, out=args.output_dim), "cpu", args.hidden_dim, backend=args.stwa_backend))
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
        torch.manual_seed(31)                                              # the same noise on both backends
        loss = tr._loss(model(src, tgt)[0], tgt)
        loss.backward()
        assert model.predictor.backend_used == name
        res[name] = (float(loss.detach()), {k: p.grad for k, p in model.named_parameters() if p.requires_grad and p.grad is not None})
    assert set(res["hip"][1]) == set(res["torch"][1])
    assert any(k.startswith("pretrain_model.") for k in res["hip"][1]) == finetune
    errs = {"loss": abs(res["hip"][0] - res["torch"][0]) / abs(res["torch"][0])}
    pk = [k for k in res["torch"][1] if k.startswith("predictor.")]
    gmax = max(float(res["torch"][1][k].abs().max()) for k in pk)
    for k, g in res["torch"][1].items():
        if k.startswith("predictor.") and su.degenerate(k[len("predictor."):]):
            assert float(res["hip"][1][k].abs().max()) <= su.ZERO * gmax and float(g.abs().max()) <= su.ZERO * gmax, k
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
    torch.manual_seed(2)
    losses = [tr.train_epoch(e) for e in (1, 2, 3)]
    assert model.predictor.backend_used == "hip"
    assert losses[2] < losses[0] and all(np.isfinite(losses)), losses
    rows = tr.test(test)
    assert model.predictor.backend_used == "hip"
    assert rows.shape == (13, 4) and bool(torch.isfinite(rows[:, :3]).all())
