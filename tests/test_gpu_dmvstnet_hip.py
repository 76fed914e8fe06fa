"""The DMVSTNET predictor on HIP (``DMVSTNET(..., backend="hip")``, csrc/dmvstnet.hip, predictors/dmvstnet_hip.py) on the GPU.  The reference
of every comparison is the explicit formula of dmvstnet_util (held to autograd of the torch module at 1e-12 by tests/test_dmvstnet_hip_cpu.py)
or the torch DMVSTNET module (pinned to the reference implementation's vectors by tests/test_predictor_dmvstnet.py), in fp64 on the CPU; the
bound is the project's element-wise one, 1e-4 of the reference tensor's largest magnitude (downstream_util.TOL), for every output, dX and
parameter gradient.  Exchanging two gates or dropping the h_{T-1} term moves the output by more than 1e-2 on these inputs
(test_dmvstnet_hip_cpu.py asserts it): the bound sits between the two.

Semantic launches (units, N, C): (1, 5, 64) below one node tile; (3, 17, 16) a tile plus one node; (130, 17, 128): 130 units are 44 splits of
3 units, so the loop over a split's units and the sum over the splits both run more than once, and at C = 128 both 64-channel chunks of a
lane are live.  Every raw launch writes into sentinel-filled buffers, runs twice and must repeat bit for bit.  The LSTM runs on ST-MGCN's
launches (tests/test_gpu_stmgcn_hip.py holds them, at one layer and at H = 128 too); the head applied inside those launches was measured
slower and is not built, so it has no launch tests here."""
import pytest
import torch

import dmvstnet_util as gu
from gptst_amd import _C, ops
from gptst_amd.config import predictor_args
from gptst_amd.predictors import DMVSTNET, dmvstnet_hip as DH
from golden_util import load
from downstream_util import _check, _err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0


def _g(t):
    return t.float().to(DEV).contiguous()


def _sent(*shape):
    return torch.full(shape, SENT, device=DEV, dtype=torch.float32)


def _twice(make, call):
    """`make()` -> sentinel-filled outputs, `call(outs)` launches into them; two runs must agree bit for bit -> the first run's outputs"""
    runs = []
    for _ in range(2):
        outs = make()
        call(outs)
        runs.append(outs)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert (a is None and b is None) or torch.equal(a, b)
    return runs[0]


# ---- 1. the plans ------------------------------------------------------------------------------------------------------------------------------
def test_split_plan_and_tile_choice_are_pinned():
    v = _C.lib().value
    assert v("gptst_dmvst_sen_nsplit", 768, 266) == 60 and v("gptst_dmvst_sen_nsplit", 130, 17) == 44 and v("gptst_dmvst_sen_nsplit", 3, 17) == 3
    assert DH.row_tiles(128) == 1 and DH.row_tiles(80) == 1 and DH.row_tiles(64) == 0 and DH.row_tiles(16) == 0     # one tile above H = 64
    assert ops.stmgcn_lds_bytes(128, 1, 1) == 16 * (7 * 128 + 4) * 4 == 57600 <= DH.LDS_MAX


# ---- 2. the semantic launches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("units,N,C", gu.SEN_CASES)
def test_sen_launches(units, N, C, parity):
    O = gu.SEN_O
    x, V, c, dz = gu.sen_inputs(units, N, C)
    gx, gv, gc, gd = _g(x), _g(V), _g(c), _g(dz)
    rows = units * N
    z = _twice(lambda: (_sent(rows, O),), lambda o: _C.lib().call("gptst_dmvst_sen_fwd", _C.ptr(gx), _C.ptr(gv), _C.ptr(gc), _C.ptr(o[0]), units,
                                                                  N, C, O, _C.stream()))[0]
    ns = _C.lib().value("gptst_dmvst_sen_nsplit", units, N)
    dx, pV, pc = _twice(lambda: (_sent(rows, C), _sent(ns, N, C, O), _sent(ns, N, O)),
                        lambda o: _C.lib().call("gptst_dmvst_sen_bwd", _C.ptr(gx), _C.ptr(gv), _C.ptr(gd), *[_C.ptr(t) for t in o], ns, units, N,
                                                C, O, _C.stream()))
    wdx, wdV, wdc = gu.sen_bwd(x, V, dz, N)
    _check(parity, {"z": _err(z, gu.sen_fwd(x, V, c, N)), "dx": _err(dx, wdx), "dV": _err(pV.sum(0), wdV), "dc": _err(pc.sum(0), wdc)})
    got = ops.dmvst_sen_bwd(gx, gv, gd, N)                                 # the wrapper: the same launch, the splits summed
    assert torch.equal(got[0], dx) and torch.equal(got[1], pV.sum(0)) and torch.equal(got[2], pc.sum(0)) and torch.equal(ops.dmvst_sen_fwd(gx, gv, gc, N), z)


def test_launches_refuse_what_they_do_not_serve():
    x = _sent(4)
    p, s = _C.ptr(x), _C.stream()
    v = _C.lib().value
    assert v("gptst_dmvst_sen_fwd", p, p, p, p, 1, 5, 24, 2, s) == _C.ESHAPE and v("gptst_dmvst_sen_fwd", p, p, p, p, 1, 5, 16, 5, s) == _C.ESHAPE
    assert v("gptst_dmvst_sen_fwd", p, p, p, p, 1, 5, 144, 2, s) == _C.ESHAPE and v("gptst_dmvst_sen_fwd", p, p, p, p, 0, 5, 16, 2, s) == -1
    assert v("gptst_dmvst_sen_bwd", p, p, p, p, p, p, 1, 1, 5, 24, 2, s) == _C.ESHAPE and v("gptst_dmvst_sen_bwd", p, p, p, p, p, p, 1, 1, 5, 16, 0, s) == _C.ESHAPE
    assert v("gptst_dmvst_sen_bwd", p, p, p, p, p, p, 2, 1, 5, 16, 2, s) == -1                                   # a split count that is not the plan's
    assert v("gptst_dmvst_sen_bwd", p, p, p, None, p, p, 1, 1, 5, 16, 2, s) == -1                                # no dx
    torch.cuda.synchronize()
    assert bool((x == SENT).all())


# ---- 3. whole models --------------------------------------------------------------------------------------------------------------------------
def _run(m, x, w):
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    y = m(xi)
    (y * w).sum().backward()
    return y.detach(), xi.grad, {k: p.grad for k, p in m.named_parameters()}


def _errs(got, ref):
    errs = {"y": _err(got[0], ref[0]), "dx": _err(got[1], ref[1])}
    assert set(got[2]) == set(ref[2])
    for k, g in ref[2].items():
        if k in gu.NO_GRAD_KEYS:
            assert g is None and got[2][k] is None, k
            continue
        assert float(g.abs().max()) > 0, k                                 # the comparison is not made where everything is zero
        errs[k] = _err(got[2][k], g)
    return errs


@pytest.mark.parametrize("B,T,N,C,hid", [(2, 3, 20, 64, 64), (1, 12, 17, 16, 8), (3, 2, 33, 128, 32)])
def test_whole_model_against_fp64_torch(B, T, N, C, hid, parity):
    ap = gu.model_args(N, gu.adjacency(N), T=T, hidden=hid)
    torch.manual_seed(3)
    mh = gu.perturb_(DMVSTNET(ap, "cpu", C, 2, backend="hip")).to(DEV).train()
    mt = DMVSTNET(ap, "cpu", C, 2).double().train()
    mt.load_state_dict({k: v.detach().cpu().double() for k, v in mh.state_dict().items()}, strict=True)
    x, w = torch.randn(B, T, N, C), torch.randn(B, T, N, 2)
    got = _run(mh, x.to(DEV), w.to(DEV))
    # hidden_dim 8 is no width of the row kernels (`supported` asks for multiples of 16): that model is held to the same bound on the path it takes
    assert mh.backend_used == ("hip" if hid % 16 == 0 else "torch")
    errs = _errs(got, _run(mt, x.double(), w.double()))
    assert len(errs) == 20
    _check(parity, errs)


def test_whole_model_against_the_reference_vectors(parity):
    G = load("dmvstnet_small.npz")
    m = DMVSTNET(gu.model_args(20, G["A"], T=12, hidden=32), "cpu", 64, 2, backend="hip")
    m.load_state_dict({k[3:]: torch.tensor(G[k]) for k in G.files if k.startswith("sd.")}, strict=True)
    m = m.to(DEV).train()
    got = _run(m, torch.tensor(G["x"]).float().to(DEV), torch.tensor(G["w"]).float().to(DEV))
    assert m.backend_used == "hip"
    grads = {k: (torch.tensor(G["grad." + k]) if ("grad." + k) in G else None) for k in m.state_dict()}
    errs = _errs(got, (torch.tensor(G["y"]), torch.tensor(G["dx"]), grads))
    assert len(errs) == 20
    _check(parity, errs)


@pytest.mark.parametrize("ds", ["NYC_TAXI", "NYC_BIKE"])
def test_shipped_configuration_against_the_torch_backend(ds, parity):
    """Forward + backward at the conf shape, B = 64, against the torch backend in fp32 on the same GPU.

    Local_GNN1's ReLU sees 13 million pre-activations here, about 0.024 wide around the bias: with the bias drawn around 0 one of them lies
    within fp32 rounding of the kink (measured with the draw of ``perturb_``: one unit at 6.1e-9 in fp64, 0 on the HIP path, positive in
    torch) and that unit's whole gradient, 3.7e-3, then shows in ``Local_GNN1.lin.bias.grad`` as 1.4e-4 of its largest entry — every other
    difference of that tensor sums to 7.2e-7.  That is the comparison's conditioning, not either backend's error, so this test puts every
    channel's bias at least 0.4 from zero, either side (the mix-then-lin term measured up to 0.22 in magnitude), and asserts what it relies on —
    every unit at least 1e-3 from the kink, four orders above the fp32 rounding of a pre-activation of this size; the kink itself, with units
    on both sides inside a channel, is what the smaller whole-model cases above exercise."""
    pa = predictor_args(ds, "DMVSTNET")
    B, C, N, T = 64, 64, pa.num_nodes, pa.input_window
    ap = gu.model_args(N, gu.adjacency(N, seed=5), T=T, hidden=pa.hidden_dim, topo=pa.topo_embedded_dim)
    torch.manual_seed(9)
    mh = gu.perturb_(DMVSTNET(ap, "cpu", C, 2, backend="hip"))
    with torch.no_grad():
        b = mh.Local_GNN1.lin.bias
        b.copy_(torch.where(torch.rand(b.shape) < 0.5, -1.0, 1.0) * (0.4 + 0.1 * torch.randn(b.shape).abs()))
    mh = mh.to(DEV).train()
    mt = DMVSTNET(ap, "cpu", C, 2).to(DEV).train()
    mt.load_state_dict(mh.state_dict(), strict=True)
    x, w = torch.randn(B, T, N, C, device=DEV), torch.randn(B, T, N, 2, device=DEV)
    assert DH.supported(mh, x)
    pre = []
    hook = mt.Local_GNN1.lin.register_forward_hook(lambda m, i, o: pre.append((float(o.detach().abs().min()), bool((o > 0).any()), bool((o < 0).any()))))
    got, ref = _run(mh, x, w), _run(mt, x, w)
    hook.remove()
    assert (mh.backend_used, mt.backend_used) == ("hip", "torch")
    assert pre[0][0] > 1e-3 and pre[0][1] and pre[0][2], pre                # no unit near the kink; units on either side of it
    errs = _errs(got, ref)
    assert len(errs) == 20
    _check(parity, errs)


# ---- 4. the modes, the fallback ---------------------------------------------------------------------------------------------------------------
def test_eval_mode_keeps_nothing_and_equals_train_mode(monkeypatch):
    torch.manual_seed(3)
    m = gu.perturb_(DMVSTNET(gu.model_args(20, gu.adjacency(20), T=4, hidden=32), "cpu", 64, 2, backend="hip")).to(DEV)
    x, w = torch.randn(2, 4, 20, 64, device=DEV), torch.randn(2, 4, 20, 2, device=DEV)
    kept, calls = [], []
    fwd, senb = ops.stmgcn_lstm_fwd, ops.dmvst_sen_bwd

    def spy(*a, **kw):
        out = fwd(*a, **kw)
        kept.append(sum(t.numel() for t in out[1:] if t is not None))
        return out
    monkeypatch.setattr(ops, "stmgcn_lstm_fwd", spy)
    monkeypatch.setattr(ops, "dmvst_sen_bwd", lambda *a, **kw: calls.append("sen_bwd") or senb(*a, **kw))
    m.train()
    y1, dx1, g1 = _run(m, x, w)
    rows, H = 2 * 20, 64
    assert m.backend_used == "hip" and kept == [4 * rows * 5 * H + 5 * rows * H] and calls == ["sen_bwd"]
    y2, dx2, g2 = _run(m, x, w)                                            # a second step on the same batch: bit for bit
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2) and all(g1[k] is None or torch.equal(g1[k], g2[k]) for k in g1)
    for mode in ("no_grad", "eval"):
        kept.clear()
        if mode == "no_grad":
            with torch.no_grad():
                y3 = m(x)
        else:
            m.eval()
            y3 = m(x.clone().requires_grad_(True))
        assert torch.equal(y3, y1) and m.backend_used == "hip" and not y3.requires_grad and kept == [0], mode


@pytest.mark.parametrize("T,hid", [(3, 40), (33, 32)])
def test_what_the_kernels_do_not_serve_takes_the_torch_path(T, hid):
    torch.manual_seed(4)
    ap = gu.model_args(20, gu.adjacency(20), T=T, hidden=hid)
    mh = gu.perturb_(DMVSTNET(ap, "cpu", 64, 2, backend="hip")).to(DEV)
    mt = DMVSTNET(ap, "cpu", 64, 2).to(DEV)
    mt.load_state_dict(mh.state_dict(), strict=True)
    x = torch.randn(2, T, 20, 64, device=DEV)
    assert not DH.supported(mh, x)
    yh, yt = mh(x), mt(x)
    assert mh.backend_used == "torch" and mt.backend_used == "torch" and torch.equal(yh, yt)
