"""The ST-MGCN LSTM launches without a GPU.

1. The explicit per-step formulas of stmgcn_util (what tests/test_gpu_stmgcn_hip.py holds the two launches of csrc/stmgcn.hip to) equal
   ``nn.LSTM`` under autograd in float64 at 1e-12: the top ring, dx and every weight and bias gradient formed from dG and the h ring the way
   predictors/stmgcn_hip.py forms them.
2. ``pack`` / ``unpack`` / ``transposed`` round-trip.
3. The inputs of the GPU launch tests can tell a wrong kernel from a right one: exchanging any two of the i / f / g / o blocks in the fp64
   formula moves the top ring by more than 100 x the GPU bound, for every input those tests use.
4. predictors/stmgcn_hip.py with every ``ops`` entry it calls replaced by its formula in torch is held to autograd on the torch path of
   the same module in fp64 at 1e-9: y, dx and all 38 gradients, and with the LSTMs frozen."""
import itertools

import pytest
import torch

import stmgcn_util as gu
from gptst_amd import ops
from gptst_amd.predictors import STMGCN, stmgcn_hip as SH

GPU_TOL = 1e-4             # downstream_util.TOL


def _rel(got, ref):
    got, ref = got.detach(), ref.detach()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("L,T,H", [(l, t, h) for l in (1, 3) for t in (1, 2, 12) for h in (16, 48)])
def test_step_formulas_equal_nn_lstm_autograd(L, T, H):
    torch.manual_seed(L * 100 + T * 10 + H)
    rows, C = 7, 16
    lstm = torch.nn.LSTM(C, H, num_layers=L, batch_first=True).double()
    with torch.no_grad():
        for p in lstm.parameters():
            if p.dim() == 2:
                p.mul_(3.0)
    x = torch.randn(rows, T, C, dtype=torch.float64, requires_grad=True)
    out, _ = lstm(x)
    w = torch.randn(rows, T, H, dtype=torch.float64)
    (out * w).sum().backward()
    with torch.no_grad():
        W, b, Wih0 = gu.lstm_operands(lstm)
        Gx0 = (x @ Wih0.t() + b[0]).transpose(0, 1).contiguous()
        top, gates, cs, hs = gu.lstm_fwd(Gx0, W, b)
        assert _rel(top.transpose(0, 1), out) < 1e-12
        dG = gu.lstm_bwd(w.transpose(0, 1).contiguous(), W, gates, cs)
        assert _rel((dG[0] @ Wih0).transpose(0, 1), x.grad) < 1e-12
        flat = lambda v: v.reshape(T * rows, -1)                           # noqa: E731
        assert _rel(flat(dG[0]).t() @ flat(x.transpose(0, 1)), lstm.weight_ih_l0.grad) < 1e-12
        for l in range(L):
            g = lambda n: getattr(lstm, "%s_l%d" % (n, l)).grad            # noqa: E731
            if T > 1:                                                      # (T = 1: h_{-1} = 0, the gradient is exactly 0 on both sides)
                assert _rel(flat(dG[l]).t() @ flat(hs[l, :T]), g("weight_hh")) < 1e-12
            else:
                assert not bool(g("weight_hh").any()) and not bool((flat(dG[l]).t() @ flat(hs[l, :T])).any())
            if l:
                assert _rel(flat(dG[l]).t() @ flat(hs[l - 1, 1:]), g("weight_ih")) < 1e-12
            assert _rel(flat(dG[l]).sum(0), g("bias_ih")) < 1e-12 and _rel(g("bias_hh"), g("bias_ih")) < 1e-12


@pytest.mark.parametrize("H,L", [(16, 1), (48, 2), (64, 3), (128, 4)])
def test_pack_round_trips(H, L):
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(32, H, num_layers=L)
    W, bias, Wih0 = SH.pack(lstm)
    assert W.numel() == ops.stmgcn_wsize(H, L) and tuple(bias.shape) == (L, 4 * H) and Wih0 is lstm.weight_ih_l0
    for l, (ih, hh) in enumerate(SH.unpack(W, H, L)):
        assert torch.equal(hh, getattr(lstm, "weight_hh_l%d" % l)) and torch.equal(bias[l], getattr(lstm, "bias_ih_l%d" % l) + getattr(lstm, "bias_hh_l%d" % l))
        assert (ih is None) == (l == 0) and (l == 0 or torch.equal(ih, getattr(lstm, "weight_ih_l%d" % l)))
    WT, off = SH.transposed(W, H, L), 0
    for l, (ih, hh) in enumerate(SH.unpack(W, H, L)):
        k = H if l == 0 else 2 * H
        full = hh if l == 0 else torch.cat([ih, hh], 1)
        assert torch.equal(WT[off:off + 4 * H * k].view(k, 4 * H), full.t())
        off += 4 * H * k
    assert off == WT.numel()


@pytest.mark.parametrize("rows,T,L,H", gu.LAUNCH_CASES)
def test_launch_inputs_tell_swapped_gates_apart(rows, T, L, H):
    Gx0, W, b, _ = gu.launch_inputs(rows, T, L, H)
    top = gu.lstm_fwd(Gx0, W, b)[0]
    for i, j in itertools.combinations(range(4), 2):
        order = list(range(4))
        order[i], order[j] = order[j], order[i]
        wrong = gu.lstm_fwd(Gx0, W, b, order=tuple(order))[0]
        assert _rel(wrong, top) > 100 * GPU_TOL, (i, j, _rel(wrong, top))


# ---- predictors/stmgcn_hip.py on torch stand-ins ---------------------------------------------------------------------------------------
def _blocks(flat, H, L, transposed=False):
    out, off = [], 0
    for l in range(L):
        k = H if l == 0 else 2 * H
        blk = flat[off:off + 4 * H * k]
        out.append(blk.view(k, 4 * H).t() if transposed else blk.view(4 * H, k))
        off += 4 * H * k
    return out


def _fwd(Gx0, W, bias, L, keep, tiles=0):
    H = Gx0.shape[2] // 4
    top, gates, cs, hs = gu.lstm_fwd(Gx0, _blocks(W, H, L), list(bias))
    return (top, gates, cs, hs) if keep else (top.clone(), None, None, None)


def _bwd(dTop, WT, gates, c, dG_layers, tiles=0):
    L, H = gates.shape[0], gates.shape[3] // 4
    return gu.lstm_bwd(dTop, _blocks(WT, H, L, transposed=True), gates, c)[:dG_layers].contiguous()


def _tapgemm(X, W, bias, taps, act, T, N, res=None, res_w=0, keep=False):
    assert tuple(taps) == (0,) and act == 0 and res is None
    y = X @ W.t()
    return y + bias if bias is not None else y


def _wgrad(D, X, taps, T, N, want_bias=True):
    return D.t() @ X, (D.sum(0) if want_bias else None)


@pytest.fixture
def stand_ins(monkeypatch):
    calls = []
    rec = lambda name, fn: lambda *a, **k: (calls.append(name), fn(*a, **k))[1]      # noqa: E731
    monkeypatch.setattr(ops, "stmgcn_lstm_fwd", rec("fwd", _fwd))
    monkeypatch.setattr(ops, "stmgcn_lstm_bwd", rec("bwd", _bwd))
    monkeypatch.setattr(ops, "stgcn_tapgemm", rec("tapgemm", _tapgemm))
    monkeypatch.setattr(ops, "stgcn_wgrad", rec("wgrad", _wgrad))
    monkeypatch.setattr(SH, "supported", lambda model, x: True)
    monkeypatch.setattr(SH._C, "lib", lambda: None)
    return calls


def _pair(N, T, C, H, L, out):
    torch.manual_seed(3)
    dis, pcc = gu.graphs(N)
    from gptst_amd import graph
    ap = gu.model_args(N, graph.stmgcn_supports(dis), graph.stmgcn_supports(pcc), T=T, H=H, L=L, G=24)
    a = gu.perturb_(STMGCN(ap, "cpu", C, out, backend="hip")).double().train()
    b = STMGCN(ap, "cpu", C, out, backend="torch").double().train()
    b.load_state_dict(a.state_dict(), strict=True)
    return a, b


@pytest.mark.parametrize("N,T,C,H,L,out", [(9, 4, 16, 16, 3, 2), (6, 1, 32, 32, 1, 1), (5, 3, 16, 48, 2, 2)])
def test_hip_module_on_stand_ins_equals_autograd(stand_ins, N, T, C, H, L, out):
    a, b = _pair(N, T, C, H, L, out)
    x = torch.randn(2, T, N, C, dtype=torch.float64)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    w = torch.randn(2, T, N, out, dtype=torch.float64)
    ya, yb = a(xa), b(xb)
    assert (a.backend_used, b.backend_used) == ("hip", "torch") and _rel(ya, yb) < 1e-9
    (ya * w).sum().backward()
    (yb * w).sum().backward()
    assert stand_ins.count("fwd") == 2 and stand_ins.count("bwd") == 2 and stand_ins.count("wgrad") == 2 * (2 * L - 1) + 1
    assert _rel(xa.grad, xb.grad) < 1e-9
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    assert len(ga) == 8 + 8 * L + 6
    for k in ga:
        if T == 1 and "weight_hh" in k:
            assert not bool(ga[k].grad.any()) and not bool(gb[k].grad.any()), k
        else:
            assert _rel(ga[k].grad, gb[k].grad) < 1e-9, k
        if "bias_ih" in k:
            assert torch.equal(ga[k].grad, ga[k.replace("bias_ih", "bias_hh")].grad), k


def test_frozen_lstm_forms_no_weight_gradient_and_dx_is_bit_equal(stand_ins):
    a, _ = _pair(9, 4, 16, 16, 3, 2)
    x = torch.randn(2, 4, 9, 16, dtype=torch.float64)
    x1 = x.clone().requires_grad_(True)
    a(x1).square().sum().backward()
    n_full = stand_ins.count("wgrad")
    del stand_ins[:]
    for r in a.rnn_list:
        for p in r.lstm.parameters():
            p.requires_grad_(False)
            p.grad = None
    x2 = x.clone().requires_grad_(True)
    a(x2).square().sum().backward()
    assert n_full == 11 and stand_ins.count("wgrad") == 0 and stand_ins.count("bwd") == 2
    assert torch.equal(x1.grad, x2.grad) and a.rnn_list[0].lstm.weight_hh_l1.grad is None and a.rnn_list[0].fc.weight.grad is not None


def test_no_grad_and_eval_keep_nothing(stand_ins):
    a, b = _pair(9, 4, 16, 16, 3, 2)
    x = torch.randn(2, 4, 9, 16, dtype=torch.float64)
    with torch.no_grad():
        y = a(x)
    assert y.grad_fn is None and _rel(y, b(x)) < 1e-9
    y = a.eval()(x.clone().requires_grad_(True))
    assert y.grad_fn is None and stand_ins.count("bwd") == 0
