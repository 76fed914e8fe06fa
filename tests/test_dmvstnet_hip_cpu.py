"""The formulas the DMVSTNET HIP backend is held to (dmvstnet_util: the LSTM with the head's columns applied to every step's h, forward and
backward, the semantic view as a per-node thin projection forward and backward), on the CPU in float64 against autograd of the torch
module, at 1e-12 of the reference tensor's largest magnitude: both reassociations are exact algebra, only the summation order moves.  Then
what the GPU tests rest on: the packing of V and c as the HIP backend forms it, the fallback on CPU input, and that the inputs of the GPU
model tests tell a wrong model from a right one by far more than their bound."""
import pytest
import torch

import dmvstnet_util as gu
from gptst_amd.predictors import DMVSTNET, dmvstnet_hip as DH

EXACT = 1e-12
MODELS = [(2, 3, 20, 64, 64), (1, 12, 17, 16, 8), (3, 2, 33, 128, 32)]          # (B, T, N, dim_in, hidden_dim): the GPU tests' whole models


def _err(got, ref):
    return float((got.detach().double() - ref.detach().double()).abs().max()) / max(float(ref.detach().abs().max()), 1e-30)


def _model(B, T, N, C, hid, seed=3, dtype=torch.float64):
    torch.manual_seed(seed)
    m = gu.perturb_(DMVSTNET(gu.model_args(N, gu.adjacency(N), T=T, hidden=hid), "cpu", C, 2)).to(dtype).train()
    return m, torch.randn(B, T, N, C, dtype=dtype), torch.randn(B, T, N, 2, dtype=dtype)


@pytest.mark.parametrize("B,T,N,C,hid", MODELS)
def test_restated_forward_and_the_four_formulas_equal_autograd(B, T, N, C, hid):
    m, x, w = _model(B, T, N, C, hid)
    H = m.lstm_dim
    xi = x.clone().requires_grad_(True)
    want = m(xi)
    out, p = gu.restated(m, xi)
    assert _err(out, want) < EXACT
    # backward: the two formulas against autograd through the restated graph's own tensors
    dout = w.permute(1, 0, 2, 3).reshape(T, B * N, 2)                      # time-major
    dy = dout.clone()
    dy[T - 1] += dout.sum(0)                                               # top[t] = y_t + y_{T-1}
    Wa = m.output.weight[:, :H]
    dG = gu.lstm_head_bwd(dy, m.lstm.weight_hh_l0, Wa, p["gates"], p["c"])
    gr = torch.autograd.grad((out * w).sum(), [p["Gx0"], p["V"], p["cvec"], p["z"]], retain_graph=True)
    assert _err(dG, gr[0]) < EXACT
    dx_s, dV, dc = gu.sen_bwd(p["X"].detach(), p["V"].detach(), gr[3], N)
    assert _err(dV, gr[1]) < EXACT and _err(dc, gr[2]) < EXACT
    # the whole restated backward equals the module's: dx and every parameter gradient
    names = [k for k, _ in m.named_parameters() if k not in gu.NO_GRAD_KEYS]
    ps = [dict(m.named_parameters())[k] for k in names]
    a = torch.autograd.grad((want * w).sum(), [xi] + ps, retain_graph=True)
    b = torch.autograd.grad((out * w).sum(), [xi] + ps, retain_graph=True)
    for k, ga, gb in zip(["dx"] + names, a, b):
        assert _err(gb, ga) < EXACT, k
    # the semantic view's share of dx, and the head's weight gradient as the HIP backend forms it
    z_only = torch.autograd.grad((p["z"] * gr[3]).sum(), xi, retain_graph=True)[0]
    assert _err(dx_s.view(T, B, N, C).permute(1, 0, 2, 3), z_only) < EXACT
    dWa = dy.reshape(-1, 2).t() @ p["h"][1:].reshape(-1, H)
    assert _err(dWa, dict(zip(names, a[1:]))["output.weight"][:, :H]) < EXACT


def test_packing_of_v_and_c():
    m, x, _ = _model(2, 3, 20, 64, 32)
    V, c = DH.sen_pack(m)                                                  # the head applied to w first
    Vl, cl = gu.sen_pack(m)                                                # the (N, h, h) weight first, as the model forms it
    assert tuple(V.shape) == (20, 64, 2) and tuple(c.shape) == (20, 2) and _err(V, Vl) < EXACT and _err(c, cl) < EXACT
    sen = torch.einsum("btni,nio->btno", m.Lin_in_sen(x), torch.einsum("nd,dio->nio", m.node_embeddings, m.w))
    want = sen @ m.output.weight[:, m.lstm_dim:].t()
    z = gu.sen_fwd(x.permute(1, 0, 2, 3).reshape(-1, 64), V, c, 20).view(3, 2, 20, 2).permute(1, 0, 2, 3)
    assert _err(z, want) < EXACT
    g = torch.autograd.grad(V.sum() + c.sum(), [m.node_embeddings, m.w, m.Lin_in_sen.weight, m.Lin_in_sen.bias, m.output.weight])
    assert all(float(t.abs().max()) > 0 for t in g)                        # autograd reaches the five parameters


def test_cpu_input_takes_the_torch_path_bit_equally():
    a, x, _ = _model(2, 3, 20, 64, 32, dtype=torch.float32)
    b = DMVSTNET(gu.model_args(20, gu.adjacency(20), T=3, hidden=32), "cpu", 64, 2, backend="hip").train()
    b.load_state_dict(a.state_dict(), strict=True)
    assert not DH.supported(b, x)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = a(xa), b(xb)
    assert (b.backend, b.backend_used, a.backend_used) == ("hip", "torch", "torch") and torch.equal(ya, yb)
    ya.square().sum().backward()
    yb.square().sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert (p.grad is None and q.grad is None) or torch.equal(p.grad, q.grad), k


@pytest.mark.parametrize("B,T,N,C,hid", MODELS)
def test_model_inputs_tell_a_wrong_model_from_a_right_one(B, T, N, C, hid):
    m, x, _ = _model(B, T, N, C, hid)
    want = m(x)
    assert _err(gu.restated(m, x, order=(0, 2, 1, 3))[0], want) > 1e-2     # f and g exchanged
    assert _err(gu.restated(m, x, order=(3, 1, 2, 0))[0], want) > 1e-2     # i and o exchanged
    if T > 1:
        assert _err(gu.restated(m, x, last=False)[0], want) > 1e-2         # the h_{T-1} term dropped


@pytest.mark.parametrize("units,N,C", gu.SEN_CASES)
def test_semantic_formulas_equal_autograd(units, N, C):
    x, V, c, dz = gu.sen_inputs(units, N, C)
    x, V, c = x.requires_grad_(True), V.requires_grad_(True), c.requires_grad_(True)
    z = torch.stack([x[r] @ V[r % N] + c[r % N] for r in range(units * N)])  # row by row
    assert _err(gu.sen_fwd(x, V, c, N), z) < EXACT
    want = torch.autograd.grad((z * dz).sum(), [x, V, c])
    for got, ref in zip(gu.sen_bwd(x.detach(), V.detach(), dz, N), want):
        assert _err(got, ref) < EXACT
