"""The Python of the CCRNN HIP path without a GPU (predictors/ccrnn_hip.py): the packing of the reference's column order, the polynomial stack,
what ``supported`` refuses, the LDS size entry — and the whole path, autograd functions and all, run in float64 on the torch restatements of
its launches (ccrnn_util.REF_OPS) against the torch backend and the golden vectors: what the GPU tests then hold the real launches to."""
import random

import pytest
import torch

import ccrnn_util as gu
from gptst_amd import _C, ops
from gptst_amd.predictors import CCRNN, ccrnn_hip
from gptst_amd.predictors.rows_hip import mirror
from golden_util import load

G = load("ccrnn_small.npz")
B, T, N, C, OUT, H = 2, 12, 20, 64, 2, 25
TOL = 1e-5                 # both sides float64


def _err(got, ref):
    ref = torch.as_tensor(ref).detach().double()
    return float((got.detach().double().reshape(ref.shape) - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


@pytest.fixture
def on_ref_ops(monkeypatch):
    """the launches replaced by their restatements, and the CUDA-only conditions lifted"""
    for k, f in gu.REF_OPS.items():
        monkeypatch.setattr(ops, k, f)
    monkeypatch.setattr(ccrnn_hip, "is_hip_input", lambda x: x.dim() == 4)
    monkeypatch.setattr(_C, "lib", lambda: type("L", (), {"value": staticmethod(lambda *a: 1)})())


@pytest.mark.parametrize("Cin,Hh,gates,M", [(2, 25, 2, 4), (64, 25, 1, 4), (25, 16, 2, 2), (3, 32, 1, 3)])
def test_pack_round_trips_the_column_order(Cin, Hh, gates, M):
    g = torch.Generator().manual_seed(Cin + Hh)
    W, b = torch.randn(gates * Hh, (Cin + Hh) * M, generator=g, dtype=torch.float64), torch.randn(gates * Hh, generator=g, dtype=torch.float64)
    Wh, Wi, pb = ccrnn_hip.pack_cell(W, b, Cin, Hh, gates, M)
    Hp = 16 * ((Hh + 15) // 16)
    assert tuple(Wh.shape) == (gates * Hp, M, Hp) and tuple(Wi.shape) == (gates * Hp, M, Cin) and tuple(pb.shape) == (gates * Hp,)
    z = torch.randn(5, Cin + Hh, M, generator=g, dtype=torch.float64)           # [input | state] channels of M matrices, as the Linear reads them
    want = z.reshape(5, -1) @ W.t() + b
    zi, zh = z[:, :Cin].permute(0, 2, 1), torch.nn.functional.pad(z[:, Cin:], (0, 0, 0, Hp - Hh)).permute(0, 2, 1)
    got = (torch.einsum("nmc,omc->no", zh, Wh) + torch.einsum("nmc,omc->no", zi, Wi) + pb).view(5, gates, Hp)
    assert _err(got[:, :, :Hh].reshape(5, -1), want) < 1e-12 and not bool(got[:, :, Hh:].any())      # a padded output is exactly 0
    Cp = 16 * ((Cin + 15) // 16)
    Ws = ccrnn_hip.slab_weight(Wh, Wi, Cp)
    slab = torch.cat([zh, torch.nn.functional.pad(zi, (0, Cp - Cin))], 2).reshape(5, -1)            # [state | input] per matrix
    assert tuple(Ws.shape) == (gates * Hp, M * (Hp + Cp)) and _err((slab @ Ws.t() + pb).view(5, gates, Hp)[:, :, :Hh].reshape(5, -1), want) < 1e-12
    assert torch.equal(gu.matrix_major(W, Cin + Hh, M).view(-1, M, Cin + Hh)[:, :, :Cin], Wi.view(gates, Hp, M, Cin)[:, :Hh].reshape(-1, M, Cin))
    assert tuple(mirror(Ws, M).shape) == (Hp + Cp, M * gates * Hp)


@pytest.mark.parametrize("n,k", [(20, 3), (37, 3), (20, 1), (16, 2)])
def test_polynomial_stack_equals_the_recursion(n, k):
    S = torch.tensor(gu.support(n)).double() * 1.5
    z = torch.randn(n, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
    P = ccrnn_hip.poly_stack(S, k)
    x0, x1, outs = z, S @ z, []
    outs.append(x1)
    for _ in range(2, k + 1):                                                  # the reference's recursion on the operand (CCRNN.py:224-229)
        x2 = 2 * S @ x1 - x0
        outs.append(x2)
        x1, x0 = x2, x1
    assert tuple(P.shape) == (k, n, n) and torch.equal(P, gu.poly_stack(S, k))
    for j in range(k):
        assert _err(P[j] @ z, outs[j]) < 1e-12, j


def test_supported_refuses_each_unserved_setting(on_ref_ops):
    x = torch.zeros(1, 3, N, C)

    def ok(x=x, **kw):
        return ccrnn_hip.supported(CCRNN(gu.model_args(N, gu.support(N), **kw), "cpu", x.shape[3], OUT, backend="hip"), x)

    assert ok() and ok(rnn=2) and ok(k_hop=1) and ok(H=32) and ok(H=16) and ok(x=torch.zeros(1, 3, N, 128)) and ok(x=torch.zeros(1, 3, N, 16))
    assert not ok(gconv=3) and not ok(gconv=2) and not ok(rnn=3) and not ok(n_supports=2) and not ok(k_hop=0) and not ok(k_hop=4) and not ok(H=33)
    assert not ok(x=torch.zeros(1, 3, N, 24)) and not ok(x=torch.zeros(1, 3, N, 144))
    m = CCRNN(gu.model_args(N, gu.support(N)), "cpu", C, OUT, backend="hip")
    assert not ccrnn_hip.supported(m, torch.zeros(1, 3, N + 1, C)) and not ccrnn_hip.supported(m, torch.zeros(3, N, C))
    assert not ccrnn_hip.supported(CCRNN(gu.model_args(N, gu.support(N)), "cpu", C, 17, backend="hip"), x)
    assert ccrnn_hip.slab_widths(m) == [16] and ccrnn_hip.slab_widths(CCRNN(gu.model_args(N, gu.support(N), rnn=2), "cpu", C, OUT)) == [16, 32]


def test_cpu_input_fp32_or_fp64_is_not_served_without_the_patches():
    m = CCRNN(gu.model_args(N, gu.support(N)), "cpu", C, OUT, backend="hip")
    m(torch.zeros(1, 2, N, C))
    assert m.backend_used == "torch" and not ccrnn_hip.is_hip_input(torch.zeros(1, 2, N, C))
    m.backend_used = None
    m.double()(torch.zeros(1, 2, N, C, dtype=torch.float64))
    assert m.backend_used == "torch" and not ccrnn_hip.is_hip_input(torch.zeros(1, 2, N, C, dtype=torch.float64))


def test_the_conf_size_tests_need_the_smaller_node_vector_noise():
    """why test_gpu_ccrnn_hip.py passes vec = 0.004 to ``perturb_`` at N = 266: at 0.05 the fp32 TORCH backend itself is further than the 1e-4
    bound from fp64 (4e-2 at this test's 3 decoder steps, 1.6 at the GPU test's 12: chaos, ccrnn_util.perturb_), so no fp32 implementation could
    be held to it; at 0.004 it is well inside (3e-7)"""
    n = 266
    gap = {}
    for vec in (0.05, 0.004):
        torch.manual_seed(gu.SEED)
        m32 = gu.perturb_(CCRNN(gu.model_args(n, gu.support(n), n_dim=50, P=3), "cpu", 16, OUT), vec)
        m64 = CCRNN(gu.model_args(n, gu.support(n), n_dim=50, P=3), "cpu", 16, OUT).double()
        m64.load_state_dict(m32.state_dict())
        x = torch.randn(1, 12, n, 16, generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            gap[vec] = _err(m32(x), m64(x.double()))
    print("fp32 torch against fp64 torch at N = 266:", gap)
    assert gap[0.05] > 1e-4 and gap[0.004] < 1e-5, gap


def test_lds_size_entry():
    v = lambda *a: _C.lib().value("gptst_ccrnn_lds_bytes", *a)                  # noqa: E731
    # (Np 68 + 16 tiles ((k + 1) max(Hp + Cp, 2 Hp) + 4)) floats: one tile per workgroup at B = 1, two once B ceil(tiles / 2) > 256
    assert v(266, 32, 16, 3, 1) == (272 * 68 + 16 * (4 * 64 + 4)) * 4 and v(266, 32, 16, 3, 64) == (272 * 68 + 32 * (4 * 64 + 4)) * 4
    assert v(20, 16, 0, 1, 1) == (32 * 68 + 16 * (2 * 32 + 4)) * 4 and v(250, 32, 32, 3, 64) == (256 * 68 + 32 * (4 * 64 + 4)) * 4
    assert v(266, 32, 16, 3, 64) <= 160 * 1024 and v(2200, 32, 32, 3, 64) > 160 * 1024
    assert v(20, 48, 0, 3, 1) == -2 and v(20, 32, 48, 3, 1) == -2 and v(20, 32, 16, 4, 1) == -2 and v(20, 32, 8, 3, 1) == -2 and v(0, 32, 16, 3, 1) == -1


@pytest.mark.parametrize("run", ["free", "tf"])
@pytest.mark.parametrize("rnn", [1, 2])
def test_the_path_on_restated_launches_reproduces_the_golden_vectors(on_ref_ops, rnn, run):
    m = CCRNN(gu.model_args(N, G["support"], rnn=rnn), "cpu", C, OUT, backend="hip")
    pre = gu.tag(rnn, 1) + ".sd."
    m.load_state_dict({k[len(pre):]: torch.tensor(G[k]) for k in G.files if k.startswith(pre)}, strict=True)
    m.double().train()
    x = torch.tensor(G["x"]).double().requires_grad_(True)
    random.seed(int(G["tf_seed"]))
    y = m(x, torch.tensor(G["targets"]).double() if run == "tf" else None)
    assert m.backend_used == "hip"
    (y * torch.tensor(G["w"]).double()).sum().backward()
    pre = "%s.%s." % (gu.tag(rnn, 1), run)
    assert _err(y, G[pre + "y"]) < TOL and _err(x.grad, G[pre + "dx"]) < TOL
    for k, p in m.named_parameters():
        if k in ("w1", "w2", "b1", "b2"):
            assert p.grad is None, k
        elif "attlinear" in k:
            assert p.grad is not None and not bool(p.grad.any()), k
        else:
            assert _err(p.grad, G[pre + "grad." + k]) < TOL, k


def test_a_forced_step_sends_no_gradient_into_its_output_and_eval_keeps_nothing(on_ref_ops, monkeypatch):
    m = CCRNN(gu.model_args(N, G["support"], P=3), "cpu", C, OUT, backend="hip").double().train()
    x, t = torch.tensor(G["x"]).double()[:1, :2], torch.tensor(G["targets"]).double()[:1, :3]
    grads = {}
    for name, draw in (("all forced", 0.0), ("none forced", 1.0)):
        monkeypatch.setattr(random, "random", lambda d=draw: d)
        y = m(x, t)
        grads[name], = torch.autograd.grad(y[:, 2].sum(), m.decoder.out.bias)
    # forced: y_2 meets out.bias once per node, nothing of y_0 and y_1 travels on; fed back, the bias reaches y_2 through two more cells
    assert torch.equal(grads["all forced"], torch.full((OUT,), float(N), dtype=torch.float64))
    assert float((grads["none forced"] - N).abs().min()) > 1e-3
    m.eval()
    ye = m(x, t)
    assert m.backend_used == "hip" and not ye.requires_grad and _err(ye, y) < 1e-12
