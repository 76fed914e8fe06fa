"""``TGCN(..., backend="hip")`` without a GPU: the switch, the fallback on CPU tensors, the command-line option, the predictor's argument set,
and the algebra the HIP path rests on — the padded, split, hoisted form of the recurrence built from ``tgcn_hip.pack`` — in plain torch."""
import types

import pytest
import torch

from gptst_amd import graph
from gptst_amd.config import FINETUNE_DEFAULTS, make_args, parse_args, predictor_args
from gptst_amd.predictors import TGCN, tgcn_hip as H

N, C, HID, T = 20, 64, 100, 12


def _ap(n=N, hid=HID, out=1, t=T):
    return types.SimpleNamespace(num_nodes=n, input_window=t, output_window=t, rnn_units=hid, output_dim=out,
                                 G=graph.tgcn_graph(graph.synthetic_adjacency(n, 2)))


def test_backend_switch_and_fallback_on_cpu_tensors():
    torch.manual_seed(0)
    mh, mt = TGCN(_ap(), "cpu", C, backend="hip"), TGCN(_ap(), "cpu", C)
    mt.load_state_dict(mh.state_dict(), strict=True)
    assert (mh.backend, mh.backend_used, mt.backend) == ("hip", None, "torch")
    x = torch.randn(2, T, N, C)
    assert not H.supported(mh, x)
    yh, yt = mh(x), mt(x)
    assert mh.backend_used == "torch" and mt.backend_used == "torch" and torch.equal(yh, yt) and yh.requires_grad
    with pytest.raises(ValueError):
        TGCN(_ap(), "cpu", C, backend="eager")


def test_tgcn_backend_option():
    base = ["-dataset", "PEMS08", "-mode", "eval", "-model", "TGCN"]
    a = parse_args("cpu", base)
    assert (a.tgcn_backend, a.stgcn_backend, a.model) == ("torch", "torch", "TGCN")
    a = parse_args("cpu", base + ["-tgcn_backend", "hip"])
    assert (a.tgcn_backend, a.stgcn_backend) == ("hip", "torch")
    assert make_args("PEMS08", mode="eval").tgcn_backend == "torch" and FINETUNE_DEFAULTS["tgcn_backend"] == "torch"
    with pytest.raises(SystemExit):
        parse_args("cpu", base + ["-tgcn_backend", "eager"])


@pytest.mark.parametrize("ds,n,out,seed", [("PEMS08", 170, 1, 12), ("METR_LA", 207, 1, 0), ("NYC_TAXI", 266, 2, 12), ("NYC_BIKE", 250, 2, 12)])
def test_predictor_args(ds, n, out, seed):
    p = predictor_args(ds, "TGCN")
    assert (p.num_nodes, p.input_window, p.output_window, p.rnn_units, p.lam, p.output_dim) == (n, 12, 12, 100, 0.0015, out)
    assert (p.seed, p.seed_mode, p.xavier, p.loss_func, p.batch_size, p.epochs) == (seed, True, False, "mask_mae", 64, 100)
    assert predictor_args(ds, "TGCN", ["--rnn_units", "64"]).rnn_units == 64
    with pytest.raises(ValueError):
        predictor_args(ds, "GWN")


def _hoisted(m, x, packed):
    """the HIP path's arithmetic in torch: L X hoisted, the gate GEMMs split into an x half (with the bias) and an h half, H padded to Hp"""
    P0, pb0, P1, pb1 = packed
    B, Hp, L = x.shape[0], P1.shape[0], m.tgcn_model.L
    LX = torch.matmul(L, x)                                             # (B, T, N, C)
    Gx0, Gx1 = LX @ P0[:, :C].t() + pb0, LX @ P1[:, :C].t() + pb1
    h, hs = x.new_zeros(B, N, Hp), []
    for t in range(x.shape[1]):
        g = torch.sigmoid(torch.matmul(L, h) @ P0[:, C:].t() + Gx0[:, t])
        r, u = g[..., :Hp], g[..., Hp:]
        c = torch.tanh(torch.matmul(L, r * h) @ P1[:, C:].t() + Gx1[:, t])
        h = u * h + (1 - u) * c
        hs.append(h)
    return h, hs


@pytest.mark.parametrize("hid", [100, 32])
def test_packing_algebra(hid):
    torch.manual_seed(1)
    m = TGCN(_ap(hid=hid, t=4), "cpu", C).double()
    with torch.no_grad():
        m.tgcn_model.bias_0.normal_(0, 0.3)
        m.tgcn_model.bias_1.normal_(0, 0.3)
    cell = m.tgcn_model
    x = torch.randn(2, 4, N, C, dtype=torch.float64)
    w = torch.randn(2, 4, N, 1, dtype=torch.float64)
    y = m(x)
    (y * w).sum().backward()
    want = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad()
    packed = H.pack(cell.weights_0, cell.bias_0, cell.weights_1, cell.bias_1, C, hid)
    Hp = H.padded(hid)
    assert Hp % 16 == 0 and 0 <= Hp - hid < 16
    assert [tuple(p.shape) for p in packed] == [(2 * Hp, C + Hp), (2 * Hp,), (Hp, C + Hp), (Hp,)]
    h, hs = _hoisted(m, x, packed)
    # 1. the padded, split, hoisted recurrence is the module's forward
    y2 = m.head(h[..., :hid])
    assert float((y2 - y).detach().abs().max()) < 1e-12 * float(y.detach().abs().max())
    # 2. a padded channel stays exactly 0 in every state
    assert all(bool((s[..., hid:] == 0).all()) for s in hs)
    # 3. unpacking: the gradients of the packed tensors go back to the parameters through the packing, the padding's are dropped
    for p in packed:
        p.retain_grad()
    (y2 * w).sum().backward()
    for k, p in m.named_parameters():
        assert float((p.grad - want[k]).abs().max()) <= 1e-11 * float(want[k].abs().max()), k
    dP0, db0, dP1, db1 = (p.grad for p in packed)
    W0g = torch.cat([dP0[:hid], dP0[Hp:Hp + hid]], 0)[:, :C + hid].t()                # (C + H, 2 H): [r columns | u columns]
    assert torch.equal(cell.weights_0.grad, W0g) and torch.equal(cell.weights_1.grad, dP1[:hid, :C + hid].t())
    assert torch.equal(cell.bias_0.grad, torch.cat([db0[:hid], db0[Hp:Hp + hid]])) and torch.equal(cell.bias_1.grad, db1[:hid])
    # the same map applied to made-up packed gradients (padding rows and columns non-zero: they must not leak)
    g0 = torch.randn_like(packed[0])
    (dW0,) = torch.autograd.grad(H.pack(cell.weights_0, cell.bias_0, cell.weights_1, cell.bias_1, C, hid)[0], cell.weights_0, g0)
    assert torch.equal(dW0, torch.cat([g0[:hid], g0[Hp:Hp + hid]], 0)[:, :C + hid].t())
