"""The block algebra predictors/stfgnn_hip.py computes, in fp64 torch on the CPU against the STFGNN module (whose torch backend keeps the dense
(4N, 4N) product and is pinned to the reference's vectors by tests/test_predictor_stfgnn.py): every form of the mix and its adjoint, the
middle-only last operation, the shared output of blocks 0 and 3, the routing of the max, the gated branch as one tap GEMM, the hand-written
backward launch by launch.  Agreement to 1e-10 in the output and every gradient, at T = 4 (one window), T = 7 (frames fed by one to four blocks)
and T = 12 (the confs')."""
import pytest
import torch

import stfgnn_util as fu
from gptst_amd import graph
from gptst_amd.predictors import STFGNN

TOL = 1e-10


def _model(T, layers, dim_out=1, seed=3):
    torch.manual_seed(seed)
    m = STFGNN(fu.model_args(20, T=T, P=3, layers=layers, output_dim=dim_out), "cpu", 64)
    fu.randomize_embeddings_(m)
    return m.double()


def _err(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def _graphs(n=20, seed=1):
    g = torch.Generator().manual_seed(seed)
    S, D = torch.randn(n, n, generator=g, dtype=torch.float64), torch.randn(n, n, generator=g, dtype=torch.float64)
    S.fill_diagonal_(1.0)
    D.fill_diagonal_(1.0)
    return g, S, D


def _dense(S, D):
    """the (4N, 4N) matrix of the blocks"""
    n = S.shape[0]
    eye = torch.eye(n, dtype=S.dtype)
    rows = [[D, eye, eye, D], [eye, S, eye, eye], [eye, eye, S, eye], [D, eye, eye, D]]
    return torch.cat([torch.cat(r, 1) for r in rows], 0)


def test_every_mix_form_is_the_dense_product():
    g, S, D = _graphs()
    adj = _dense(S, D)
    assert torch.equal(graph.stfgnn_fusion_graph(S.numpy(), D.numpy()), adj.float())
    for W in (1, 2, 4, 9):
        H = torch.randn(2, W + 3, 20, 4, generator=g, dtype=torch.float64)
        E = torch.randn(2, W, 4, 20, 4, generator=g, dtype=torch.float64)
        M = torch.randn(2, W, 20, 4, generator=g, dtype=torch.float64)
        prod = lambda A, X: (A @ X.reshape(2, W, 80, 4)).reshape(2, W, 4, 20, 4)                                     # noqa: E731
        e2e = fu.mix_expanded(S, D, E)
        assert _err(e2e, prod(adj, E)) < 1e-12 and torch.equal(e2e[:, :, 0], e2e[:, :, 3])                           # blocks 0 and 3 share one output
        assert _err(fu.mix_middle(S, E), prod(adj, E)[:, :, 1]) < 1e-12
        assert _err(fu.mix_f2e(S, D, H), prod(adj, fu.expand(H))) < 1e-12
        # the adjoints, with the transposed graphs: the transposed matrix has the same form
        assert _err(fu.mix_expanded(S.t(), D.t(), E), prod(adj.t(), E)) < 1e-12
        only1 = torch.zeros_like(E)
        only1[:, :, 1] = M
        assert _err(fu.mix_m2e(S.t(), M), prod(adj.t(), only1)) < 1e-12
        assert _err(fu.mix_e2f(S.t(), D.t(), E), fu.fold(prod(adj.t(), E))) < 1e-12


def test_adjoint_identity_of_every_form():
    g, S, D = _graphs(seed=2)
    for W in (1, 2, 3, 9):
        H = torch.randn(2, W + 3, 20, 4, generator=g, dtype=torch.float64)
        G = torch.randn(2, W, 4, 20, 4, generator=g, dtype=torch.float64)
        G2 = torch.randn(2, W, 4, 20, 4, generator=g, dtype=torch.float64)
        M = torch.randn(2, W, 20, 4, generator=g, dtype=torch.float64)
        assert abs(float((fu.expand(H) * G).sum() - (H * fu.fold(G)).sum())) < 1e-9
        assert abs(float((fu.mix_f2e(S, D, H) * G).sum() - (H * fu.mix_e2f(S.t(), D.t(), G)).sum())) < 1e-9
        assert abs(float((fu.mix_expanded(S, D, G) * G2).sum() - (G * fu.mix_expanded(S.t(), D.t(), G2)).sum())) < 1e-9
        assert abs(float((fu.mix_middle(S, G) * M).sum() - (G * fu.mix_m2e(S.t(), M)).sum())) < 1e-9


@pytest.mark.parametrize("T,layers,dim_out", [(4, 1, 1), (7, 2, 2), (12, 3, 1)])
def test_block_algebra_is_the_module(T, layers, dim_out):
    m = _model(T, layers, dim_out)
    x, w = torch.randn(2, T, 20, 64, dtype=torch.float64), torch.randn(2, 3, 20, dim_out, dtype=torch.float64)
    res = []
    for f in (m, lambda t: fu.model_blocks(m, t)):
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        y = f(xi)
        (y * w).sum().backward()
        res.append(dict({"y": y.detach(), "dx": xi.grad}, **{k: p.grad.clone() for k, p in m.named_parameters()}))
    want, got = res
    assert set(got) == set(want) and all(float(v.abs().max()) > 0 for v in want.values())
    errs = {k: _err(got[k], want[k]) for k in want}
    assert all(v <= TOL for v in errs.values()), {k: v for k, v in errs.items() if v > TOL}


@pytest.mark.parametrize("T", [4, 7, 12])
def test_hand_written_backward_of_a_layer(T):
    """the launch sequence of LayerFn — gate backward with the winner index, weight gradient per window, mirrored GEMM, the three adjoint forms
    of the mix — and of _GateFn, against autograd through the module's layer"""
    m = _model(T, 1)
    lay = m.STSGCLS[0]
    H = torch.randn(2, T, 20, 16, dtype=torch.float64, requires_grad=True)
    dOut = torch.randn(2, T - 3, 20, 16, dtype=torch.float64)
    cands = lay.candidates(H, m.adj)
    best = cands.max(0)[0]
    g = lay.gated(H)
    ((best + g) * dOut).sum().backward()
    assert fu.ambiguous(cands.detach(), gap=1e-9)[0] == 0              # both sides are fp64 (rounding 1e-16): no winner within 1e-9 can differ
    gb, which, dH, dWs, dbs = fu.layer_manual(lay, m.s_hat, m.d_hat, H.detach(), dOut)
    gg, dHg, dw1, db1, dw2, db2 = fu.gate_manual(lay, H.detach(), dOut)
    assert torch.equal(which.long(), cands.argmax(0)) and set(which.unique().tolist()) == {0, 1, 2}
    errs = {"best": _err(gb, best.detach()), "gate": _err(gg, g.detach()), "dH": _err(dH + dHg, H.grad),
            "conv1.w": _err(dw1, lay.conv1.weight.grad), "conv1.b": _err(db1, lay.conv1.bias.grad),
            "conv2.w": _err(dw2, lay.conv2.weight.grad), "conv2.b": _err(db2, lay.conv2.bias.grad)}
    assert _err(dw1, lay.conv2.weight.grad) > 1e-2 and _err(dw1.flip(-1), lay.conv1.weight.grad) > 1e-2               # a swapped half or tap would show
    for j in range(3):
        for wdx, op in enumerate(sm.gcn_operations[j].FC for sm in lay.STSGCMS):
            errs["dW%d.%d" % (j, wdx)], errs["db%d.%d" % (j, wdx)] = _err(dWs[j][wdx], op.weight.grad), _err(dbs[j][wdx], op.bias.grad)
    assert all(v <= TOL for v in errs.values()), {k: v for k, v in errs.items() if v > TOL}
