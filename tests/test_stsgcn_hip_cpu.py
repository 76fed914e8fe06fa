"""The block algebra predictors/stsgcn_hip.py computes, in fp64 torch on the CPU against the STSGCN module (whose torch backend keeps the dense
(3N, 3N) product and is pinned to the reference's vectors by tests/test_predictor_stsgcn.py): the mix as blocks, the middle-only last operation,
the routing of the max, the fold of the window-expanded gradient onto the frames, the stacked heads.  Agreement to 1e-10 in the output and
every gradient, at T = 5 (windows fed by one, two and three blocks) and T = 12 (the confs')."""
import pytest
import torch

import stsgcn_util as su
from gptst_amd.predictors import STSGCN

TOL = 1e-10


def _model(T, layers, module_type="individual", dim_out=1, seed=3):
    torch.manual_seed(seed)
    m = STSGCN(su.model_args(20, T=T, P=3, layers=layers, module_type=module_type), "cpu", 64, dim_out)
    su.randomize_embeddings_(m)
    return m.double()


def _err(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("T,layers,module_type,dim_out", [(5, 1, "individual", 1), (5, 1, "sharing", 2), (12, 4, "individual", 1), (12, 2, "sharing", 2)])
def test_block_algebra_is_the_module(T, layers, module_type, dim_out):
    m = _model(T, layers, module_type, dim_out)
    x, w = torch.randn(2, T, 20, 64, dtype=torch.float64), torch.randn(2, 3, 20, dim_out, dtype=torch.float64)
    res = []
    for f in (m, lambda t: su.model_blocks(m, t)):
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        y = f(xi)
        (y * w).sum().backward()
        res.append(dict({"y": y.detach(), "dx": xi.grad}, **{k: p.grad.clone() for k, p in m.named_parameters()}))
    want, got = res
    assert set(got) == set(want) and all(float(v.abs().max()) > 0 for v in want.values())
    errs = {k: _err(got[k], want[k]) for k in want}
    assert all(v <= TOL for v in errs.values()), {k: v for k, v in errs.items() if v > TOL}


@pytest.mark.parametrize("T,module_type", [(5, "individual"), (12, "individual"), (6, "sharing")])
def test_hand_written_backward_of_a_layer(T, module_type):
    """the launch sequence of LayerFn — gate backward with the winner index, weight gradient per window, mirrored GEMM, the three adjoint forms
    of the mix — against autograd through the module's layer"""
    m = _model(T, 1, module_type)
    lay, a_hat = m.stsgcl_layers[0].layer, m.a_hat
    H = torch.randn(2, T, 20, 16, dtype=torch.float64, requires_grad=True)
    dBest = torch.randn(2, T - 2, 20, 16, dtype=torch.float64)
    cands = lay.candidates(H, m.adj)
    best = cands.max(0)[0]
    (best * dBest).sum().backward()
    assert su.ambiguous(cands.detach(), gap=1e-9)[0] == 0              # both sides are fp64 (rounding 1e-16): no winner within 1e-9 can differ
    gb, which, dH, dWs, dbs = su.layer_manual(lay, a_hat, H.detach(), dBest)
    assert torch.equal(which.long(), cands.argmax(0)) and set(which.unique().tolist()) == {0, 1, 2}
    errs = {"best": _err(gb, best.detach()), "dH": _err(dH, H.grad)}
    for j in range(3):
        ops_j = [g.layers[j].layer for g in (lay.gcms if lay.individual else [lay.gcm])]
        dW = dWs[j] if lay.individual else dWs[j].sum(0, keepdim=True)
        db = dbs[j] if lay.individual else dbs[j].sum(0, keepdim=True)
        for wdx, op in enumerate(ops_j):
            errs["dW%d.%d" % (j, wdx)], errs["db%d.%d" % (j, wdx)] = _err(dW[wdx], op.weight.grad), _err(db[wdx], op.bias.grad)
    assert all(v <= TOL for v in errs.values()), {k: v for k, v in errs.items() if v > TOL}


def test_fold_is_the_adjoint_of_expand_and_the_gathered_form_agrees():
    g = torch.Generator().manual_seed(1)
    A = torch.randn(20, 20, generator=g, dtype=torch.float64)
    for W in (1, 2, 3, 10):
        H = torch.randn(2, W + 2, 20, 4, generator=g, dtype=torch.float64)
        G = torch.randn(2, W, 3, 20, 4, generator=g, dtype=torch.float64)
        assert abs(float((su.expand(H) * G).sum() - (H * su.fold(G)).sum())) < 1e-9
        assert abs(float((su.mix_f2e(A, H) * G).sum() - (H * su.mix_e2f(A.t(), G)).sum())) < 1e-9
        assert float((su.mix_e2f(A.t(), G) - su.fold(su.mix_expanded(A.t(), G))).abs().max()) < 1e-12
        g1 = G[:, :, 1]
        assert abs(float((su.mix_middle(A, G) * g1).sum() - (G * su.mix_m2e(A.t(), g1)).sum())) < 1e-9
        assert abs(float((su.mix_expanded(A, G) * G.flip(0)).sum() - (G * su.mix_expanded(A.t(), G.flip(0))).sum())) < 1e-9
