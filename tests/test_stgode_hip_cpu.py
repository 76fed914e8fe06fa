"""What predictors/stgode_hip.py computes launch by launch, transcribed in float64 torch (tests/stgode_util.py) and held to autograd on the
module at 1e-10: the step with its coefficients 3 alpha, 6, 6, -11; its hand-written backward with -17 and alpha on the SOURCE rows (x0 is
detached in the reference, so the backward is not the derivative of the forward expression); the dalpha, dW and dW2 reductions; the batch
norm over the node channel forward and backward; the routing of the max.  No kernel runs here: this pins the arithmetic the kernels are then
tested against (tests/test_gpu_stgode_hip.py).  At the widths 16 and 48: the GPU tests run the definitions at widths that are no multiple of
32, so the yardstick is pinned at one of them as well."""
import pytest
import torch

import stgode_util as gu
from gptst_amd.predictors import STGODE

TOL = 1e-10
N, T, P, B = 9, 4, 2, 2
WIDTHS = (16, 48)


def _err(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _model(n_layers=2, seed=3, redraw=True, width=16):
    torch.manual_seed(seed)
    m = STGODE(gu.model_args(N, T=T, P=P, n_layers=n_layers, out_channels=(width, width // 2, width), in_channels=width), "cpu", width, 1)
    if redraw:
        gu.xavier_redraw_(m)
    return m.double().train()


def test_step_forward_is_the_module_s_euler_step():
    for C in WIDTHS:
        m = _model(width=C)
        blk, A = m.sp_blocks[0][0], m.A_sp
        X = torch.randn(B, T, N, C, dtype=torch.float64)
        alpha, W, W2 = (t.detach() for t in blk.odeg.odeblock.odefunc.mats())
        z, At, _ = gu.step_fwd(X, A, alpha, W, W2)
        assert _err(z, torch.relu(blk.odeg(blk.temporal1(X), A))) < TOL
        assert _err(At, torch.einsum("ij,btjc->btic", A, torch.relu(X))) < TOL
        assert float((z > 0).double().mean()) > 0.1                              # not a dead block


def test_step_backward_has_minus_17_and_alpha_on_the_source_rows():
    for C in WIDTHS:
        m = _model(width=C)
        blk, A = m.se_blocks[1][0], m.A_se
        f = blk.odeg.odeblock.odefunc
        X = torch.randn(B, T, N, C, dtype=torch.float64, requires_grad=True)
        z = torch.relu(blk.odeg(blk.temporal1(X), A))
        dz = torch.randn_like(z)
        z.backward(dz)
        alpha, W, W2 = (t.detach() for t in f.mats())
        g = dz * (z > 0)
        assert _err(gu.step_bwd(g, X.detach(), A, alpha, W, W2), X.grad) < TOL
        # the derivative of the forward EXPRESSION (-11) is another function: the test can tell them apart
        wrong = gu.step_bwd(g, X.detach(), A, alpha, W, W2) + 6 * g * (X.detach() > 0)
        assert _err(wrong, X.grad) > 1e-2
        # ... and so can it a transposed graph or alpha on the output side
        dt_out = 3 * alpha[:, None] * torch.einsum("ji,btjc->btic", A, g) + 6 * (g @ W.t()) + 6 * torch.einsum("km,bmnc->bknc", W2, g) - 17 * g
        assert _err(dt_out * (X.detach() > 0), X.grad) > 1e-3
        # the reductions, through torch's chains back to the parameters
        _, At, _ = gu.step_fwd(X.detach(), A, alpha, W, W2)
        da, dW, dW2 = gu.step_param_grads(g, X.detach(), At)
        al, Wm, W2m = f.mats()
        want = torch.autograd.grad([al, Wm, W2m], [f.alpha, f.w, f.d, f.w2, f.d2], [da, dW, dW2])
        for k, w in zip(("alpha", "w", "d", "w2", "d2"), want):
            assert _err(w, getattr(f, k).grad) < TOL, k


def test_batch_norm_over_the_node_channel_forward_backward_and_buffers():
    for C in WIDTHS:
        m = _model(width=C)
        bn = m.sp_blocks[0][1].batch_norm
        z = torch.relu(torch.randn(B, T, N, C, dtype=torch.float64)).requires_grad_(True)
        y = bn(z.transpose(1, 2)).transpose(1, 2)
        dy = torch.randn_like(y)
        y.backward(dy)
        mine, mean, var, varu = gu.bn_fwd(z.detach(), bn.weight.detach(), bn.bias.detach(), bn.eps)
        assert _err(mine, y) < TOL
        assert _err(0.1 * mean, bn.running_mean) < TOL and _err(0.9 + 0.1 * varu, bn.running_var) < TOL and int(bn.num_batches_tracked) == 1
        dz, dg, db = gu.bn_bwd(dy, z.detach(), bn.weight.detach(), mean, var, bn.eps)
        assert _err(dz, z.grad) < TOL and _err(dg, bn.weight.grad) < TOL and _err(db, bn.bias.grad) < TOL
        bn.eval()
        assert _err(gu.bn_eval(z.detach(), bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps),
                    bn(z.detach().transpose(1, 2)).transpose(1, 2)) < TOL


@pytest.mark.parametrize("redraw,C", [pytest.param(True, 16, id="True"), pytest.param(False, 16, id="False"), pytest.param(True, 48, id="True-w48"),
                                      pytest.param(False, 48, id="False-w48")])
def test_whole_trunk_by_hand_equals_autograd(redraw, C):
    """redraw=False: the default initialisation, where the branches of a graph tie exactly and the lowest index takes the gradient"""
    m = _model(redraw=redraw, width=C)
    x = torch.randn(B, T, N, C, dtype=torch.float64, requires_grad=True)
    outs = []
    for seq, A in m.branches():
        h = x
        for blk in seq:
            h = blk(h, A)
        outs.append(h)
    best = torch.max(torch.stack(outs), dim=0)[0]
    dB = torch.randn_like(best)
    best.backward(dB)
    for bn in (b.batch_norm for seq, _ in m.branches() for b in seq):         # model_manual reads the affine only
        assert int(bn.num_batches_tracked) == 1
    res = gu.model_manual(m, x.detach(), dB)
    assert _err(res["best"], best) < TOL and _err(res["dx"], x.grad) < TOL
    assert torch.equal(res["which"].long(), torch.stack(outs).max(0)[1])
    if not redraw:
        assert set(res["which"].unique().tolist()) == {0, 2}
    for r in res["recs"]:
        f, bn = r["blk"].odeg.odeblock.odefunc, r["blk"].batch_norm
        al, Wm, W2m = f.mats()
        want = torch.autograd.grad([al, Wm, W2m], [f.alpha, f.w, f.d, f.w2, f.d2], [r["dalpha"], r["dW"], r["dW2"]])
        for k, w in zip(("alpha", "w", "d", "w2", "d2"), want):
            assert _err(w, getattr(f, k).grad) < TOL or (not bool(w.any()) and not bool(getattr(f, k).grad.any())), (r["branch"], k)
        for mine, ref in ((r["dgamma"], bn.weight.grad), (r["dbeta"], bn.bias.grad)):
            assert _err(mine, ref) < TOL or (not bool(mine.any()) and not bool(ref.any())), r["branch"]
