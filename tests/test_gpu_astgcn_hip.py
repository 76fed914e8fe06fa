"""The ASTGCN predictor on HIP (``ASTGCN(..., backend="hip")``, csrc/astgcn.hip, predictors/astgcn_hip.py) on the GPU.  The reference of every
comparison is fp64 torch on the CPU — the definition of a launch, or the torch ASTGCN module (pinned to the reference implementation's vectors by
tests/test_predictor_astgcn.py); the bound is the project's element-wise one, 1e-4 of the reference tensor's largest magnitude, for every
output, dX and parameter gradient."""
import copy
import logging

import pytest
import torch

import astgcn_util as au
from gptst_amd import graph, ops, synth
from gptst_amd.config import make_args
from gptst_amd.predictors import ASTGCN, astgcn_hip as H
from downstream_util import _check, _err
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pad(Tk):
    ks, n = Tk.shape[0], Tk.shape[1]
    npad = 16 * ((n + 15) // 16)
    tp = Tk.new_zeros(ks, npad, npad)
    tp[:, :n, :n] = Tk
    return tp


# ---- 1. the launches against their definitions ---------------------------------------------------------------------------------------------
#         B  T   N   c   K
MIX = [(3, 12, 20, 64, 3),            # a padded tile
       (2, 5, 16, 32, 1),             # no padding, one polynomial, half a channel group
       (2, 12, 37, 64, 2),
       (2, 12, 70, 128, 3)]           # more than four node tiles, two channel groups


@pytest.mark.parametrize("B,T,N,c,K", MIX)
def test_masked_mix_and_its_graph_gradient(B, T, N, c, K, parity):
    """non-symmetric T_k and S, S different for every b: a transposed operand, or one sample's graph used for all, fails"""
    g = torch.Generator().manual_seed(N + c)
    Tk = torch.randn(K, N, N, generator=g, dtype=torch.float64)
    S = torch.softmax(torch.randn(B, N, N, generator=g, dtype=torch.float64), dim=1)
    x = torch.randn(B, T, N, c, generator=g, dtype=torch.float64)
    G = torch.randn(B, T, N, K, c, generator=g, dtype=torch.float64)
    res = torch.randn(B, T, N, c, generator=g, dtype=torch.float64)
    want = {"expand": torch.einsum("kmn,bmn,btmc->btnkc", Tk, S, x).reshape(B * T * N, K * c),
            "reduce": torch.einsum("kmn,bmn,btnkc->btmc", Tk, S, G).reshape(B * T * N, c),
            "attgrad": torch.einsum("kmn,btmc,btnkc->bmn", Tk, x, G)}
    want["reduce_res"] = want["reduce"] + res.reshape(B * T * N, c)
    assert float((S[0] - S[1]).abs().max()) > 1e-3 and float((S[0] - S[0].t()).abs().max()) > 1e-3
    f = lambda t, *shape: t.float().reshape(*shape).contiguous().to(DEV)                       # noqa: E731
    tp, Sd, xd, Gd, rd = _pad(Tk).float().to(DEV), f(S, B, N, N), f(x, B * T * N, c), f(G, B * T * N, K * c), f(res, B * T * N, c)
    got = {"expand": ops.astgcn_attmix(tp, Sd, xd, T, c, reduce=False),
           "reduce": ops.astgcn_attmix(tp, Sd, Gd, T, c, reduce=True),
           "reduce_res": ops.astgcn_attmix(tp, Sd, Gd, T, c, reduce=True, res=rd),
           "attgrad": ops.astgcn_attgrad(tp, xd, Gd, B, T, N)}
    torch.cuda.synchronize()
    _check(parity, {k: _err(got[k], want[k]) for k in want})


@pytest.mark.parametrize("rows,c", [(1003, 16), (1003, 64), (1003, 128), (131077, 16)])
def test_row_layernorm(rows, c, parity):
    """1003 rows: no multiple of the 16 rows of a pass; 131077 rows: more than the 8192 x 16 rows of one sweep of the grid, and the most splits"""
    g = torch.Generator().manual_seed(c)
    x = (torch.randn(rows, c, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    gamma = (1 + 0.3 * torch.randn(c, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = (0.3 * torch.randn(c, generator=g, dtype=torch.float64)).requires_grad_(True)
    dy = torch.randn(rows, c, generator=g, dtype=torch.float64)
    y = torch.nn.functional.layer_norm(x, (c,), gamma, beta, 1e-5)
    y.backward(dy)
    xd, gd, bd, dyd = (t.detach().float().to(DEV) for t in (x, gamma, beta, dy))
    yd, mean, rstd = ops.astgcn_rowln_fwd(xd, gd, bd, 1e-5, keep=True)
    y0, m0, r0 = ops.astgcn_rowln_fwd(xd, gd, bd, 1e-5, keep=False)
    assert m0 is None and r0 is None and torch.equal(y0, yd)
    dx = ops.astgcn_rowln_bwd(dyd, xd, gd, mean, rstd)
    dg, db = ops.astgcn_rowln_bwd_param(dyd, xd, mean, rstd)
    torch.cuda.synchronize()
    _check(parity, {"y": _err(yd, y), "mean": _err(mean, x.detach().mean(1)), "dx": _err(dx, x.grad), "dgamma": _err(dg, gamma.grad),
                    "dbeta": _err(db, beta.grad)})


# ---- 2. the whole model ----------------------------------------------------------------------------------------------------------------------
def _ap(N, K=3, **kw):
    return au.model_args(N, graph.astgcn_graph(au.nonsymmetric_adjacency(N), K), K=K, **kw)


def _pair(N, K=3, dim_in=64, dim_out=1, seed=5, **kw):
    """(fp64 torch module on the CPU, its fp32 copy on the GPU with backend hip), with the parameter set of the golden vectors"""
    torch.manual_seed(seed)
    m64 = ASTGCN(_ap(N, K, **kw), "cpu", dim_in, dim_out)
    au.xavier_pass_(m64)
    au.move_score_vectors_(m64)
    m64 = m64.double().train()
    mh = copy.deepcopy(m64).float().to(DEV)
    mh.backend = "hip"
    return m64, mh.train()


def _run(m, x, w):
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    y = m(xi)
    (y * w).sum().backward()
    out = {"y": y.detach(), "dx": xi.grad}
    out.update({k: p.grad.clone() for k, p in m.named_parameters()})
    return out


@pytest.mark.parametrize("N,K", [(20, 3), (70, 3)])
def test_whole_model_against_fp64_torch(N, K, parity):
    m64, mh = _pair(N, K)
    torch.manual_seed(N)
    x, w = torch.randn(2, 12, N, 64, dtype=torch.float64), torch.randn(2, 12, N, 1, dtype=torch.float64)
    zs = []
    with au.recorded_sigmoids(zs):
        want = _run(m64, x, w)
    au.assert_condition(zs, {k: v for k, v in want.items() if k not in ("y", "dx")})
    got = _run(mh, x.float().to(DEV), w.float().to(DEV))
    assert m64.backend_used == "torch" and mh.backend_used == "hip" and set(got) == set(want) and len(want) == 42
    _check(parity, {k: _err(got[k], want[k]) for k in want})


# ---- 3. behaviour ----------------------------------------------------------------------------------------------------------------------------
def test_repeatable_and_nothing_saved_without_a_backward(monkeypatch):
    _, mh = _pair(37, 2)
    torch.manual_seed(1)
    x, w = torch.randn(2, 12, 37, 64, device=DEV), torch.randn(2, 12, 37, 1, device=DEV)
    a, b = _run(mh, x, w), _run(mh, x, w)
    assert mh.backend_used == "hip" and all(torch.equal(a[k], b[k]) for k in a)
    stats, saved = [], []
    ln = ops.astgcn_rowln_fwd

    def ln_fwd(*args, **kw):
        out = ln(*args, **kw)
        stats.append(out[1] is not None or out[2] is not None)
        return out
    monkeypatch.setattr(ops, "astgcn_rowln_fwd", ln_fwd)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(1) or t, lambda t: t):
        y_train = mh(x.clone().requires_grad_(True))
        n_train = len(saved)
        assert n_train > 0 and stats == [True, True]
        for mode in ("no_grad", "eval"):
            stats.clear(), saved.clear()
            if mode == "no_grad":
                with torch.no_grad():
                    y = mh(x)
            else:
                mh.eval()
                y = mh(x.clone().requires_grad_(True))
            assert torch.equal(y, y_train) and mh.backend_used == "hip" and not y.requires_grad and y.grad_fn is None
            assert saved == [] and stats == [False, False], (mode, len(saved), stats)


def test_state_dict_loads_strictly_both_ways_between_backends():
    torch.manual_seed(0)
    ap = _ap(20)
    mt, mh = ASTGCN(ap, DEV, 64, 1), ASTGCN(ap, DEV, 64, 1, backend="hip")
    au.xavier_pass_(mt)
    assert len(mt.state_dict()) == 40 and list(mt.state_dict()) == list(mh.state_dict())
    mh.load_state_dict(mt.state_dict(), strict=True)
    mt.load_state_dict(mh.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(mt.state_dict().values(), mh.state_dict().values()))


@pytest.mark.parametrize("kw", [dict(time_strides=2), dict(width=24)])
def test_unsupported_configuration_takes_the_torch_modules(kw):
    """a strided time convolution, or a width the kernels do not serve: the forward is the torch backend's, bit for bit (with the convolution
    library's deterministic algorithms selected, as in the STGCN test; the setting is put back)"""
    torch.manual_seed(4)
    ap = _ap(20, **kw)
    mh, mt = ASTGCN(ap, DEV, 64, 1, backend="hip"), ASTGCN(ap, DEV, 64, 1)
    au.xavier_pass_(mh)
    au.move_score_vectors_(mh)
    mt.load_state_dict(mh.state_dict(), strict=True)
    x = torch.randn(2, 12, 20, 64, device=DEV)
    assert not H.supported(mh, x)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yh, yt = mh(x), mt(x)
    finally:
        torch.backends.cudnn.deterministic = was
    assert mh.backend_used == "torch" and mt.backend_used == "torch" and yh.shape == (2, 12, 20, 1)
    assert torch.equal(yh, yt), float((yh - yt).abs().max())


# ---- 4. the chain ----------------------------------------------------------------------------------------------------------------------------
def _front_end(tmp_path, backend, sd, psd):
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    N = 20
    args = make_args("PEMS08", mode="eval", num_nodes=N, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros(), batch_size=8, epochs=3,
                     early_stop=False, log_dir=str(tmp_path), debug=True, model="ASTGCN_test", astgcn_backend=backend)
    sd = O.init_state_dict(args, 4) if sd is None else sd
    torch.manual_seed(0)
    pred = ASTGCN(_ap(N), DEV, args.hidden_dim, args.output_dim, backend=args.astgcn_backend)
    if psd is None:
        au.xavier_pass_(pred)
        au.move_score_vectors_(pred)
    else:
        pred.load_state_dict(psd, strict=True)
    model = EnhanceFrontEnd(args, predictor=pred, finetune_encoder=False).to(DEV)
    model.load_pretrained_model(sd)
    return args, sd, model, EvalTrainer


def test_chain_one_step_agrees_with_the_torch_backend(tmp_path, parity):
    args, sd, mh, ET = _front_end(tmp_path, "hip", None, None)
    _, _, mt, _ = _front_end(tmp_path, "torch", sd, mh.predictor.state_dict())
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
        res[name] = (float(loss.detach()), {k: p.grad for k, p in model.named_parameters() if p.requires_grad})
    assert set(res["hip"][1]) == set(res["torch"][1]) and len(res["hip"][1]) == 6 + 2 + 40
    errs = {"loss": abs(res["hip"][0] - res["torch"][0]) / abs(res["torch"][0])}
    for k, g in res["torch"][1].items():
        errs[k] = _err(res["hip"][1][k], g)
    _check(parity, errs)
