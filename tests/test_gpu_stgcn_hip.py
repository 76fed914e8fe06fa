"""The STGCN predictor on HIP (``STGCN(..., backend="hip")``, csrc/stgcn.hip, predictors/stgcn_hip.py) on the GPU.  The reference of every
comparison is the torch STGCN module (pinned to the reference implementation's vectors by tests/test_predictor_stgcn.py) in fp64 on the CPU; the
bound is the project's element-wise one, 1e-4 of the reference tensor's largest magnitude, for every output, dX and parameter gradient."""
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gptst_amd import _C, graph, ops, synth
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import STGCN, stgcn as S, stgcn_hip as H
from golden_util import load
from downstream_util import _check, _err
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rows(x):            # (B, C, T, N) -> (B*T*N, C)
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _gpu_copy(m64):
    import copy
    return copy.deepcopy(m64).float().to(DEV)


# ---- 1. temporal convolution -------------------------------------------------------------------------------------------------------------
TCONV = [(64, 32, 3, "GLU"), (32, 64, 3, "relu"), (32, 128, 3, "relu"), (128, 128, 3, "GLU"), (128, 128, 1, "sigmoid")]


def _cps(rows, cw, ktot):
    """64-row chunks one split of the weight gradient sums: ceil(ceil(rows / 64) / nsplit)"""
    ns = _C.lib().value("gptst_stgcn_wgrad_nsplit", rows, cw, ktot)
    nchunks = -(-rows // 64)
    return -(-nchunks // ns)


def _tconv_plan(ci, co, kt, act, rows):
    """what the launch plans of csrc/stgcn.hip make of a temporal convolution and its backward: tiles per wave of the forward and of the data
    backward (the plan queries of include/gptst_hip_testing.h), 64-row chunks per split of the weight gradient, float4s of the gate backward"""
    v = _C.lib().value
    cw, ktot = (2 * co if act == "GLU" else co), kt * ci + (ci if ci > co else 0)
    ntap = ktot // ci
    return SimpleNamespace(ktot=ktot, fwd=v("gptst_stgcn_tapgemm_tpw", rows, co, ktot, H._ACT[act]),
                           bwd=v("gptst_stgcn_tapgemm_tpw", rows, ci, ntap * cw, H.ACT_NONE), cps=_cps(rows, cw, ktot), n4=rows * co // 4)


@pytest.mark.parametrize("btn", [(2, 12, 20), (1, 3, 37)])
@pytest.mark.parametrize("ci,co,kt,act", TCONV)
def test_temporal_convolution(ci, co, kt, act, btn, parity):
    _tconv_case(ci, co, kt, act, btn, parity)


# Shapes at which a wave's loop over its row tiles, a split's loop over its 64-row chunks and the gate backward's grid-stride loop run more than
# once, as they do at every real batch (130 560 rows and more).  N = 461 is no multiple of 16; 16 596 rows are 1 038 tiles and 33 192 rows
# 2 075 tiles, against 1 024 waves: the tile count is no multiple of the wave count, so the last wave ends early and some get no tile.
#              ci   co  kt  act    (B, T, N)     tiles per wave: forward, data backward
TCONV_MULTI = [(128, 128, 3, "GLU", (3, 12, 461), 2, 2),
               (128, 128, 3, "GLU", (6, 12, 461), 3, 3),          # and 1 062 144 float4s in the gate backward: a second grid-stride pass
               (128, 64, 3, "GLU", (3, 12, 461), 2, 2)]           # Ktot = 512 > 384 (the align block joins K): the narrow kernel, forward too


@pytest.mark.parametrize("ci,co,kt,act,btn,fwd,bwd", TCONV_MULTI)
def test_temporal_convolution_multi_tile(ci, co, kt, act, btn, fwd, bwd, parity):
    plan = _tconv_plan(ci, co, kt, act, btn[0] * btn[1] * btn[2])
    assert (plan.fwd, plan.bwd) == (fwd, bwd) and plan.cps >= 2, vars(plan)
    assert (plan.ktot > 384) == (ci > co)
    if btn[0] == 6:
        assert plan.n4 > 4096 * 256, plan.n4
    _tconv_case(ci, co, kt, act, btn, parity)


def _tconv_case(ci, co, kt, act, btn, parity):
    B, T, N = btn
    torch.manual_seed(ci + co + kt + N)
    m64 = S._TConv(kt, ci, co, act).double()
    x64 = torch.randn(B, ci, T, N, dtype=torch.float64, requires_grad=True)
    w64 = torch.randn(B, co, T, N, dtype=torch.float64)
    y64 = m64(x64)
    (y64 * w64).sum().backward()
    m = _gpu_copy(m64)
    x = _rows(x64.detach()).float().to(DEV).requires_grad_(True)
    y = H._tconv(m, x, T, N)
    (y * _rows(w64).float().to(DEV)).sum().backward()
    errs = {"y": _err(y, _rows(y64)), "dx": _err(x.grad, _rows(x64.grad))}
    want = dict(m64.named_parameters())
    assert ("align.conv1x1.weight" in want) == (ci > co)
    for k, p in m.named_parameters():
        errs[k] = _err(p.grad, want[k].grad)
    _check(parity, errs)


def test_wgrad_three_chunks_per_split_and_a_short_last_split(parity):
    """ops.stgcn_wgrad alone, cw = 256 and Ktot = 384 (24 tiles, so at most 42 splits) over 5 424 rows = 85 chunks (the last one of 48 rows):
    29 splits of 3 chunks, the last split with ONE chunk.  dW and db against the fp64 sums with the taps' 'same' padding in T"""
    B, T, N, ci, cw, taps = 2, 12, 226, 128, 256, (-1, 0, 1)
    rows, ktot = B * T * N, 3 * ci
    ns = _C.lib().value("gptst_stgcn_wgrad_nsplit", rows, cw, ktot)
    nchunks, cps = -(-rows // 64), _cps(rows, cw, ktot)
    assert (nchunks, ns, cps) == (85, 29, 3) and nchunks - (ns - 1) * cps == 1
    g = torch.Generator().manual_seed(226)
    D, X = torch.randn(rows, cw, dtype=torch.float64, generator=g), torch.randn(rows, ci, dtype=torch.float64, generator=g)
    x4, want = X.view(B, T, N, ci), []
    for dt in taps:                                                                # X[b, t + dt, n] where that is inside [0, T), else 0
        sh = torch.zeros_like(x4)
        sh[:, max(0, -dt):T - max(0, dt)] = x4[:, max(0, dt):T - max(0, -dt)]
        want.append(D.t() @ sh.view(rows, ci))
    dW, db = ops.stgcn_wgrad(D.float().to(DEV), X.float().to(DEV), taps, T, N)
    _check(parity, {"dW": _err(dW, torch.cat(want, 1)), "db": _err(db, D.sum(0))})


# ---- 2. graph convolution ----------------------------------------------------------------------------------------------------------------
def _nodemix_lds(N):
    """bytes of dynamic LDS of the node-mix launch: 36 floats for each of the 16 ceil(N / 16) padded nodes (NODE_MIX_P of csrc/node_mix_dev.h)"""
    return 16 * ((N + 15) // 16) * 36 * 4


@pytest.mark.parametrize("N", [20, 37, 170, 461])
def test_graph_convolution(N, parity):
    """(N = 461: a slab of 66 816 bytes, beyond the 64 KB a launch gets without asking for more)"""
    assert (_nodemix_lds(N) > 64 * 1024) == (N == 461)
    B, T, c = 1, 2, 32
    torch.manual_seed(N)
    lk = torch.randn(3, N, N, dtype=torch.float64) / N ** 0.5            # non-symmetric: a transposed L_k in the backward shows
    m64 = S._SConv(3, c, c, lk).double()
    x64 = torch.randn(B, c, T, N, dtype=torch.float64, requires_grad=True)
    w64 = torch.randn(B, c, T, N, dtype=torch.float64)
    y64 = m64(x64)
    (y64 * w64).sum().backward()
    m = _gpu_copy(m64)
    x = _rows(x64.detach()).float().to(DEV).requires_grad_(True)
    y = H._sconv(m, x, T, N)
    (y * _rows(w64).float().to(DEV)).sum().backward()
    _check(parity, {"y": _err(y, _rows(y64)), "dx": _err(x.grad, _rows(x64.grad)), "theta": _err(m.theta.grad, m64.theta.grad),
                    "b": _err(m.b.grad, m64.b.grad)})


def test_nodemix_reduce_beyond_64_kb_of_lds(parity):
    """ops.stgcn_nodemix alone at N = 461: Y = sum_k L_k Z_k + R for three non-symmetric graphs, 48 channels (a whole 32-channel group and a half
    one) and two units, against fp64"""
    N, ks, c, units = 461, 3, 48, 2
    assert _nodemix_lds(N) == 66816 > 64 * 1024
    g = torch.Generator().manual_seed(461)
    L = torch.randn(ks, N, N, dtype=torch.float64, generator=g) / N ** 0.5
    Z, R = torch.randn(units * N, ks * c, dtype=torch.float64, generator=g), torch.randn(units * N, c, dtype=torch.float64, generator=g)
    want = torch.einsum("knm,umkc->unc", L, Z.view(units, N, ks, c)).reshape(units * N, c) + R
    Np = 16 * ((N + 15) // 16)
    Lp = torch.zeros(ks, Np, Np, dtype=torch.float64)
    Lp[:, :N, :N] = L
    got = ops.stgcn_nodemix(Lp.float().to(DEV), Z.float().to(DEV), N, c, reduce=True, res=R.float().to(DEV))
    _check(parity, {"y": _err(got, want)})


# ---- 3. LayerNorm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C", [(20, 64), (37, 128), (170, 128)])
def test_layernorm(N, C, parity):
    _layernorm_case(N, C, 3, parity)


def test_layernorm_several_units_per_split(parity):
    """40 units against at most 16 splits: 14 splits of 3 units, the last one with a single unit (3 units, as above, are one unit per split)"""
    ns = _C.lib().value("gptst_stgcn_ln_nsplit", 40)
    ups = -(-40 // ns)
    assert ups >= 2 and 40 - (ns - 1) * ups == 1, (ns, ups)
    _layernorm_case(20, 64, 40, parity)


def _layernorm_case(N, C, units, parity):
    torch.manual_seed(N + C)
    ln64 = torch.nn.LayerNorm([N, C]).double()
    with torch.no_grad():
        ln64.weight.copy_(1 + 0.5 * torch.randn(N, C, dtype=torch.float64))
        ln64.bias.copy_(0.5 * torch.randn(N, C, dtype=torch.float64))
    x64 = (10 + torch.randn(units, N, C, dtype=torch.float64)).requires_grad_(True)
    w64 = torch.randn(units, N, C, dtype=torch.float64)
    y64 = ln64(x64)
    (y64 * w64).sum().backward()
    ln = _gpu_copy(ln64)
    x = x64.detach().float().to(DEV).view(units * N, C).requires_grad_(True)
    y = H._ln(ln, x, units)
    (y * w64.float().to(DEV).view(units * N, C)).sum().backward()
    _check(parity, {"y": _err(y, y64.view(-1, C)), "dx": _err(x.grad, x64.grad.view(-1, C)), "gamma": _err(ln.weight.grad, ln64.weight.grad),
                    "beta": _err(ln.bias.grad, ln64.bias.grad)})


# ---- 4./5. the whole model ---------------------------------------------------------------------------------------------------------------
def _ap(N, lk=None, blocks1=(64, 32, 128), drop_prob=0):
    lk = graph.stgcn_graph(graph.synthetic_adjacency(N, 2)) if lk is None else lk
    return SimpleNamespace(Ks=3, Kt=3, num_nodes=N, G=lk, blocks1=list(blocks1), drop_prob=drop_prob, outputl_ks=3)


def test_whole_model_against_the_reference_vectors(parity):
    G = load("stgcn_small.npz")
    ap = _ap(G["A"].shape[0], graph.stgcn_graph(G["A"]))
    m = STGCN(ap, DEV, 64, 1, backend="hip").to(DEV)
    m.load_state_dict({k[3:]: torch.tensor(G[k]) for k in G.files if k.startswith("sd.")}, strict=True)
    m.train()
    x = torch.tensor(G["x"], device=DEV, requires_grad=True)
    y = m(x)
    assert m.backend_used == "hip" and y.shape == (2, 12, 20, 1)
    (y * torch.tensor(G["w"], device=DEV)).sum().backward()
    errs = {"y": _err(y, torch.tensor(G["y"])), "dx": _err(x.grad, torch.tensor(G["dx"]))}
    for k, p in m.named_parameters():
        errs[k] = _err(p.grad, torch.tensor(G["grad." + k]))
    _check(parity, errs)


def _model_pair(B, T, N, dim_out, seed, ap=None):
    """the torch module in fp64 on the CPU (default init, LayerNorm parameters perturbed), its HIP twin, and a batch with its fp64 results"""
    torch.manual_seed(seed)
    ap = _ap(N) if ap is None else ap
    m64 = STGCN(ap, "cpu", 64, dim_out).double()
    with torch.no_grad():
        for k, p in m64.named_parameters():
            if ".ln." in k:
                p.add_(0.3 * torch.randn_like(p))
    x64 = torch.randn(B, T, N, 64, dtype=torch.float64, requires_grad=True)
    w64 = torch.randn(B, T, N, dim_out, dtype=torch.float64)
    y64 = m64(x64)
    (y64 * w64).sum().backward()
    m = STGCN(ap, DEV, 64, dim_out, backend="hip").to(DEV)
    m.load_state_dict({k: v.float() for k, v in m64.state_dict().items()}, strict=True)
    return m64, x64, w64, y64, m


@pytest.mark.parametrize("B,T,N,dim_out", [(3, 12, 37, 2), (1, 12, 170, 1), (2, 3, 16, 1)])
def test_whole_model_against_fp64_torch(B, T, N, dim_out, parity):
    _whole_model(_model_pair(B, T, N, dim_out, 5 + N), parity)


@pytest.mark.parametrize("ds", ["METR_LA", "NYC_BIKE", "NYC_TAXI"])
def test_shipped_stgcn_configuration_against_fp64_torch(ds, parity):
    """the predictor as ``-mode eval -model STGCN`` builds it from conf/STGCN/<dataset>.conf (207, 250 and 266 nodes; the output width is the
    dataset's) over a synthetic graph, one batch element of the 64-wide embedding"""
    pa = predictor_args(ds, "STGCN")
    N, dim_out = pa.num_nodes, make_args(ds).output_dim
    assert (N, dim_out) == {"METR_LA": (207, 1), "NYC_BIKE": (250, 2), "NYC_TAXI": (266, 2)}[ds]
    ap = SimpleNamespace(Ks=pa.Ks, Kt=pa.Kt, num_nodes=N, G=graph.stgcn_graph(graph.synthetic_adjacency(N, 2)), blocks1=list(pa.blocks1),
                         drop_prob=pa.drop_prob, outputl_ks=pa.outputl_ks)
    _whole_model(_model_pair(1, pa.input_window, N, dim_out, 5 + N, ap), parity)


def _whole_model(pair, parity):
    m64, x64, w64, y64, m = pair
    m.train()
    x = x64.detach().float().to(DEV).requires_grad_(True)
    y = m(x)
    assert m.backend_used == "hip"
    (y * w64.float().to(DEV)).sum().backward()
    errs = {"y": _err(y, y64), "dx": _err(x.grad, x64.grad)}
    want = dict(m64.named_parameters())
    for k, p in m.named_parameters():
        errs[k] = _err(p.grad, want[k].grad)
    _check(parity, errs)


# ---- 6. repeatability and modes ----------------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    """record what every launch wrapper of the backend is asked to keep or returns for a backward"""
    from gptst_amd import ops
    seen = {"keep": [], "ln_stats": [], "wgrad": 0}
    tap, ln, wg = ops.stgcn_tapgemm, ops.stgcn_ln_fwd, ops.stgcn_wgrad

    def tapgemm(*a, **kw):
        seen["keep"].append(bool(kw.get("keep", False)))
        return tap(*a, **kw)

    def ln_fwd(*a, **kw):
        out = ln(*a, **kw)
        seen["ln_stats"].append(out[1] is not None or out[2] is not None)
        return out

    def wgrad(*a, **kw):
        seen["wgrad"] += 1
        return wg(*a, **kw)
    monkeypatch.setattr(ops, "stgcn_tapgemm", tapgemm)
    monkeypatch.setattr(ops, "stgcn_ln_fwd", ln_fwd)
    monkeypatch.setattr(ops, "stgcn_wgrad", wgrad)
    return seen


def test_repeatable_and_mode_independent(monkeypatch):
    torch.manual_seed(3)
    m = STGCN(_ap(37), DEV, 64, 1, backend="hip").to(DEV)
    x = torch.randn(2, 12, 37, 64, device=DEV)
    w = torch.randn(2, 12, 37, 1, device=DEV)
    seen = _spy(monkeypatch)

    def grads():
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        (y * w).sum().backward()
        return y.detach(), [xi.grad] + [p.grad.clone() for p in m.parameters()]
    m.train()
    y1, g1 = grads()
    # training: the three GLU launches keep sigmoid(Q) and P + res, the three LayerNorms their statistics; one weight-gradient launch for each of the 6 temporal and 2 graph convolutions
    assert sum(seen["keep"]) == 3 and seen["ln_stats"] == [True] * 3 and seen["wgrad"] == 8, seen
    y2, g2 = grads()
    assert m.backend_used == "hip" and torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    # no_grad, and eval mode with gradients enabled: the same output, and no launch writes or keeps anything for a backward
    for mode in ("no_grad", "eval"):
        seen["keep"].clear(), seen["ln_stats"].clear()
        if mode == "no_grad":
            with torch.no_grad():
                y3 = m(x)
        else:
            m.eval()
            y3 = m(x.clone().requires_grad_(True))
        assert torch.equal(y3, y1) and m.backend_used == "hip" and not y3.requires_grad and y3.grad_fn is None
        assert len(seen["keep"]) == 8 and not any(seen["keep"]) and seen["ln_stats"] == [False] * 3, (mode, seen)


def test_frozen_predictor_skips_the_weight_gradients(monkeypatch):
    """parameters that take no gradient: the input's gradient is the same, bit for bit, and no weight-gradient kernel is launched"""
    torch.manual_seed(3)
    m = STGCN(_ap(20), DEV, 64, 1, backend="hip").to(DEV).train()
    x = torch.randn(2, 12, 20, 64, device=DEV)
    w = torch.randn(2, 12, 20, 1, device=DEV)

    def dx():
        xi = x.clone().requires_grad_(True)
        (m(xi) * w).sum().backward()
        return xi.grad
    want = dx()
    for p in m.parameters():
        p.requires_grad_(False)
    seen = _spy(monkeypatch)
    got = dx()
    assert m.backend_used == "hip" and seen["wgrad"] == 0 and torch.equal(got, want)


# ---- 7. fallback -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(drop_prob=0.1), dict(blocks1=(64, 24, 128))])
def test_fallback_takes_the_torch_modules(kw):
    """active dropout, or a width the kernels do not serve: the forward is the torch backend's, bit for bit.  The convolution library's default
    algorithms are not bit-repeatable on this GPU (the torch backend differs from ITSELF by one ulp from run to run, 8.9e-8 at |y| <= 0.26), so both
    modules run with its deterministic algorithms selected; the setting is put back."""
    torch.manual_seed(4)
    ap = _ap(20, **kw)
    mh, mt = STGCN(ap, DEV, 64, 1, backend="hip").to(DEV), STGCN(ap, DEV, 64, 1).to(DEV)
    mt.load_state_dict(mh.state_dict(), strict=True)
    x = torch.randn(2, 12, 20, 64, device=DEV)
    mh.train(), mt.train()
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(9)
        yh = mh(x)
        torch.manual_seed(9)
        yt = mt(x)
    finally:
        torch.backends.cudnn.deterministic = was
    assert mh.backend_used == "torch" and mt.backend_used == "torch"
    assert torch.equal(yh, yt), float((yh - yt).abs().max())
    if "drop_prob" in kw:                                 # eval mode: dropout is inactive and the kernels serve the call
        mh.eval()
        mh(x)
        assert mh.backend_used == "hip"


# ---- 8. the chain ------------------------------------------------------------------------------------------------------------------------
def _front_end(tmp_path, backend, finetune, sd):
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    N = 20
    args = make_args("PEMS08", mode="eval", num_nodes=N, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros(), batch_size=8, epochs=3,
                     early_stop=False, log_dir=str(tmp_path), debug=True, model="STGCN_test", stgcn_backend=backend)
    sd = O.init_state_dict(args, 4) if sd is None else sd
    torch.manual_seed(0)
    model = EnhanceFrontEnd(args, predictor=STGCN(_ap(N), DEV, args.hidden_dim, args.output_dim, backend=args.stgcn_backend),
                            finetune_encoder=finetune).to(DEV)
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
        loss = tr._loss(model(src, tgt)[0], tgt)
        loss.backward()
        assert model.predictor.backend_used == name
        res[name] = (float(loss), {k: p.grad for k, p in model.named_parameters() if p.requires_grad})
    assert set(res["hip"][1]) == set(res["torch"][1])
    assert any(k.startswith("pretrain_model.") for k in res["hip"][1]) == finetune
    errs = {"loss": abs(res["hip"][0] - res["torch"][0]) / abs(res["torch"][0])}
    for k, g in res["torch"][1].items():
        errs[k] = _err(res["hip"][1][k], g)
    _check(parity, errs)


def test_eval_trainer_learns_on_the_hip_backend(tmp_path):
    from gptst_amd import data as gdata
    args, sd, model, ET = _front_end(tmp_path, "hip", False, None)
    raw = synth.make_series(20, 3, days=6, seed=3)
    train, val, test, scaler, _, _ = gdata.get_dataloader(args, device=DEV, raw=raw, generator=torch.Generator().manual_seed(1))
    tr = ET(model, args, train, val, test, float(scaler.mean), float(scaler.std))
    tr.logger.setLevel(logging.WARNING)
    losses = [tr.train_epoch(e) for e in (1, 2, 3)]
    assert model.predictor.backend_used == "hip"
    assert losses[2] < losses[0] and all(np.isfinite(losses)), losses
    rows = tr.test(test)
    assert model.predictor.backend_used == "hip"
    assert rows.shape == (13, 4) and bool(torch.isfinite(rows[:, :3]).all())
