"""The ST-MGCN predictor on HIP (``STMGCN(..., backend="hip")``, csrc/stmgcn.hip, predictors/stmgcn_hip.py) on the GPU.  The reference of
every comparison is the explicit per-step formula of stmgcn_util (held to ``nn.LSTM`` autograd at 1e-12 by tests/test_stmgcn_hip_cpu.py) or
the torch STMGCN module (pinned to the reference implementation's vectors by tests/test_predictor_stmgcn.py), in fp64 on the CPU; the bound
is the project's element-wise one, 1e-4 of the reference tensor's largest magnitude (downstream_util.TOL), for every output, dX and
parameter gradient.  fp32 ``nn.LSTM`` itself stays within 5e-7 of fp64 on the launch inputs, and exchanging any two gates moves the
output by more than 1e-2 (test_stmgcn_hip_cpu.py asserts that for every input used here): the bound sits between the two.

Launch shapes (rows, T, L, H): (40, 2, 1, 64) a half-filled last tile; (111, 12, 3, 64) the shipped depth, a workgroup with a missing tile
when two are forced; (16, 1, 2, 16) T = 1 and K below one 64-wide k-block, three waves idle; (48, 3, 3, 48) three channel tiles;
(33, 2, 2, 128) two channel tiles a wave, K = 512 backward; (64, 32, 1, 32) the step bound; (32, 2, 4, 64) the layer bound.  Each with one
and two row tiles forced; every launch writes into sentinel-filled buffers, runs twice and must repeat bit for bit."""
import logging

import pytest
import torch

import stmgcn_util as gu
from gptst_amd import _C, graph, ops, synth
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import STMGCN, stmgcn_hip as SH
from golden_util import load
from downstream_util import _check, _err
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0


def _g(t):
    return t.float().to(DEV).contiguous()


def _sent(*shape):
    return torch.full(shape, SENT, device=DEV, dtype=torch.float32)


# ---- 1. the LDS plan and the tile rule ------------------------------------------------------------------------------------------------------
def test_lds_plan_and_tile_rule_are_pinned():
    # backward: 16 tiles (2 L H + 5 H + 4) floats — the dh and dc carries, layer l + 1's dx, dG at pitch 4H + 4; forward 16 tiles L (3 H + 4)
    assert ops.stmgcn_lds_bytes(64, 3, 2) == 32 * (2 * 3 * 64 + 5 * 64 + 4) * 4 == 90624 > 64 * 1024          # the shipped shape: above the default
    assert ops.stmgcn_lds_bytes(64, 3, 1) == 45312
    assert ops.stmgcn_lds_bytes(128, 4, 1) == 16 * (2 * 4 * 128 + 5 * 128 + 4) * 4 == 106752 <= SH.LDS_MAX     # the largest served shape
    assert ops.stmgcn_lds_bytes(128, 4, 2) == 213504 > SH.LDS_MAX and ops.stmgcn_lds_bytes(128, 2, 2) == 147968 <= SH.LDS_MAX
    assert ops.stmgcn_tiles(64 * 266, 64, 3) == 2 and ops.stmgcn_tiles(64 * 266, 128, 4) == 1                 # (two tiles would not fit)
    assert ops.stmgcn_tiles(16 * 512, 64, 3) == 1 and ops.stmgcn_tiles(16 * 512 + 1, 64, 3) == 2              # more workgroups than CUs first
    assert ops.stmgcn_tiles(100, 144, 3) < 0 and ops.stmgcn_tiles(100, 64, 5) < 0 and ops.stmgcn_tiles(100, 8, 1) < 0


# ---- 2. the two launches, each alone, against their formulas ----------------------------------------------------------------------------------
def _flat(ws):
    return torch.cat([w.reshape(-1) for w in ws])


def _launch_fwd(Gx0, W, bias, rows, T, L, H, keep, tiles):
    """the raw entry on sentinel-filled outputs, twice -> (top, gates, c, h) of the first run (None where not written)"""
    runs = []
    for _ in range(2):
        top = gates = c = h = None
        if keep:
            gates, c, h = _sent(L, T, rows, 4 * H), _sent(L, T, rows, H), _sent(L, T + 1, rows, H)
            h[:, 0] = 0
        else:
            top = _sent(T, rows, H)
        _C.lib().call("gptst_stmgcn_lstm_fwd", _C.ptr(Gx0), _C.ptr(W), _C.ptr(bias), _C.ptr(top), _C.ptr(gates), _C.ptr(c), _C.ptr(h), rows, T, L, H,
                      tiles, _C.stream())
        runs.append((top, gates, c, h))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert (a is None and b is None) or torch.equal(a, b)
    return runs[0]


def _launch_bwd(dTop, WT, gates, c, nl, rows, T, L, H, tiles):
    runs = []
    for _ in range(2):
        dG = _sent(nl, T, rows, 4 * H)
        _C.lib().call("gptst_stmgcn_lstm_bwd", _C.ptr(dTop), _C.ptr(WT), _C.ptr(gates), _C.ptr(c), _C.ptr(dG), nl, rows, T, L, H, tiles, _C.stream())
        runs.append(dG)
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1])
    return runs[0]


@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("rows,T,L,H", gu.LAUNCH_CASES)
def test_lstm_fwd_launch(rows, T, L, H, tiles, parity):
    assert ops.stmgcn_lds_bytes(H, L, tiles) <= SH.LDS_MAX
    Gx0, W, b, _ = gu.launch_inputs(rows, T, L, H)
    top, gates, cs, hs = gu.lstm_fwd(Gx0, W, b)
    gx, gw, gb = _g(Gx0), _g(_flat(W)), _g(torch.stack(b))
    _, kg, kc, kh = _launch_fwd(gx, gw, gb, rows, T, L, H, True, tiles)
    assert not bool(kh[:, 0].any())
    errs = {"gates": _err(kg, gates), "c": _err(kc, cs), "h": _err(kh, hs), "top": _err(kh[L - 1, 1:], top)}
    for l in range(L):
        errs["h.l%d.last" % l] = _err(kh[l, T], hs[l, T])
    t_only = _launch_fwd(gx, gw, gb, rows, T, L, H, False, tiles)[0]
    assert torch.equal(t_only, kh[L - 1, 1:])                              # keep = False: the same values, the top ring alone
    rule = ops.stmgcn_tiles(rows, H, L)
    if tiles == rule:                                                      # tiles = 0 is the count the rule names, bit for bit
        assert torch.equal(_launch_fwd(gx, gw, gb, rows, T, L, H, False, 0)[0], t_only)
    _check(parity, errs)


@pytest.mark.parametrize("last_only", [False, True])
@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("rows,T,L,H", gu.LAUNCH_CASES)
def test_lstm_bwd_launch(rows, T, L, H, tiles, last_only, parity):
    Gx0, W, b, dTop = gu.launch_inputs(rows, T, L, H, last_only=last_only)
    _, gates, cs, _ = gu.lstm_fwd(Gx0, W, b)
    gates, cs = gates.float().double(), cs.float().double()                # what the launch reads: the fp32 values
    dG = gu.lstm_bwd(dTop, W, gates, cs)
    gd, gwt, gg, gc = _g(dTop), _g(_flat([w.t().contiguous() for w in W])), _g(gates), _g(cs)
    got = _launch_bwd(gd, gwt, gg, gc, L, rows, T, L, H, tiles)
    errs = {"dG.l%d" % l: _err(got[l], dG[l]) for l in range(L)}
    errs["dGx0.first_step"] = _err(got[0, 0], dG[0, 0])                    # the end of the whole chain
    assert torch.equal(_launch_bwd(gd, gwt, gg, gc, 1, rows, T, L, H, tiles)[0], got[0])      # layer 0's alone: the same values
    if tiles == ops.stmgcn_tiles(rows, H, L):
        assert torch.equal(_launch_bwd(gd, gwt, gg, gc, L, rows, T, L, H, 0), got)
    _check(parity, errs)


def test_launches_refuse_what_they_do_not_serve():
    x = _sent(4)
    p, s = _C.ptr(x), _C.stream()
    v = _C.lib().value
    assert v("gptst_stmgcn_lstm_fwd", p, p, p, p, None, None, None, 16, 33, 1, 16, 0, s) == _C.ESHAPE       # T above 32
    assert v("gptst_stmgcn_lstm_fwd", p, p, p, p, None, None, None, 16, 1, 5, 16, 0, s) == _C.ESHAPE        # five layers
    assert v("gptst_stmgcn_lstm_fwd", p, p, p, p, None, None, None, 16, 1, 1, 24, 0, s) == _C.ESHAPE        # a width that is no multiple of 16
    assert v("gptst_stmgcn_lstm_fwd", p, p, p, p, None, None, None, 16, 1, 4, 128, 2, s) == _C.ESHAPE       # two tiles forced beyond the LDS
    assert v("gptst_stmgcn_lstm_fwd", p, p, p, p, p, p, p, 16, 1, 1, 16, 0, s) == -1                        # top and the kept set together
    assert v("gptst_stmgcn_lstm_bwd", p, p, p, p, p, 2, 16, 1, 1, 16, 0, s) == -1                           # more dG layers than layers
    torch.cuda.synchronize()
    assert bool((x == SENT).all())


# ---- 3. whole models ------------------------------------------------------------------------------------------------------------------------
def _ap(N, **kw):
    dis, pcc = gu.graphs(N)
    return gu.model_args(N, graph.stmgcn_supports(dis), graph.stmgcn_supports(pcc), **kw)


def _run(m, x, w):
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    y = m(xi)
    (y * w).sum().backward()
    return y.detach(), xi.grad, {k: p.grad for k, p in m.named_parameters()}


def _pair(ap, C, out, seed, B):
    """the module on the GPU with the HIP backend, its fp64 twin on the CPU with the torch ops, a batch and a loss weight"""
    torch.manual_seed(seed)
    mh = gu.perturb_(STMGCN(ap, "cpu", C, out, backend="hip")).to(DEV).train()
    mt = STMGCN(ap, "cpu", C, out).double().train()
    mt.load_state_dict({k: v.detach().cpu().double() for k, v in mh.state_dict().items()}, strict=True)
    return mh, mt, torch.randn(B, ap.seq_len, ap.n_nodes, C), torch.randn(B, ap.seq_len, ap.n_nodes, out)


def _errs(got, ref, T):
    errs = {"y": _err(got[0], ref[0]), "dx": _err(got[1], ref[1])}
    assert set(got[2]) == set(ref[2])
    for k, g in ref[2].items():
        assert float(g.abs().max()) > 0, k                                 # the comparison is not made where everything is zero
        errs[k] = _err(got[2][k], g)
        if "bias_ih" in k:
            assert torch.equal(got[2][k], got[2][k.replace("bias_ih", "bias_hh")]), k
    return errs


def _compare(mh, mt, x, w, parity):
    got = _run(mh, x.to(DEV), w.to(DEV))
    assert mh.backend_used == "hip"
    ref = _run(mt, x.double(), w.double())
    errs = _errs(got, ref, x.shape[1])
    assert len(errs) == 2 + 2 * (4 + 4 * mh.lstm_num_layers) + 6
    _check(parity, errs)


# (the seeds: ones at which no reference gradient is exactly zero — at T = 5 the five hidden units of a branch's gate can all be dead, seed 42 is such a draw)
@pytest.mark.parametrize("B,T,N,C,out,H,L,seed", [(2, 12, 20, 64, 2, 64, 3, 32), (3, 5, 37, 16, 1, 32, 2, 1)])
def test_whole_model_against_fp64_torch(B, T, N, C, out, H, L, seed, parity):
    mh, mt, x, w = _pair(_ap(N, T=T, H=H, L=L), C, out, seed, B)
    _compare(mh, mt, x, w, parity)


@pytest.mark.parametrize("ds,C", [("NYC_TAXI", 64), ("NYC_BIKE", 128)])
def test_shipped_configuration_against_fp64_torch(ds, C, parity):
    pa = predictor_args(ds, "STMGCN")
    dis, pcc = gu.graphs(pa.n_nodes, seed=5)
    ap = gu.model_args(pa.n_nodes, graph.stmgcn_supports(dis), graph.stmgcn_supports(pcc), T=pa.seq_len, H=pa.lstm_hidden_dim,
                       L=pa.lstm_num_layers, G=pa.gcn_hidden_dim, bias=pa.gconv_use_bias)
    mh, mt, x, w = _pair(ap, C, 2, 9, 1)
    assert SH.supported(mh, x.to(DEV))
    _compare(mh, mt, x, w, parity)


def test_whole_model_against_the_reference_vectors(parity):
    G = load("stmgcn_small.npz")
    m = STMGCN(gu.model_args(20, torch.tensor(G["sup.dis"]), torch.tensor(G["sup.pcc"])), "cpu", 64, 2, backend="hip")
    m.load_state_dict({k[3:]: torch.tensor(G[k]) for k in G.files if k.startswith("sd.")}, strict=True)
    m = m.to(DEV).train()
    got = _run(m, torch.tensor(G["x"]).float().to(DEV), torch.tensor(G["w"]).float().to(DEV))
    assert m.backend_used == "hip"
    ref = (torch.tensor(G["y"]), torch.tensor(G["dx"]), {k[5:]: torch.tensor(G[k]) for k in G.files if k.startswith("grad.")})
    errs = _errs(got, ref, 12)
    assert len(errs) == 40
    _check(parity, errs)


# ---- 4. the launch count, repeatability, the modes --------------------------------------------------------------------------------------------
FAMILY = ["stmgcn_lstm_fwd", "stmgcn_lstm_bwd"]
HOISTED = ["stgcn_tapgemm", "stgcn_wgrad"]


def _spy(monkeypatch):
    seen = {"calls": [], "kept": [], "dG_layers": []}

    def wrap(name):
        fn = getattr(ops, name)

        def f(*a, **kw):
            seen["calls"].append(name)
            out = fn(*a, **kw)
            if name == "stmgcn_lstm_fwd":
                seen["kept"].append(sum(t.numel() * 4 for t in out[1:] if t is not None))
            if name == "stmgcn_lstm_bwd":
                seen["dG_layers"].append(out.shape[0])
            return out
        monkeypatch.setattr(ops, name, f)
    for n in FAMILY + HOISTED:
        wrap(n)
    return seen


def test_launch_count_repeatability_and_modes(monkeypatch):
    B, T, N, C, H, L = 2, 6, 37, 32, 48, 3
    torch.manual_seed(3)
    m = gu.perturb_(STMGCN(_ap(N, T=T, H=H, L=L), "cpu", C, 2, backend="hip")).to(DEV)
    x, w = torch.randn(B, T, N, C, device=DEV), torch.randn(B, T, N, 2, device=DEV)
    seen = _spy(monkeypatch)
    m.train()
    y1, dx1, g1 = _run(m, x, w)
    # one training step: ONE forward launch per branch, ONE backward launch per branch; around them the input GEMM of both branches, its data
    # and weight gradient, and per branch 2 L - 1 weight gradients
    assert m.backend_used == "hip" and seen["calls"].count("stmgcn_lstm_fwd") == 2 and seen["calls"].count("stmgcn_lstm_bwd") == 2
    assert seen["calls"][:3] == ["stgcn_tapgemm", "stmgcn_lstm_fwd", "stmgcn_lstm_fwd"]
    assert seen["calls"].count("stgcn_wgrad") == 2 * (2 * L - 1) + 1 and seen["calls"].count("stgcn_tapgemm") == 2
    rows = B * N
    assert seen["kept"] == [4 * (L * T * rows * 5 * H + L * (T + 1) * rows * H)] * 2 and seen["dG_layers"] == [L, L]
    # a second step on the same batch: bit for bit
    y2, dx2, g2 = _run(m, x, w)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    # no_grad, and eval mode with gradients enabled: the same forward launch, the same output, nothing kept
    for mode in ("no_grad", "eval"):
        seen["calls"].clear(), seen["kept"].clear()
        if mode == "no_grad":
            with torch.no_grad():
                y3 = m(x)
        else:
            m.eval()
            y3 = m(x.clone().requires_grad_(True))
        assert torch.equal(y3, y1) and m.backend_used == "hip" and not y3.requires_grad and y3.grad_fn is None
        assert seen["calls"] == ["stgcn_tapgemm", "stmgcn_lstm_fwd", "stmgcn_lstm_fwd"] and seen["kept"] == [0, 0], (mode, seen)


def test_frozen_lstm_skips_the_weight_gradients(monkeypatch):
    torch.manual_seed(3)
    m = gu.perturb_(STMGCN(_ap(20, T=4), "cpu", 64, 2, backend="hip")).to(DEV).train()
    x, w = torch.randn(2, 4, 20, 64, device=DEV), torch.randn(2, 4, 20, 2, device=DEV)
    want = _run(m, x, w)[1]
    for r in m.rnn_list:
        for p in r.lstm.parameters():
            p.requires_grad_(False)
    seen = _spy(monkeypatch)
    xi = x.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    (m(xi) * w).sum().backward()
    assert m.backend_used == "hip" and "stgcn_wgrad" not in seen["calls"] and seen["dG_layers"] == [1, 1] and torch.equal(xi.grad, want)
    assert m.rnn_list[0].lstm.weight_hh_l0.grad is None and m.rnn_list[0].fc.weight.grad is not None


def test_state_dict_loads_strictly_both_ways_and_a_training_step_repeats():
    ap = _ap(20, T=4)
    torch.manual_seed(5)
    mh = gu.perturb_(STMGCN(ap, "cpu", 64, 2, backend="hip")).to(DEV).train()
    mt = STMGCN(ap, "cpu", 64, 2).to(DEV).train()
    mt.load_state_dict(mh.state_dict(), strict=True)
    mh.load_state_dict(mt.state_dict(), strict=True)
    assert list(mh.state_dict()) == list(mt.state_dict()) and len(mh.state_dict()) == 38
    x, w = torch.randn(2, 4, 20, 64, device=DEV), torch.randn(2, 4, 20, 2, device=DEV)
    sd0 = {k: v.clone() for k, v in mh.state_dict().items()}
    after = []
    for _ in range(2):                                                     # the same Adam step from the same state, twice
        mh.load_state_dict(sd0, strict=True)
        opt = torch.optim.Adam(mh.parameters(), lr=1e-3)
        _run(mh, x, w)
        opt.step()
        after.append({k: v.clone() for k, v in mh.state_dict().items()})
    assert mh.backend_used == "hip" and all(torch.equal(after[0][k], after[1][k]) for k in sd0)
    assert any(not torch.equal(after[0][k], sd0[k]) for k in sd0)


@pytest.mark.parametrize("kw,C", [(dict(L=5), 16), (dict(T=33), 16), (dict(), 24)])
def test_the_first_refused_shapes_take_the_torch_path(kw, C):
    torch.manual_seed(4)
    ap = _ap(20, **{"T": 3, "H": 16, **kw})
    mh = gu.perturb_(STMGCN(ap, "cpu", C, 1, backend="hip")).to(DEV)
    mt = STMGCN(ap, "cpu", C, 1).to(DEV)
    mt.load_state_dict(mh.state_dict(), strict=True)
    x = torch.randn(2, ap.seq_len, 20, C, device=DEV)
    assert not SH.supported(mh, x)
    yh, yt = mh(x), mt(x)
    assert mh.backend_used == "torch" and mt.backend_used == "torch" and torch.equal(yh, yt)


# ---- 5. the chain ---------------------------------------------------------------------------------------------------------------------------
def _front_end(tmp_path, backend, sd):
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    N = 20
    args = make_args("PEMS08", mode="eval", num_nodes=N, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros(), batch_size=8, epochs=3,
                     early_stop=False, log_dir=str(tmp_path), debug=True, model="STMGCN_test", stmgcn_backend=backend)
    sd = O.init_state_dict(args, 4) if sd is None else sd
    torch.manual_seed(0)
    pred = gu.perturb_(STMGCN(_ap(N), "cpu", args.hidden_dim, args.output_dim, backend=args.stmgcn_backend))
    model = EnhanceFrontEnd(args, predictor=pred, finetune_encoder=False).to(DEV)
    model.load_pretrained_model(sd)
    return args, sd, model, EvalTrainer


def test_chain_one_step_agrees_with_the_torch_backend(tmp_path, parity):
    args, sd, mh, ET = _front_end(tmp_path, "hip", None)
    _, _, mt, _ = _front_end(tmp_path, "torch", sd)
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
        res[name] = (float(loss.detach()), {k: p.grad for k, p in model.named_parameters() if p.requires_grad and p.grad is not None})
    assert set(res["hip"][1]) == set(res["torch"][1]) and sum(k.startswith("predictor.") for k in res["hip"][1]) == 38
    errs = {"loss": abs(res["hip"][0] - res["torch"][0]) / abs(res["torch"][0])}
    for k, g in res["torch"][1].items():
        errs[k] = _err(res["hip"][1][k], g)
    _check(parity, errs)
