"""The STSGCN predictor on HIP (``STSGCN(..., backend="hip")``, csrc/stsgcn.hip, predictors/stsgcn_hip.py) on the GPU.  The reference of every
comparison is fp64 torch on the CPU — the definition of a launch (tests/stsgcn_util.py, checked against the module by test_stsgcn_hip_cpu.py),
or the torch STSGCN module (pinned to the reference implementation's vectors by tests/test_predictor_stsgcn.py); the bound is the project's
element-wise one, 1e-4 of the reference tensor's largest magnitude, for every output, dX and parameter gradient.

The max and near-ties: where two candidates of the max nearly tie, fp32 and fp64 can pick different winners — the value barely moves, the
gradient is routed elsewhere.  That is a condition on the INPUT, checked on the fp64 reference alone: an element is ambiguous if its top-two gap
is below su.GAP = 1e-5 of the largest candidate magnitude, ten times the largest launch error recorded for like kernels (< 1e-6,
profiles/parity_astgcn_shipped_sizes.json; the candidate error this file measures is recorded as ``cand``).  Gradient comparisons of whole
models use shapes and seeds for which the test asserts ZERO ambiguous elements; the full confs are compared on the forward only."""
import copy
import logging
from types import SimpleNamespace

import pytest
import torch

import stsgcn_util as su
from gptst_amd import _C, ops, synth
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import STSGCN, stsgcn_hip as H, rows_hip
from downstream_util import _check, _err
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pad(A):
    n = A.shape[0]
    lp = A.new_zeros(rows_hip.pad16(n), rows_hip.pad16(n))
    lp[:n, :n] = A
    return lp.float().contiguous().to(DEV)


def _dev(t, *shape):
    return t.float().reshape(*shape).contiguous().to(DEV)


# ---- 1. the launches against their definitions ---------------------------------------------------------------------------------------------
#        B  W   N    c
MIX = [(3, 3, 20, 64),            # a padded tile; a frame fed by one, two and three blocks
       (1, 1, 16, 16),            # no padding, one window, half a channel group
       (3, 2, 37, 48),            # a second channel group half filled
       (1, 10, 20, 32),           # the conf's window count
       (3, 10, 37, 128),
       (1, 2, 170, 64), (1, 1, 266, 64),          # shipped node counts: 11 and 17 node tiles (the last workgroup has waves without a tile)
       (1, 1, 320, 128),
       (1, 2, 305, 16),           # 20 node tiles, the last with ONE real node
       (1, 1, 448, 16)]           # the largest node count served: 63 KB of LDS


@pytest.mark.parametrize("B,W,N,c", MIX)
def test_mix_every_form(B, W, N, c, parity):
    """a non-symmetric A^: a transposed operand fails; the adjoint forms are called with A^T as the predictor calls them"""
    T = W + 2
    g = torch.Generator().manual_seed(N + c + W)
    A = torch.randn(N, N, generator=g, dtype=torch.float64) / N ** 0.5
    Hf = torch.randn(B, T, N, c, generator=g, dtype=torch.float64)
    E = torch.randn(B, W, 3, N, c, generator=g, dtype=torch.float64)
    M = torch.randn(B, W, N, c, generator=g, dtype=torch.float64)
    assert float((A - A.t()).abs().max()) > 1e-2
    want = {"f2e": su.mix_f2e(A, Hf), "e2e": su.mix_expanded(A, E), "e2m": su.mix_middle(A, E),
            "e2e_adj": su.mix_expanded(A.t(), E), "m2e": su.mix_m2e(A.t(), M), "e2f": su.mix_e2f(A.t(), E)}
    lp, lpt = _pad(A), _pad(A.t())
    Hd, Ed, Md = _dev(Hf, B * T * N, c), _dev(E, B * W * 3 * N, c), _dev(M, B * W * N, c)
    got = {"f2e": ops.stsgcn_mix(lp, Hd, ops.MIX_F2E, B, T, N), "e2e": ops.stsgcn_mix(lp, Ed, ops.MIX_E2E, B, T, N),
           "e2m": ops.stsgcn_mix(lp, Ed, ops.MIX_E2M, B, T, N), "e2e_adj": ops.stsgcn_mix(lpt, Ed, ops.MIX_E2E, B, T, N),
           "m2e": ops.stsgcn_mix(lpt, Md, ops.MIX_M2E, B, T, N), "e2f": ops.stsgcn_mix(lpt, Ed, ops.MIX_E2F, B, T, N)}
    torch.cuda.synchronize()
    assert all(got[k].shape == (want[k].numel() // c, c) for k in want)
    _check(parity, {k: _err(got[k].view(want[k].shape), want[k]) for k in want})


def test_mix_refuses_more_nodes_than_its_slab_holds():
    """449 nodes are 29 node tiles, one more than the 64 KB slab holds: the launch answers ESHAPE and writes nothing, the predictor does not claim
    the shape and its forward takes the torch modules"""
    N, c = 449, 16
    assert rows_hip.pad16(N) == 464 and rows_hip.pad16(H.MAX_NODES) == H.MAX_NODES == 448 and 448 * 36 * 4 <= 64 * 1024 < 464 * 36 * 4
    lp, x = torch.zeros(464, 464, device=DEV), torch.randn(3 * N, c, device=DEV)
    for mode in (ops.MIX_F2E, ops.MIX_E2E, ops.MIX_E2M, ops.MIX_M2E, ops.MIX_E2F):
        out = torch.full((3 * N, c), 7.0, device=DEV)
        with pytest.raises(_C.GptstError) as e:
            _C.lib().call("gptst_stsgcn_mix", _C.ptr(lp), 464, _C.ptr(x), _C.ptr(out), c, mode, 1, 3, N, _C.stream())
        torch.cuda.synchronize()
        assert e.value.code == _C.ESHAPE and bool((out == 7.0).all())
    torch.manual_seed(4)
    mh = STSGCN(su.model_args(N, T=3, P=2, layers=1), DEV, 64, 1, backend="hip")
    xin = torch.randn(1, 3, N, 64, device=DEV)
    assert not H.supported(mh, xin)
    assert H.supported(STSGCN(su.model_args(448, T=3, P=2, layers=1), DEV, 64, 1, backend="hip"), torch.randn(1, 3, 448, 64, device=DEV))
    with torch.no_grad():
        y = mh(xin)
    assert mh.backend_used == "torch" and y.shape == (1, 2, N, 1) and bool(torch.isfinite(y).all())


def _glu(pre, co):
    A, S = pre[..., :co], torch.sigmoid(pre[..., co:])
    return A * S, S, A


#            B   W   N  ci  co   what
WINGEMM = [(3, 3, 37, 32, 64),           # ci != co; 3N = 111 and N = 37 are no multiples of 16: tiles are counted inside a (b, w) group
           (2, 2, 20, 128, 128),         # the widest GLU; its mirrored form has 256 input columns: the 32-row weight block
           (128, 10, 20, 16, 64)]        # 512 row tiles per window over 51 workgroups of 8 waves: a wave's loop over its tiles runs twice
# tiles per wave of each case's GLU launch on expanded rows, by hand: ceil(3 N / 16) B row tiles per window, ceil(co / 32) column blocks,
# 1024 // (column blocks * W) row blocks of 8 waves.  The third: 512 tiles, 2 column blocks, 51 row blocks: ceil(512 / 408) = 2
WINGEMM_TPW = {WINGEMM[0]: 1, WINGEMM[1]: 1, WINGEMM[2]: 2}


@pytest.mark.parametrize("B,W,N,ci,co", WINGEMM)
def test_wingemm_per_window_weights(B, W, N, ci, co, parity):
    """expanded and middle rows, GLU with the kept S and A, the ``sharing`` form, and the mirrored form without activation"""
    assert _C.lib().value("gptst_stsgcn_wingemm_tpw", B, W, 3 * N, ci, co, ops.ACT_GLU) == WINGEMM_TPW[(B, W, N, ci, co)]
    g = torch.Generator().manual_seed(ci + co + N)
    Wt = torch.randn(W, 2 * co, ci, generator=g, dtype=torch.float64) / ci ** 0.5
    bs = 0.3 * torch.randn(W, 2 * co, generator=g, dtype=torch.float64)
    want, got = {}, {}
    for name, R in (("exp", 3 * N), ("mid", N)):
        X = torch.randn(B, W, R, ci, generator=g, dtype=torch.float64)
        D = torch.randn(B, W, R, 2 * co, generator=g, dtype=torch.float64)
        y, S, A = _glu(X @ Wt.transpose(-1, -2)[None] + bs[None, :, None, :], co)
        y0 = _glu(X @ Wt[0].t() + bs[0], co)[0]
        assert W == 1 or _err(y0, y) > 1e-2                              # one window's weights for all would fail the comparison below
        want.update({name + ".y": y, name + ".S": S, name + ".A": A, name + ".shared": y0, name + ".mirror": D @ Wt[None]})
        Xd, Dd, Wd, bd = _dev(X, B * W * R, ci), _dev(D, B * W * R, 2 * co), Wt.float().to(DEV), bs.float().to(DEV)
        yd, Sd, Ad = ops.stsgcn_wingemm(Xd, Wd, bd, ops.ACT_GLU, B, W, R, N, keep=True)
        y1 = ops.stsgcn_wingemm(Xd, Wd, bd, ops.ACT_GLU, B, W, R, N)
        ys = ops.stsgcn_wingemm(Xd, Wd[:1].contiguous(), bd[:1].contiguous(), ops.ACT_GLU, B, W, R, N)
        dz = ops.stsgcn_wingemm(Dd, Wd.transpose(1, 2).contiguous(), None, ops.ACT_NONE, B, W, R, N)
        torch.cuda.synchronize()
        assert torch.equal(y1, yd) and dz.shape == (B * W * R, ci)
        got.update({name + ".y": yd, name + ".S": Sd, name + ".A": Ad, name + ".shared": ys, name + ".mirror": dz})
    _check(parity, {k: _err(got[k].view(want[k].shape), want[k]) for k in want})


def test_wingemm_running_max_over_three_calls(parity):
    """the epilogue's max as a layer uses it: operations 0 and 1 on expanded rows, 2 on the middle rows.  best within TOL; which equals the fp64
    argmax on every unambiguous element; the ambiguous share of this input is at most 1e-3, asserted on the reference"""
    B, W, N, ci, co = 3, 3, 37, 32, 64
    g = torch.Generator().manual_seed(7)
    cands, best, which = [], torch.full((B * W * N, co), 9.0, device=DEV), torch.full((B * W * N, co), -1, device=DEV, dtype=torch.int32)
    for j, R in enumerate((3 * N, 3 * N, N)):
        X = torch.randn(B, W, R, ci, generator=g, dtype=torch.float64)
        Wt = torch.randn(W, 2 * co, ci, generator=g, dtype=torch.float64) / ci ** 0.5
        bs = 0.3 * torch.randn(W, 2 * co, generator=g, dtype=torch.float64)
        y = _glu(X @ Wt.transpose(-1, -2)[None] + bs[None, :, None, :], co)[0]
        cands.append(y if R == N else y[:, :, N:2 * N])
        yd = ops.stsgcn_wingemm(_dev(X, B * W * R, ci), Wt.float().to(DEV), bs.float().to(DEV), ops.ACT_GLU, B, W, R, N, best=best, which=which, opj=j)
        parity("cand", _err(yd.view(y.shape), y))
    torch.cuda.synchronize()
    cands = torch.stack(cands)
    top = cands.topk(2, dim=0)[0]
    clear = ((top[0] - top[1]) >= su.GAP * float(cands.abs().max())).reshape(B * W * N, co)
    namb, n = su.ambiguous(cands)
    assert namb <= 1e-3 * n and int(clear.sum()) == n - namb
    wh, arg = which.cpu().long(), cands.argmax(0).reshape(B * W * N, co)
    assert set(wh.unique().tolist()) == {0, 1, 2} and torch.equal(wh[clear], arg[clear])
    _check(parity, {"best": _err(best.view(B, W, N, co), cands.max(0)[0])})


@pytest.mark.parametrize("R3", [True, False])
def test_gate_bwd_routes_by_the_winner_index(R3, parity):
    """``which`` is the test's own, every operation index present; on expanded rows the upstream gradient covers all three blocks and dBest
    lands on the middle one only"""
    B, W, N, co, opj = 3, 2, 37, 48, 1
    R = 3 * N if R3 else N
    g = torch.Generator().manual_seed(R)
    which = torch.randint(0, 3, (B, W, N, co), generator=g)
    assert set(which.unique().tolist()) == {0, 1, 2}
    dBest, S, A = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((B, W, N, co), (B, W, R, co), (B, W, R, co)))
    S = torch.sigmoid(S)
    up = torch.randn(B, W, R, co, generator=g, dtype=torch.float64) if R3 else None
    gsum = (up.clone() if R3 else torch.zeros(B, W, R, co, dtype=torch.float64))
    routed = dBest * (which == opj)
    if R3:
        gsum[:, :, N:2 * N] += routed
    else:
        gsum += routed
    want = torch.cat([gsum * S, gsum * A * S * (1 - S)], -1)
    got = ops.stsgcn_gate_bwd(None if up is None else _dev(up, B * W * R, co), _dev(dBest, B * W * N, co),
                              which.reshape(B * W * N, co).int().contiguous().to(DEV), opj, _dev(S, B * W * R, co), _dev(A, B * W * R, co), B, W, R, N)
    torch.cuda.synchronize()
    _check(parity, {"dPre": _err(got.view(want.shape), want)})


@pytest.mark.parametrize("B,W,N,cw,ci,R3", [(64, 10, 20, 128, 64, True),      # 60 chunks of 64 rows per window over 51 splits: a split's loop runs twice
                                            (3, 3, 37, 64, 32, False),       # the middle rows; the last chunk of a window is part filled
                                            (2, 1, 20, 32, 16, True)])
def test_winwgrad_per_window(B, W, N, cw, ci, R3, parity):
    R = 3 * N if R3 else N
    ns = _C.lib().value("gptst_stsgcn_winwgrad_nsplit", B * R, cw, ci, W)
    nchunks = -(-B * R // 64)
    assert ns >= 1 and (B != 64 or -(-nchunks // ns) >= 2)
    g = torch.Generator().manual_seed(cw + ci)
    D = torch.randn(B, W, R, cw, generator=g, dtype=torch.float64)
    X = torch.randn(B, W, R, ci, generator=g, dtype=torch.float64)
    dW, db = ops.stsgcn_winwgrad(_dev(D, B * W * R, cw), _dev(X, B * W * R, ci), B, W, R)
    torch.cuda.synchronize()
    assert dW.shape == (W, cw, ci) and db.shape == (W, cw)
    _check(parity, {"dW": _err(dW, torch.einsum("bwro,bwri->woi", D, X)), "db": _err(db, D.sum((0, 2)))})


# ---- 2. the whole model ----------------------------------------------------------------------------------------------------------------------
def _ref(N, T, layers, width, module_type="individual", dim_out=1, seed=0, B=2, ap=None):
    """(fp64 torch module on the CPU with non-zero position embeddings, x, w)"""
    torch.manual_seed(seed)
    m64 = STSGCN(su.model_args(N, T=T, P=3, layers=layers, width=width, module_type=module_type) if ap is None else ap, "cpu", 64, dim_out)
    su.randomize_embeddings_(m64)
    m64 = m64.double().train()
    x = torch.randn(B, T, N, 64, dtype=torch.float64)
    return m64, x, torch.randn(B, m64.output_window, N, dim_out, dtype=torch.float64)


def _pair(*a, **kw):
    """(the reference above, its fp32 copy on the GPU with backend hip, x, w)"""
    m64, x, w = _ref(*a, **kw)
    mh = copy.deepcopy(m64).float().to(DEV)
    mh.backend = "hip"
    return m64, mh.train(), x, w


def _run(m, x, w):
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    y = m(xi)
    (y * w).sum().backward()
    out = {"y": y.detach(), "dx": xi.grad}
    out.update({k: p.grad.clone() for k, p in m.named_parameters()})
    return out


def _whole_model(pair, parity):
    """y, dx and every parameter gradient of one batch, on an input whose fp64 reference has no ambiguous element of any layer's max"""
    m64, mh, x, w = pair
    cands = []
    with su.recorded_candidates(m64, cands):
        want = _run(m64, x, w)
    amb = [su.ambiguous(c) for c in cands]
    assert len(cands) == len(m64.stsgcl_layers) and all(a == 0 for a, _ in amb), amb
    got = _run(mh, x.float().to(DEV), w.float().to(DEV))
    assert m64.backend_used == "torch" and mh.backend_used == "hip" and set(got) == set(want) and len(want) == len(m64.state_dict()) + 2
    assert all(float(v.abs().max()) > 0 for v in want.values())
    _check(parity, {k: _err(got[k], want[k]) for k in want})


# seeds for which the fp64 reference has zero ambiguous elements (the test asserts it)
SMALL = [("individual", 1, 0), ("individual", 2, 0), ("sharing", 1, 0), ("sharing", 2, 0)]


@pytest.mark.parametrize("module_type,dim_out,seed", SMALL)
def test_small_model_against_fp64_torch(module_type, dim_out, seed, parity):
    _whole_model(_pair(20, 5, 2, 16, module_type, dim_out, seed), parity)


SHIPPED_NODES = [(170, 1), (207, 1), (250, 0), (266, 0)]       # (of the seeds 0 .. 5, two or three per node count have no ambiguous element)


@pytest.mark.parametrize("N,seed", SHIPPED_NODES)
def test_one_layer_at_the_shipped_node_counts(N, seed, parity):
    """B 1, T 3, one layer of [64, 64, 64]: every launch at the node tiling of a shipped configuration, with gradients"""
    _whole_model(_pair(N, 3, 1, 64, seed=seed, B=1), parity)


# ---- 3. the four shipped confs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds", ["PEMS08", "METR_LA", "NYC_BIKE", "NYC_TAXI"])
def test_shipped_configuration_forward_against_fp64_torch(ds, parity):
    """the predictor as ``-mode eval -model STSGCN`` builds it from the dataset's argument set, one batch element: the forward within TOL of
    fp64 (a near-tie moves a value by less than the tie's gap), the no-grad forward bit-equal to the training one, and one backward whose
    gradients are finite and of the parameters' shapes"""
    pa = predictor_args(ds, "STSGCN")
    N, dim_out = pa.num_nodes, make_args(ds).output_dim
    assert (N, dim_out, len(pa.filter_list)) == {"PEMS08": (170, 1, 4), "METR_LA": (207, 1, 4), "NYC_BIKE": (250, 2, 1), "NYC_TAXI": (266, 2, 1)}[ds]
    ap = SimpleNamespace(**vars(pa), A=su.adjacency(N))
    m64, mh, x, w = _pair(N, 12, None, None, dim_out=dim_out, seed=pa.seed, B=1, ap=ap)
    assert len(m64.state_dict()) == {4: 226, 1: 112}[len(pa.filter_list)]
    with torch.no_grad():
        want = m64(x)
    xd = x.float().to(DEV).requires_grad_(True)
    y = mh(xd)
    assert mh.backend_used == "hip" and y.shape == (1, 12, N, dim_out)
    with torch.no_grad():
        y0 = mh(xd)
    assert mh.backend_used == "hip" and torch.equal(y0, y) and y0.grad_fn is None
    (y * w.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    for k, p in mh.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), k
    assert xd.grad.shape == xd.shape and bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) > 0
    _check(parity, {"y": _err(y, want)})


# ---- 4. launch count and fallbacks -------------------------------------------------------------------------------------------------------------
def test_launches_per_layer_do_not_grow_with_the_windows(monkeypatch):
    """all windows and the whole batch of an operation go in one launch: two launches per forward operation, at 4 windows as at 10"""
    counts = {}
    for name in [n for n in dir(ops) if n.startswith("stsgcn_")]:
        def wrap(*a, _f=getattr(ops, name), _n=name, **kw):
            counts[_n] = counts.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, wrap)
    per_layer = {}
    for T in (6, 12):
        _, mh, x, _ = _pair(20, T, 2, 16, seed=1)
        counts.clear()
        with torch.no_grad():
            mh(x.float().to(DEV))
        assert mh.backend_used == "hip"
        per_layer[T] = {k: v / 2 for k, v in counts.items()}
    assert per_layer[6] == per_layer[12] == {"stsgcn_mix": 3, "stsgcn_wingemm": 3}, per_layer
    _, mh, x, w = _pair(20, 12, 2, 16, seed=1)
    counts.clear()
    _run(mh, x.float().to(DEV), w.float().to(DEV))
    assert counts == {"stsgcn_mix": 12, "stsgcn_wingemm": 12, "stsgcn_gate_bwd": 6, "stsgcn_winwgrad": 6}, counts


def test_relu_and_cpu_input_take_the_torch_modules():
    torch.manual_seed(2)
    ap = su.model_args(20, T=6, P=3, activation="relu")
    mh, mt = STSGCN(ap, DEV, 64, 1, backend="hip"), STSGCN(ap, DEV, 64, 1)
    mt.load_state_dict(mh.state_dict(), strict=True)
    x = torch.randn(2, 6, 20, 64, device=DEV)
    assert not H.supported(mh, x)
    yh, yt = mh(x), mt(x)
    assert mh.backend_used == "torch" and torch.equal(yh, yt)
    mc = STSGCN(su.model_args(20, T=6, P=3), "cpu", 64, 1, backend="hip")
    y = mc(x.cpu())
    assert mc.backend_used == "torch" and y.shape == (2, 3, 20, 1)
    mg = STSGCN(su.model_args(20, T=6, P=3), DEV, 64, 1, backend="hip")
    assert H.supported(mg, x) and not H.supported(mg, x[:, :5]) and not H.supported(mg, x.double())
    mw = STSGCN(su.model_args(20, T=6, P=3, filter_list=[[16, 32, 16]]), DEV, 64, 1, backend="hip")
    assert not H.supported(mw, x)                                      # unequal widths within a layer's filter entry


# ---- 5. the chain ----------------------------------------------------------------------------------------------------------------------------
def _front_end(tmp_path, backend, sd, psd):
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    N = 20
    args = make_args("PEMS08", mode="eval", num_nodes=N, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros(), batch_size=8, epochs=3,
                     early_stop=False, log_dir=str(tmp_path), debug=True, model="STSGCN_test", stsgcn_backend=backend, loss_func="mask_huber")
    sd = O.init_state_dict(args, 4) if sd is None else sd
    torch.manual_seed(0)
    pred = STSGCN(su.model_args(N, T=12, P=12, layers=2), DEV, args.hidden_dim, args.output_dim, backend=args.stsgcn_backend)
    if psd is None:
        su.randomize_embeddings_(pred)
    else:
        pred.load_state_dict(psd, strict=True)
    model = EnhanceFrontEnd(args, predictor=pred, finetune_encoder=False).to(DEV)
    model.load_pretrained_model(sd)
    return args, sd, model, EvalTrainer


def test_chain_two_huber_steps_agree_with_the_torch_backend(tmp_path, parity):
    args, sd, mh, ET = _front_end(tmp_path, "hip", None, None)
    _, _, mt, _ = _front_end(tmp_path, "torch", sd, mh.predictor.state_dict())
    mt.load_state_dict(mh.state_dict(), strict=True)
    src = synth.make_batch(2, 12, 20, 1, interval=args.interval, seed=21).to(DEV)
    tgt = synth.make_batch(2, 12, 20, 1, interval=args.interval, seed=22, start_slot=12).to(DEV)
    losses = {}
    for name, model in (("hip", mh), ("torch", mt)):
        tr = ET(model, args, None, None, None, synth.SCALER_MEAN, synth.SCALER_STD)
        tr.logger.setLevel(logging.WARNING)
        model.train()
        losses[name] = []
        for _ in range(2):
            tr.opt.zero_grad()
            loss = tr._loss(model(src, tgt)[0], tgt)
            loss.backward()
            tr.opt.step()
            assert model.predictor.backend_used == name
            losses[name].append(float(loss.detach()))
    assert losses["torch"][0] != losses["torch"][1]
    _check(parity, {"loss%d" % i: abs(losses["hip"][i] - losses["torch"][i]) / abs(losses["torch"][i]) for i in range(2)})
