"""The STFGNN predictor on HIP (``STFGNN(..., backend="hip")``, csrc/stfgnn.hip, predictors/stfgnn_hip.py) on the GPU.  The reference of every
comparison is fp64 torch on the CPU — the definition of a launch (tests/stfgnn_util.py, checked against the module by test_stfgnn_hip_cpu.py),
or the torch STFGNN module (pinned to the reference implementation's vectors by tests/test_predictor_stfgnn.py); the bound is the project's
element-wise one, 1e-4 of the reference tensor's largest magnitude, for every output, dX and parameter gradient.

The max and near-ties are handled as in test_gpu_stsgcn_hip.py: an element is ambiguous if its top-two gap on the fp64 reference is below
GAP = 1e-5 of the largest candidate magnitude; gradient comparisons of whole models use shapes and seeds for which the test asserts ZERO
ambiguous elements (the seeds were chosen on the CPU); the full confs are compared on the forward only.  The candidate error measured here is
recorded as ``cand``.

The mix runs at the widths 16, 32, 48, 64, 80, 112 and 128 (one column tile, full 32-channel groups, a half-filled last group behind one to
three full ones, four groups), at 128 with 3 and with 20 node tiles, as test_gpu_stsgcn_hip.py holds the same slab product."""
import copy
import logging
from types import SimpleNamespace

import pytest
import torch

import stfgnn_util as fu
from gptst_amd import _C, graph, ops, synth
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import STFGNN, stfgnn_hip as H, rows_hip
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
MIX = [(3, 3, 20, 64),            # a padded tile; frames fed by one to four blocks
       (1, 1, 16, 16),            # no padding, one window, half a channel group
       (3, 2, 37, 48),            # a second channel group half filled
       (1, 9, 20, 32),            # the conf's window count
       (1, 1, 170, 64), (1, 1, 266, 64),          # shipped node counts: 11 and 17 node tiles (the last workgroup has waves without a tile)
       (1, 2, 305, 16),           # 20 node tiles, the last with ONE real node
       (1, 1, 448, 16),           # the largest node count served: 63 KB of LDS
       (3, 9, 37, 128),           # the widest rows (four channel groups) at the conf's window count, three samples
       (2, 3, 37, 80), (2, 3, 37, 112),           # a half-filled last group behind two and three full ones
       (1, 1, 320, 128)]          # 20 node tiles at the widest rows


@pytest.mark.parametrize("B,W,N,c", MIX)
def test_mix_every_form(B, W, N, c, parity):
    """two different non-symmetric graphs: a swapped or transposed operand fails; the adjoint forms are called with S^T, D^T as the predictor
    calls them"""
    T = W + 3
    g = torch.Generator().manual_seed(N + c + W)
    S = torch.randn(N, N, generator=g, dtype=torch.float64) / N ** 0.5
    D = torch.randn(N, N, generator=g, dtype=torch.float64) / N ** 0.5
    Hf = torch.randn(B, T, N, c, generator=g, dtype=torch.float64)
    E = torch.randn(B, W, 4, N, c, generator=g, dtype=torch.float64)
    M = torch.randn(B, W, N, c, generator=g, dtype=torch.float64)
    assert float((S - S.t()).abs().max()) > 1e-2 and float((D - D.t()).abs().max()) > 1e-2 and float((S - D).abs().max()) > 1e-2
    want = {"f2e": fu.mix_f2e(S, D, Hf), "e2e": fu.mix_expanded(S, D, E), "e2m": fu.mix_middle(S, E),
            "e2e_adj": fu.mix_expanded(S.t(), D.t(), E), "m2e": fu.mix_m2e(S.t(), M), "e2f": fu.mix_e2f(S.t(), D.t(), E)}
    sp, dp, spt, dpt = _pad(S), _pad(D), _pad(S.t()), _pad(D.t())
    Hd, Ed, Md = _dev(Hf, B * T * N, c), _dev(E, B * W * 4 * N, c), _dev(M, B * W * N, c)

    def run():
        return {"f2e": ops.stfgnn_mix(sp, dp, Hd, ops.MIX_F2E, B, T, N), "e2e": ops.stfgnn_mix(sp, dp, Ed, ops.MIX_E2E, B, T, N),
                "e2m": ops.stfgnn_mix(sp, dp, Ed, ops.MIX_E2M, B, T, N), "e2e_adj": ops.stfgnn_mix(spt, dpt, Ed, ops.MIX_E2E, B, T, N),
                "m2e": ops.stfgnn_mix(spt, dpt, Md, ops.MIX_M2E, B, T, N), "e2f": ops.stfgnn_mix(spt, dpt, Ed, ops.MIX_E2F, B, T, N)}
    got, again = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(got[k], again[k]) for k in want)                                              # fixed summation order: bit-equal
    assert all(got[k].shape == (want[k].numel() // c, c) for k in want)
    f2e, e2e = got["f2e"].view(B, W, 4, N, c), got["e2e"].view(B, W, 4, N, c)
    assert torch.equal(f2e[:, :, 0], f2e[:, :, 3]) and torch.equal(e2e[:, :, 0], e2e[:, :, 3])          # one product, written to both blocks
    _check(parity, {k: _err(got[k].view(want[k].shape), want[k]) for k in want})


def test_mix_refuses_more_nodes_than_its_slab_holds():
    """449 nodes are 29 node tiles, one more than the 64 KB slab holds: the launch answers ESHAPE and writes nothing, the predictor does not claim
    the shape and its forward takes the torch modules"""
    N, c = 449, 16
    assert rows_hip.pad16(N) == 464 and rows_hip.pad16(H.MAX_NODES) == H.MAX_NODES == 448 and 448 * 36 * 4 <= 64 * 1024 < 464 * 36 * 4
    lp, x = torch.zeros(464, 464, device=DEV), torch.randn(4 * N, c, device=DEV)
    for mode in (ops.MIX_F2E, ops.MIX_E2E, ops.MIX_E2M, ops.MIX_M2E, ops.MIX_E2F):
        out = torch.full((4 * N, c), 7.0, device=DEV)
        with pytest.raises(_C.GptstError) as e:
            _C.lib().call("gptst_stfgnn_mix", _C.ptr(lp), _C.ptr(lp), 464, _C.ptr(x), _C.ptr(out), c, mode, 1, 4, N, _C.stream())
        torch.cuda.synchronize()
        assert e.value.code == _C.ESHAPE and bool((out == 7.0).all())
    torch.manual_seed(4)
    mh = STFGNN(fu.model_args(N, T=4, P=2, layers=1), DEV, 64, backend="hip")
    xin = torch.randn(1, 4, N, 64, device=DEV)
    assert not H.supported(mh, xin)
    assert H.supported(STFGNN(fu.model_args(448, T=4, P=2, layers=1), DEV, 64, backend="hip"), torch.randn(1, 4, 448, 64, device=DEV))
    with torch.no_grad():
        y = mh(xin)
    assert mh.backend_used == "torch" and y.shape == (1, 2, N, 1) and bool(torch.isfinite(y).all())


def _glu(pre, co):
    A, S = pre[..., :co], torch.sigmoid(pre[..., co:])
    return A * S, S, A


#            B  W   N   ci   co
WINGEMM = [(3, 3, 37, 32, 64),           # ci != co; 4N = 148 is no multiple of 16: tiles are counted inside a (b, w) group
           (2, 2, 20, 128, 128)]         # the widest GLU; its mirrored form has 256 input columns: the 32-row weight block


@pytest.mark.parametrize("B,W,N,ci,co", WINGEMM)
def test_four_block_window_kernels(B, W, N, ci, co, parity):
    """stsgcn_wingemm, stsgcn_gate_bwd and stsgcn_winwgrad on groups of R = 4N rows: GLU with the kept S and A, the mirrored form without
    activation, dBest landing on rows N .. 2N of a group only, the weight gradient per window"""
    R = 4 * N
    g = torch.Generator().manual_seed(ci + co + N)
    Wt = torch.randn(W, 2 * co, ci, generator=g, dtype=torch.float64) / ci ** 0.5
    bs = 0.3 * torch.randn(W, 2 * co, generator=g, dtype=torch.float64)
    X = torch.randn(B, W, R, ci, generator=g, dtype=torch.float64)
    D = torch.randn(B, W, R, 2 * co, generator=g, dtype=torch.float64)
    y, S, A = _glu(X @ Wt.transpose(-1, -2)[None] + bs[None, :, None, :], co)
    assert W == 1 or _err(_glu(X @ Wt[0].t() + bs[0], co)[0], y) > 1e-2          # one window's weights for all would fail the comparison below
    want = {"y": y, "S": S, "A": A, "mirror": D @ Wt[None]}
    Xd, Dd, Wd, bd = _dev(X, B * W * R, ci), _dev(D, B * W * R, 2 * co), Wt.float().to(DEV), bs.float().to(DEV)
    best = torch.full((B * W * N, co), 9.0, device=DEV)
    which = torch.full((B * W * N, co), -1, device=DEV, dtype=torch.int32)
    yd, Sd, Ad = ops.stsgcn_wingemm(Xd, Wd, bd, ops.ACT_GLU, B, W, R, N, keep=True, best=best, which=which, opj=0)
    y1 = ops.stsgcn_wingemm(Xd, Wd, bd, ops.ACT_GLU, B, W, R, N)
    dz = ops.stsgcn_wingemm(Dd, Wd.transpose(1, 2).contiguous(), None, ops.ACT_NONE, B, W, R, N)
    torch.cuda.synchronize()
    assert torch.equal(y1, yd) and dz.shape == (B * W * R, ci)
    assert torch.equal(best.view(B, W, N, co), yd.view(B, W, R, co)[:, :, N:2 * N]) and bool((which == 0).all())     # the crop is rows N .. 2N
    got = {"y": yd, "S": Sd, "A": Ad, "mirror": dz}
    # gate_bwd: the upstream gradient covers all four blocks, dBest lands on block 1 only
    opj = 1
    whichr = torch.randint(0, 3, (B, W, N, co), generator=g)
    assert set(whichr.unique().tolist()) == {0, 1, 2}
    dBest, up = torch.randn(B, W, N, co, generator=g, dtype=torch.float64), torch.randn(B, W, R, co, generator=g, dtype=torch.float64)
    gsum = up.clone()
    gsum[:, :, N:2 * N] += dBest * (whichr == opj)
    want["dPre"] = torch.cat([gsum * S, gsum * A * S * (1 - S)], -1)
    got["dPre"] = ops.stsgcn_gate_bwd(_dev(up, B * W * R, co), _dev(dBest, B * W * N, co), whichr.reshape(B * W * N, co).int().contiguous().to(DEV),
                                      opj, _dev(S, B * W * R, co), _dev(A, B * W * R, co), B, W, R, N)
    only = ops.stsgcn_gate_bwd(None, _dev(dBest, B * W * N, co), whichr.reshape(B * W * N, co).int().contiguous().to(DEV),
                               opj, _dev(S, B * W * R, co), _dev(A, B * W * R, co), B, W, R, N).view(B, W, R, 2 * co)
    torch.cuda.synchronize()
    assert not bool(only[:, :, :N].any()) and not bool(only[:, :, 2 * N:].any()) and bool(only[:, :, N:2 * N].any())
    dW, db = ops.stsgcn_winwgrad(Dd, Xd, B, W, R)
    torch.cuda.synchronize()
    assert dW.shape == (W, 2 * co, ci) and db.shape == (W, 2 * co)
    want.update({"dW": torch.einsum("bwro,bwri->woi", D, X), "db": D.sum((0, 2))})
    got.update({"dW": dW, "db": db})
    _check(parity, {k: _err(got[k].view(want[k].shape), want[k]) for k in want})


RUNNING_MAX_SEED = 7        # chosen on the CPU: the ambiguous share of this input is below 1e-3 (asserted)


def test_wingemm_running_max_over_three_calls(parity):
    """the epilogue's max as a layer uses it: operations 0 and 1 on groups of 4N rows, 2 on the middle rows.  best within TOL; which equals the
    fp64 argmax on every unambiguous element; the ambiguous share of this input is at most 1e-3, asserted on the reference"""
    B, W, N, ci, co = 3, 3, 37, 32, 64
    g = torch.Generator().manual_seed(RUNNING_MAX_SEED)
    cands, best, which = [], torch.full((B * W * N, co), 9.0, device=DEV), torch.full((B * W * N, co), -1, device=DEV, dtype=torch.int32)
    for j, R in enumerate((4 * N, 4 * N, N)):
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
    clear = ((top[0] - top[1]) >= fu.GAP * float(cands.abs().max())).reshape(B * W * N, co)
    namb, n = fu.ambiguous(cands)
    assert namb <= 1e-3 * n and int(clear.sum()) == n - namb
    wh, arg = which.cpu().long(), cands.argmax(0).reshape(B * W * N, co)
    assert set(wh.unique().tolist()) == {0, 1, 2} and torch.equal(wh[clear], arg[clear])
    _check(parity, {"best": _err(best.view(B, W, N, co), cands.max(0)[0])})


def test_gated_branch_through_the_tap_gemm(parity):
    """offsets (0, 3), T 9 -> 6, N 37, c 32 -> 48 against the module's own conv arithmetic in fp64: y and the conv1 / conv2 weight and bias
    gradients — a swapped tanh / sigmoid half or a swapped tap fails"""
    B, T, N, ci, co = 2, 9, 37, 32, 48
    torch.manual_seed(5)
    lay = STFGNN(fu.model_args(N, T=T, P=2, layers=1, hidden_dims=[[co, co, co]], first_layer_embedding_size=ci), "cpu", 64).STSGCLS[0].double()
    x = torch.randn(B, T, N, ci, dtype=torch.float64, requires_grad=True)
    w = torch.randn(B, T - 3, N, co, dtype=torch.float64)
    y = lay.gated(x)
    (y * w).sum().backward()
    want = {"y": y, "dx": x.grad, "conv1.w": lay.conv1.weight.grad, "conv1.b": lay.conv1.bias.grad, "conv2.w": lay.conv2.weight.grad,
            "conv2.b": lay.conv2.bias.grad}
    assert _err(want["conv1.w"], want["conv2.w"]) > 1e-2 and _err(want["conv1.w"].flip(-1), want["conv1.w"]) > 1e-2
    ld = copy.deepcopy(lay).float().to(DEV)
    ld.zero_grad(set_to_none=True)
    xd = x.detach().float().to(DEV).requires_grad_(True)
    Wg, bg = H.gate_weight(ld)
    yd = H._GateFn.apply(xd.view(B * T * N, ci), Wg, bg, B, T, N, True)
    (yd.view(B, T - 3, N, co) * w.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = {"y": yd.view(B, T - 3, N, co), "dx": xd.grad, "conv1.w": ld.conv1.weight.grad, "conv1.b": ld.conv1.bias.grad,
           "conv2.w": ld.conv2.weight.grad, "conv2.b": ld.conv2.bias.grad}
    _check(parity, {k: _err(got[k], want[k]) for k in want})


# ---- 2. the whole model ----------------------------------------------------------------------------------------------------------------------
def _ref(N, T, layers, width, dim_out=1, seed=0, B=2, ap=None):
    """(fp64 torch module on the CPU with position embeddings of size 0.3, x, w)"""
    torch.manual_seed(seed)
    m64 = STFGNN(fu.model_args(N, T=T, P=3, layers=layers, width=width, output_dim=dim_out) if ap is None else ap, "cpu", 64)
    fu.randomize_embeddings_(m64)
    m64 = m64.double().train()
    x = torch.randn(B, T, N, 64, dtype=torch.float64)
    return m64, x, torch.randn(B, m64.horizon, N, m64.output_dim, dtype=torch.float64)


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
    with fu.recorded_candidates(m64, cands):
        want = _run(m64, x, w)
    amb = [fu.ambiguous(c) for c in cands]
    assert len(cands) == len(m64.STSGCLS) and all(a == 0 for a, _ in amb), amb
    got = _run(mh, x.float().to(DEV), w.float().to(DEV))
    assert m64.backend_used == "torch" and mh.backend_used == "hip" and set(got) == set(want) and len(want) == len(m64.state_dict()) + 2
    assert all(float(v.abs().max()) > 0 for v in want.values())
    _check(parity, {k: _err(got[k], want[k]) for k in want})


# seeds for which the fp64 reference has zero ambiguous elements (the test asserts it)
SMALL = [(1, 52), (2, 1)]          # (dim_out, seed): of the seeds 0 .. 52 most have a handful of ambiguous elements in the second layer


@pytest.mark.parametrize("dim_out,seed", SMALL)
def test_small_model_against_fp64_torch(dim_out, seed, parity):
    _whole_model(_pair(20, 9, 2, 16, dim_out, seed), parity)


SHIPPED_NODES = [(170, 3), (207, 3), (250, 4), (266, 5)]       # (of the seeds 0 .. 5, one to three per node count have no ambiguous element)


@pytest.mark.parametrize("N,seed", SHIPPED_NODES)
def test_one_layer_at_the_shipped_node_counts(N, seed, parity):
    """B 1, T 4, one layer of [64, 64, 64]: every launch at the node tiling of a shipped configuration, with gradients"""
    _whole_model(_pair(N, 4, 1, 64, seed=seed, B=1), parity)


# ---- 3. the four shipped confs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds", ["PEMS08", "METR_LA", "NYC_BIKE", "NYC_TAXI"])
def test_shipped_configuration_forward_against_fp64_torch(ds, parity):
    """the predictor as ``-mode eval -model STFGNN`` builds it from the dataset's argument set, one batch element: the forward within TOL of
    fp64 (a near-tie moves a value by less than the tie's gap), the no-grad forward bit-equal to the training one, and one backward whose
    gradients are finite and of the parameters' shapes"""
    pa = predictor_args(ds, "STFGNN")
    N, dim_out = pa.num_nodes, pa.output_dim
    assert (N, dim_out, len(pa.hidden_dims)) == {"PEMS08": (170, 1, 3), "METR_LA": (207, 1, 3), "NYC_BIKE": (250, 2, 1), "NYC_TAXI": (266, 2, 1)}[ds]
    ap = SimpleNamespace(**vars(pa), adj=graph.stfgnn_fusion_graph(*fu.graphs(N)))
    m64, mh, x, w = _pair(N, 12, None, None, seed=pa.seed, B=1, ap=ap)
    assert len(m64.state_dict()) == {3: 176, 1: 110}[len(pa.hidden_dims)]
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
    """all windows and the whole batch of an operation go in one launch: two launches per forward operation and one for the gated branch, at
    4 windows as at 9"""
    counts = {}
    for name in [n for n in dir(ops) if n.startswith(("stsgcn_", "stfgnn_", "mtgnn_"))]:
        def wrap(*a, _f=getattr(ops, name), _n=name, **kw):
            counts[_n] = counts.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, wrap)
    first = {}
    for T in (7, 12):
        _, mh, x, _ = _pair(20, T, 1, 16, seed=1)
        counts.clear()
        with torch.no_grad():
            mh(x.float().to(DEV))
        assert mh.backend_used == "hip"
        first[T] = dict(counts)
    assert first[7] == first[12] == {"stfgnn_mix": 3, "stsgcn_wingemm": 3, "mtgnn_tapgemm": 1}, first
    _, mh, x, w = _pair(20, 12, 2, 16, seed=1)
    counts.clear()
    _run(mh, x.float().to(DEV), w.float().to(DEV))
    # per layer: forward 3 mix + 3 GEMMs + the gate; backward 3 gate_bwd, 3 weight gradients, 3 mirrored GEMMs, 3 adjoint mixes, and the gate's
    # gate_bwd, weight gradient and mirrored tap GEMM
    assert counts == {"stfgnn_mix": 12, "stsgcn_wingemm": 12, "stsgcn_gate_bwd": 6, "stsgcn_winwgrad": 6, "mtgnn_tapgemm": 4, "mtgnn_gate_bwd": 2,
                      "mtgnn_wgrad": 2}, counts


def test_fallbacks_take_the_torch_modules():
    torch.manual_seed(2)
    x = torch.randn(2, 9, 20, 64, device=DEV)

    def same_as_torch(ap, xin, dev=DEV):
        mh, mt = STFGNN(ap, dev, 64, backend="hip"), STFGNN(ap, dev, 64)
        mt.load_state_dict(mh.state_dict(), strict=True)
        assert not H.supported(mh, xin)
        yh, yt = mh(xin), mt(xin)
        assert mh.backend_used == "torch" and mt.backend_used == "torch" and torch.equal(yh, yt)
        return mh
    same_as_torch(fu.model_args(20, activation="relu"), x)                                          # relu
    same_as_torch(fu.model_args(20), x.cpu(), "cpu")                                                # CPU input
    other = graph.stfgnn_fusion_graph(*fu.graphs(20))
    other[3, 47] = 0.5
    assert same_as_torch(fu.model_args(20, adj=other), x).s_hat is None                             # an unrecognised fusion matrix
    mg = STFGNN(fu.model_args(20), DEV, 64, backend="hip")
    assert H.supported(mg, x)
    for bad in (x[:, :8], x.double()):                                                              # the wrong window, fp64
        assert not H.supported(mg, bad)
    with pytest.raises(RuntimeError):                                                               # (a window of another length fits no
        mg(x[:, :8])                                                                                # embedding or weight stack of the torch modules either)
    assert mg.backend_used == "torch"
    md = copy.deepcopy(mg).double()
    y = md(x.double())
    assert md.backend_used == "torch" and y.dtype == torch.float64
    with torch.no_grad():
        assert float((mg(x) - y.float()).abs().max()) < 1e-3 * float(y.abs().max()) and mg.backend_used == "hip"
    mw = STFGNN(fu.model_args(20, hidden_dims=[[16, 32, 16]]), DEV, 64, backend="hip")              # unequal widths within a layer: the max over the
    assert not H.supported(mw, x)                                                                   # operations is undefined on either backend
    with pytest.raises(RuntimeError):
        mw(x)
    assert mw.backend_used == "torch"
    m2 = same_as_torch(fu.model_args(20, hidden_dims=[[16]]), x)                                    # fewer than two operations
    assert m2.backend_used == "torch"


# ---- 5. the chain ----------------------------------------------------------------------------------------------------------------------------
def _front_end(tmp_path, backend, sd, psd):
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    N = 20
    args = make_args("PEMS08", mode="eval", num_nodes=N, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros(), batch_size=8, epochs=3,
                     early_stop=False, log_dir=str(tmp_path), debug=True, model="STFGNN_test", stfgnn_backend=backend, loss_func="mask_huber")
    sd = O.init_state_dict(args, 4) if sd is None else sd
    torch.manual_seed(0)
    pred = STFGNN(fu.model_args(N, T=12, P=12, layers=2, first_layer_embedding_size=16), DEV, args.hidden_dim, backend=args.stfgnn_backend)
    if psd is None:
        fu.randomize_embeddings_(pred)
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
