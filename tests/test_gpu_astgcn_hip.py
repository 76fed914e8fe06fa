"""The ASTGCN predictor on HIP (``ASTGCN(..., backend="hip")``, csrc/astgcn.hip, predictors/astgcn_hip.py) on the GPU.  The reference of every
comparison is fp64 torch on the CPU — the definition of a launch, or the torch ASTGCN module (pinned to the reference implementation's vectors by
tests/test_predictor_astgcn.py); the bound is the project's element-wise one, 1e-4 of the reference tensor's largest magnitude, for every
output, dX and parameter gradient."""
import copy
import logging
from types import SimpleNamespace

import pytest
import torch

import astgcn_util as au
from gptst_amd import _C, graph, ops, synth
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import ASTGCN, astgcn_hip as H, rows_hip
from gptst_amd.predictors.rows_hip import TapFn
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
       (2, 12, 70, 128, 3),           # more than four node tiles, two channel groups
       # the first padded node count of each K whose masked tiles and slab pass the 64 KB a launch gets without asking for more: expand and
       # reduce of a case are two template instances, so the three cases set the attribute of all six
       (2, 2, 129, 64, 3),            # and 9 node tiles: the last workgroup of the graph gradient has three waves without a tile
       (2, 2, 145, 64, 2),
       (2, 2, 177, 64, 1),
       (2, 2, 320, 64, 3),            # the largest node count served: all of a CU's LDS, every float4 of the prefetch array in use
       (1, 2, 305, 32, 3),            # the same 20 node tiles, the last with ONE real node
       (2, 3, 37, 16, 3),             # widths that are no multiple of 64: the (second) channel group has one to three live waves
       (2, 3, 37, 48, 3),
       (2, 3, 37, 80, 3),
       (2, 3, 37, 112, 3),
       (2, 3, 37, 96, 2),
       (1, 1, 16, 16, 1),             # T = 1, one group, expand: ONE slab in the walk, the first fetch has no successor
       (1, 1, 20, 128, 3)]            # the shortest walk with two groups (reduce: 6 slabs)
# (N, K) -> bytes of dynamic LDS of the cases beyond 64 KB, and for the boundary cases the padded node count one tile below, still within
MIX_LDS = {(129, 3): 73728, (145, 2): 69120, (177, 1): 67584, (320, 3): 163840, (305, 3): 163840}
MIX_BELOW = {(145, 2): 144, (177, 1): 176}


def _mix_lds(Np, K):
    """bytes of dynamic LDS of the mix, from the function the launch sizes with (include/gptst_hip_testing.h)"""
    return _C.lib().value("gptst_astgcn_attmix_lds", Np, K)


@pytest.mark.parametrize("B,T,N,c,K", MIX)
def test_masked_mix_and_its_graph_gradient(B, T, N, c, K, parity):
    """non-symmetric T_k and S, S different for every b: a transposed operand, or one sample's graph used for all, fails"""
    lds = _mix_lds(rows_hip.pad16(N), K)
    assert (lds > 64 * 1024) == ((N, K) in MIX_LDS) and lds == MIX_LDS.get((N, K), lds), lds
    if (N, K) in MIX_BELOW:
        assert 0 < _mix_lds(MIX_BELOW[N, K], K) <= 64 * 1024 and MIX_BELOW[N, K] == rows_hip.pad16(N) - 16
    if N >= 305:
        assert lds == rows_hip.LDS_MAX and rows_hip.pad16(N) == 320
    g = torch.Generator().manual_seed(N + c)
    Tk = torch.randn(K, N, N, generator=g, dtype=torch.float64)
    S = torch.softmax(torch.randn(B, N, N, generator=g, dtype=torch.float64), dim=1)
    x = torch.randn(B, T, N, c, generator=g, dtype=torch.float64)
    G = torch.randn(B, T, N, K, c, generator=g, dtype=torch.float64)
    res = torch.randn(B, T, N, c, generator=g, dtype=torch.float64)
    # the definitions as matmuls with the masked graph M[b,k,m,n] = T_k[m,n] S[b,m,n] (the five-index contractions take seconds at 320 nodes)
    M, Gk = Tk[None] * S[:, None], G.permute(0, 1, 3, 2, 4)                                    # Gk (B, T, K, N, c)
    want = {"expand": (M.transpose(2, 3)[:, None] @ x[:, :, None]).permute(0, 1, 3, 2, 4).reshape(B * T * N, K * c),
            "reduce": (M[:, None] @ Gk).sum(2).reshape(B * T * N, c),
            "attgrad": (Tk[None] * (x[:, :, None] @ Gk.transpose(3, 4)).sum(1)).sum(1)}
    if N <= 70:                                                                                # the same thing, as written in csrc/astgcn.hip
        ein = {"expand": torch.einsum("kmn,bmn,btmc->btnkc", Tk, S, x).reshape(B * T * N, K * c),
               "reduce": torch.einsum("kmn,bmn,btnkc->btmc", Tk, S, G).reshape(B * T * N, c),
               "attgrad": torch.einsum("kmn,btmc,btnkc->bmn", Tk, x, G)}
        assert all(float((ein[k] - want[k]).abs().max()) <= 1e-12 * float(ein[k].abs().max()) for k in ein)
    want["reduce_res"] = want["reduce"] + res.reshape(B * T * N, c)
    assert (B == 1 or float((S[0] - S[1]).abs().max()) > 1e-3) and float((S[0] - S[0].t()).abs().max()) > 1e-3
    f = lambda t, *shape: t.float().reshape(*shape).contiguous().to(DEV)                       # noqa: E731
    tp, Sd, xd, Gd, rd = _pad(Tk).float().to(DEV), f(S, B, N, N), f(x, B * T * N, c), f(G, B * T * N, K * c), f(res, B * T * N, c)
    got = {"expand": ops.astgcn_attmix(tp, Sd, xd, T, c, reduce=False),
           "reduce": ops.astgcn_attmix(tp, Sd, Gd, T, c, reduce=True),
           "reduce_res": ops.astgcn_attmix(tp, Sd, Gd, T, c, reduce=True, res=rd),
           "attgrad": ops.astgcn_attgrad(tp, xd, Gd, B, T, N)}
    torch.cuda.synchronize()
    _check(parity, {k: _err(got[k], want[k]) for k in want})


def test_mix_refuses_more_nodes_than_its_lds_holds():
    """321 nodes are 21 node tiles, one more than the prefetch array and the LDS of a CU hold: the launch answers ESHAPE for every K (at K = 1 the
    bytes alone would fit), the predictor does not claim the shape and its forward takes the torch modules"""
    N, c, T = 321, 16, 1
    assert rows_hip.pad16(N) == 336 and _mix_lds(320, 3) == rows_hip.LDS_MAX
    assert [_mix_lds(336, k) for k in (1, 2, 3)] == [_C.ESHAPE] * 3 and 0 < 336 * (20 + 68) * 4 < rows_hip.LDS_MAX
    assert (_mix_lds(0, 3), _mix_lds(16, 0), _mix_lds(24, 1), _mix_lds(16, 4)) == (-1, -1, _C.ESHAPE, _C.ESHAPE)
    S, x = torch.softmax(torch.randn(1, N, N, device=DEV), dim=1), torch.randn(N, c, device=DEV)
    for K in (1, 3):
        tp = torch.zeros(K, 336, 336, device=DEV)
        for reduce in (False, True):
            with pytest.raises(_C.GptstError) as e:
                ops.astgcn_attmix(tp, S, x.repeat(1, K) if reduce else x, T, c, reduce=reduce)
            assert e.value.code == _C.ESHAPE
    out = torch.full((N, 3 * c), 7.0, device=DEV)                         # the entry point itself, K = 3, into a buffer of the test's: nothing is written
    with pytest.raises(_C.GptstError) as e:
        _C.lib().call("gptst_astgcn_attmix", _C.ptr(tp), 336, 3, _C.ptr(S), _C.ptr(x), _C.ptr(out), None, c, 0, 1, T, N, _C.stream())
    torch.cuda.synchronize()
    assert e.value.code == _C.ESHAPE and bool((out == 7.0).all())
    torch.manual_seed(4)
    mh = ASTGCN(_ap(N), DEV, 64, 1, backend="hip")
    au.xavier_pass_(mh)
    au.move_score_vectors_(mh)
    au.scale_u1_(mh, N)
    xin = torch.randn(1, 12, N, 64, device=DEV)
    assert not H.supported(mh, xin) and H.supported(ASTGCN(_ap(320), DEV, 64, 1, backend="hip"), torch.randn(1, 12, 320, 64, device=DEV))
    with torch.no_grad():
        y = mh(xin)
    assert mh.backend_used == "torch" and y.shape == (1, 12, N, 1) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("rows,c", [(1003, 16), (1003, 64), (1003, 128), (131077, 16),
                                    (1003, 32), (1003, 48), (1003, 80), (1003, 96), (1003, 112), (65793, 48), (65793, 112), (131077, 80)])
def test_row_layernorm(rows, c, parity):
    """1003 rows: no multiple of the 16 rows of a pass; 131077 rows: more than the 8192 x 16 rows of one sweep of the grid, and the most splits.
    Widths 48, 80, 96 and 112: 256 / c row-lanes of the parameter gradient leave threads idle, and from 80 on the second half-row is partly
    filled (at 131077 rows in the second sweep too).  65793 rows: 256 splits of 258 rows, the last one with 3 rows — fewer than the five
    row-lanes of width 48"""
    if rows == 65793:
        ns = _C.lib().value("gptst_astgcn_rowln_nsplit", rows)
        rps = -(-rows // ns)
        assert (ns, rps, rows - (ns - 1) * rps) == (256, 258, 3) and (c != 48 or 256 // c == 5)
    if rows == 131077:
        assert rows > 8192 * 16
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


# The launches of csrc/stgcn.hip in the forms only this predictor makes, at 6 x 12 x 920 = 66 240 rows (4 140 row tiles, 1 035 chunks of 64): a
# wave's loop over its row tiles, a split's loop over its chunks and the gate backward's grid-stride loop all run more than once, as at every
# real batch.  920 nodes are no multiple of 16, and the taps cross the ends of six samples.
BTN = (6, 12, 920)


def _shared_plan(co, ktot, act, bwd_co, bwd_ktot, gate):
    """asserts that the launches of a case are on the multi-tile paths -> tiles per wave of the forward and of the data backward (the plan query of
    include/gptst_hip_testing.h), 64-row chunks per split of the weight gradient"""
    v, rows = _C.lib().value, BTN[0] * BTN[1] * BTN[2]
    fwd, bwd = v("gptst_stgcn_tapgemm_tpw", rows, co, ktot, act), v("gptst_stgcn_tapgemm_tpw", rows, bwd_co, bwd_ktot, ops.ACT_NONE)
    nchunks = -(-rows // 64)
    cps = -(-nchunks // v("gptst_stgcn_wgrad_nsplit", rows, co, ktot))
    assert fwd >= 2 and bwd >= 2 and cps >= 2, (fwd, bwd, cps)
    assert not gate or rows * co // 4 > 4096 * 256                          # the gate backward's grid is 4096 workgroups of 256 float4s
    return fwd, bwd, cps


def test_theta_gemm_several_tiles_per_wave(parity):
    """relu(Z Theta^T) and its backward, called on ``ops`` as astgcn_hip._MixFn does: no bias, one tap over Ktot = 192, the gate backward from the
    kept output, the weight gradient without a bias sum, and the data backward with co = 192 (three column blocks, linear epilogue)"""
    B, T, N = BTN
    rows, c, K, co = B * T * N, 64, 3, 64
    assert _shared_plan(co, K * c, ops.ACT_RELU, K * c, co, True) == (2, 4, 4)
    g = torch.Generator().manual_seed(192)
    Z = torch.randn(rows, K * c, generator=g, dtype=torch.float64).requires_grad_(True)
    Th = (torch.randn(co, K * c, generator=g, dtype=torch.float64) / (K * c) ** 0.5).requires_grad_(True)
    w = torch.randn(rows, co, generator=g, dtype=torch.float64)
    y = torch.relu(au.tap(Z.view(B, T, N, K * c), Th, None, (0,))).view(rows, co)
    (y * w).sum().backward()
    Zd, Thd, wd = (t.detach().float().to(DEV) for t in (Z, Th, w))
    yd = ops.stgcn_tapgemm(Zd, Thd, None, (0,), ops.ACT_RELU, T, N)
    dPre = ops.stgcn_gate_bwd(wd, ops.ACT_RELU, out=yd)
    dTh, none = ops.stgcn_wgrad(dPre, Zd, (0,), T, N, want_bias=False)
    Gd = ops.stgcn_tapgemm(dPre, Thd.t().contiguous(), None, (0,), ops.ACT_NONE, T, N)
    torch.cuda.synchronize()
    assert none is None and Gd.shape == (rows, K * c)
    _check(parity, {"y": _err(yd, y), "dPre": _err(dPre, w * (y.detach() > 0)), "dTheta": _err(dTh, Th.grad), "dZ": _err(Gd, Z.grad)})


#                 ci  co  taps        act           residual   tiles per wave (forward, data backward), chunks per split
SHARED_TAPFN = [(64, 64, (0,), ops.ACT_NONE, False, (2, 2, 2)),            # the block's 1x1 residual convolution
                (64, 64, (-1, 0, 1), ops.ACT_RELU, True, (2, 2, 4))]       # its time convolution, with R = the residual convolution's output


@pytest.mark.parametrize("ci,co,taps,act,with_res,plan", SHARED_TAPFN)
def test_block_convolutions_several_tiles_per_wave(ci, co, taps, act, with_res, plan, parity):
    """rows_hip.TapFn as astgcn_hip.forward calls it: y, dX, dW, db and — where the residual is a tensor of its own, which takes dPre — dR"""
    B, T, N = BTN
    rows, ktot = B * T * N, len(taps) * ci
    assert _shared_plan(co, ktot, act, ci, len(taps) * co, act != ops.ACT_NONE) == plan
    g = torch.Generator().manual_seed(ktot + co)
    x = torch.randn(rows, ci, generator=g, dtype=torch.float64).requires_grad_(True)
    W = (torch.randn(co, ktot, generator=g, dtype=torch.float64) / ktot ** 0.5).requires_grad_(True)
    b = (0.3 * torch.randn(co, generator=g, dtype=torch.float64)).requires_grad_(True)
    R = torch.randn(rows, co, generator=g, dtype=torch.float64).requires_grad_(True) if with_res else None
    w = torch.randn(rows, co, generator=g, dtype=torch.float64)
    pre = au.tap(x.view(B, T, N, ci), W, b, taps).view(rows, co)
    pre = pre + R if with_res else pre
    y = torch.relu(pre) if act == ops.ACT_RELU else pre
    (y * w).sum().backward()
    want = {"y": y, "dx": x.grad, "dW": W.grad, "db": b.grad}
    leaves = [t.detach().float().to(DEV).requires_grad_(True) for t in ((x, W, b, R) if with_res else (x, W, b))]
    xd, Wd, bd, Rd = leaves if with_res else leaves + [None]
    yd = TapFn.apply(xd, Wd, bd, Rd, taps, act, co if with_res else 0, T, N, True)
    (yd * w.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = {"y": yd, "dx": xd.grad, "dW": Wd.grad, "db": bd.grad}
    if with_res:
        want["dR"], got["dR"] = R.grad, Rd.grad
    _check(parity, {k: _err(got[k], want[k]) for k in want})


# ---- 2. the whole model ----------------------------------------------------------------------------------------------------------------------
def _ap(N, K=3, **kw):
    return au.model_args(N, graph.astgcn_graph(au.nonsymmetric_adjacency(N), K), K=K, **kw)


def _pair(N, K=3, dim_in=64, dim_out=1, seed=5, ap=None, **kw):
    """(fp64 torch module on the CPU, its fp32 copy on the GPU with backend hip), with the parameter set of the golden vectors — and U1 scaled
    down beyond 64 nodes, where that set saturates the first temporal sigmoid"""
    torch.manual_seed(seed)
    m64 = ASTGCN(_ap(N, K, **kw) if ap is None else ap, "cpu", dim_in, dim_out)
    au.xavier_pass_(m64)
    au.move_score_vectors_(m64)
    au.scale_u1_(m64, N)
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


#                N  K
WHOLE_MODEL = [(20, 3), (70, 3),
               (320, 3),                 # one sample of the most nodes the mix serves: all of a CU's LDS
               (305, 3),                 # the same 20 node tiles, the last with one real node
               (37, 2), (37, 3)]         # filter widths that are no multiple of 64 (below), from the 64-wide embedding
WHOLE_MODEL_WIDTH = {(37, 2): 48, (37, 3): 112}


@pytest.mark.parametrize("N,K", WHOLE_MODEL)
def test_whole_model_against_fp64_torch(N, K, parity):
    _whole_model(_pair(N, K, width=WHOLE_MODEL_WIDTH.get((N, K), 64)), N, 1 if N >= 305 else 2, 1, parity)


@pytest.mark.parametrize("ds", ["PEMS08", "METR_LA", "NYC_BIKE", "NYC_TAXI"])
def test_shipped_astgcn_configuration_against_fp64_torch(ds, parity):
    """the predictor as ``-mode eval -model ASTGCN`` builds it from the dataset's argument set (170, 207, 250 and 266 nodes, K = 3, two blocks
    of 64 filters; the output width is the dataset's) over a non-symmetric graph, one batch element of the 64-wide embedding: every mix of these
    models asks for more than the 64 KB of LDS a launch gets by default"""
    pa = predictor_args(ds, "ASTGCN")
    N, dim_out = pa.num_nodes, make_args(ds).output_dim
    assert (N, dim_out) == {"PEMS08": (170, 1), "METR_LA": (207, 1), "NYC_BIKE": (250, 2), "NYC_TAXI": (266, 2)}[ds]
    assert _mix_lds(rows_hip.pad16(N), pa.K) > 64 * 1024 and pa.len_input == 12
    ap = SimpleNamespace(**dict(vars(pa), G=graph.astgcn_graph(au.nonsymmetric_adjacency(N), pa.K)))
    _whole_model(_pair(N, pa.K, dim_out=dim_out, ap=ap), N, 1, dim_out, parity)


def _whole_model(pair, N, B, dim_out, parity):
    """y, dx and the 40 parameter gradients of one batch, with the condition on the reference's own sigmoid inputs that makes them mean something"""
    m64, mh = pair
    torch.manual_seed(N)
    x, w = torch.randn(B, 12, N, 64, dtype=torch.float64), torch.randn(B, 12, N, dim_out, dtype=torch.float64)
    zs = []
    with au.recorded_sigmoids(zs):
        want = _run(m64, x, w)
    au.assert_condition(zs, {k: v for k, v in want.items() if k not in ("y", "dx")})
    got = _run(mh, x.float().to(DEV), w.float().to(DEV))
    K = m64.cheb.shape[0]                                                  # y, dx, final_conv's two, and per block K Thetas and 16 others: 42 at K = 3
    assert m64.backend_used == "torch" and mh.backend_used == "hip" and set(got) == set(want) and len(want) == 36 + 2 * K
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
