"""predictors/windows_hip.py — the layer function the STSGCN and STFGNN predictors share on HIP — without a GPU: the real ``LayerFn`` (and
STFGNN's ``_GateFn``, and ``rows_hip.TapFn`` in front of them) with every ``ops`` entry they call replaced by its definition in fp64 torch, in
the row layouts the launches use.  The stand-ins are built from the block algebra of stsgcn_util / stfgnn_util, which test_stsgcn_hip_cpu.py and
test_stfgnn_hip_cpu.py hold to the modules and test_gpu_stsgcn_hip.py / test_gpu_stfgnn_hip.py hold the kernels to.

1. ``STSGCN(..., backend="hip")`` and ``STFGNN(..., backend="hip")`` on the stand-ins equal the torch backend of the same state dict under
   autograd at 1e-9: the output, dx and every parameter gradient, with no element ambiguous under GAP (asserted).  STSGCN "individual" and
   "sharing" (one weight for all windows: the windows' gradients are summed), STFGNN with one window and with two layers.
2. Where the layer's input needs no gradient, the backward stops before operation 0's mirrored GEMM and adjoint mix.
3. With the stacked weights frozen no weight gradient is formed and dx is bit-equal.
4. Under no_grad and in eval mode nothing is kept: no grad_fn, no winner index allocated."""
import pytest
import torch

import stfgnn_util as fu
import stsgcn_util as su
from gptst_amd import ops
from gptst_amd.ops import ACT_GLU, ACT_NONE, ACT_RELU
from gptst_amd.predictors import STFGNN, STSGCN, stfgnn_hip, stsgcn_hip

TOL = 1e-9
C = 16


def _rel(got, ref):
    got, ref = got.detach(), ref.detach()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# ---- the launches in fp64 torch, rows in and rows out ----------------------------------------------------------------------------------
def _mix(span, algebra, graphs, In, mode, B, T, N):
    """algebra: (f2e, expanded, middle, m2e, e2f) of stsgcn_util or stfgnn_util over the graphs' (N, N) corners"""
    f2e, expanded, middle, m2e, e2f = algebra
    W, c = T - span + 1, In.shape[1]
    g = [p[:N, :N] for p in graphs]
    if mode == ops.MIX_F2E:
        out = f2e(*g, In.view(B, T, N, c))
    elif mode == ops.MIX_E2E:
        out = expanded(*g, In.view(B, W, span, N, c))
    elif mode == ops.MIX_E2M:
        out = middle(g[0], In.view(B, W, span, N, c))
    elif mode == ops.MIX_M2E:
        out = m2e(g[0], In.view(B, W, N, c))
    else:
        assert mode == ops.MIX_E2F
        out = e2f(*g, In.view(B, W, span, N, c))
    return out.reshape(-1, c)


def _stsgcn_mix(Lp, In, mode, B, T, N):
    return _mix(3, (su.mix_f2e, su.mix_expanded, su.mix_middle, su.mix_m2e, su.mix_e2f), (Lp,), In, mode, B, T, N)


def _stfgnn_mix(Sp, Dp, In, mode, B, T, N):
    return _mix(4, (fu.mix_f2e, fu.mix_expanded, fu.mix_middle, fu.mix_m2e, fu.mix_e2f), (Sp, Dp), In, mode, B, T, N)


def _mid(R, N):
    return slice(0, N) if R == N else slice(N, 2 * N)


def _wingemm(X, Wt, bias, act, B, W, R, N, keep=False, best=None, which=None, opj=0):
    assert Wt.shape[0] in (1, W) and Wt.is_contiguous() and (bias is None or bias.shape == Wt.shape[:2])
    pre = X.view(B, W, R, -1) @ Wt.transpose(1, 2)                        # (W | 1, ci, cw) against (B, W, R, ci)
    if bias is not None:
        pre = pre + bias[:, None, :]
    if act == ACT_NONE:
        assert not keep and best is None and which is None
        return pre.reshape(B * W * R, -1)
    assert act == ACT_GLU
    co = pre.shape[-1] // 2
    A, S = pre[..., :co], torch.sigmoid(pre[..., co:])
    Y = A * S
    if best is not None:                                                   # in place: operation 0 writes, later ones replace on strictly greater
        mid, bv = Y[:, :, _mid(R, N)], best.view(B, W, N, co)
        win = torch.ones_like(mid, dtype=torch.bool) if opj == 0 else mid > bv
        bv[win] = mid[win]
        if which is not None:
            assert which.dtype == torch.int32 and which.shape == best.shape
            which.view(B, W, N, co)[win] = opj
    flat = lambda t: t.reshape(B * W * R, co).contiguous()                 # noqa: E731
    return (flat(Y), flat(S), flat(A)) if keep else flat(Y)


def _gate_bwd(up, dBest, which, opj, S, A, B, W, R, N):
    co = S.shape[1]
    g = (torch.zeros_like(S) if up is None else up.clone()).view(B, W, R, co)
    g[:, :, _mid(R, N)] += dBest.view(B, W, N, co) * (which.view(B, W, N, co) == opj)
    g = g.view(B * W * R, co)
    return torch.cat([g * S, g * A * S * (1 - S)], 1)


def _winwgrad(D, X, B, W, R):
    Dv = D.view(B, W, R, -1)
    return torch.einsum("bwro,bwri->woi", Dv, X.view(B, W, R, -1)), Dv.sum((0, 2))


def _tapgemm(X, W, bias, taps, act, T, N, res=None, res_w=0, keep=False):
    assert tuple(taps) == (0,) and act in (ACT_NONE, ACT_RELU) and res is None and not keep
    y = X @ W.t()
    y = y + bias if bias is not None else y
    return torch.relu(y) if act == ACT_RELU else y


def _relu_bwd(dOut, act, out=None, S=None, A=None):
    assert act == ACT_RELU
    return dOut * (out > 0)


def _wgrad(D, X, taps, T, N, want_bias=True):
    return D.t() @ X, (D.sum(0) if want_bias else None)


def _shifted(X, off, B, Tsrc, Tdst, N):
    """(B, Tdst, N, ci): frame to + off of X (B Tsrc N, ci), zero where there is none"""
    Xv, out = X.view(B, Tsrc, N, -1), X.new_zeros(B, Tdst, N, X.shape[1])
    lo, hi = max(0, -off), min(Tdst, Tsrc - off)
    out[:, lo:hi] = Xv[:, lo + off:hi + off]
    return out


def _gated_tapgemm(X, W, bias, offs, B, Tsrc, Tdst, N, gated=False, keep=False):
    pre = torch.cat([_shifted(X, o, B, Tsrc, Tdst, N) for o in offs], -1).view(B * Tdst * N, -1) @ W.t()
    pre = pre + bias if bias is not None else pre
    if not gated:
        assert not keep
        return pre
    co = pre.shape[1] // 2
    tn, s = torch.tanh(pre[:, :co]), torch.sigmoid(pre[:, co:])
    return (tn * s, tn, s) if keep else tn * s


def _gated_bwd(dG, Tn, S):
    return torch.cat([dG * S * (1 - Tn * Tn), dG * Tn * S * (1 - S)], 1)


def _gated_wgrad(D, X, offs, B, Tsrc, Tdst, N):
    return D.t() @ torch.cat([_shifted(X, o, B, Tsrc, Tdst, N) for o in offs], -1).view(B * Tdst * N, -1), D.sum(0)


STAND_INS = {"stsgcn_mix": _stsgcn_mix, "stfgnn_mix": _stfgnn_mix, "stsgcn_wingemm": _wingemm, "stsgcn_gate_bwd": _gate_bwd,
             "stsgcn_winwgrad": _winwgrad, "stgcn_tapgemm": _tapgemm, "stgcn_gate_bwd": _relu_bwd, "stgcn_wgrad": _wgrad,
             "mtgnn_tapgemm": _gated_tapgemm, "mtgnn_gate_bwd": _gated_bwd, "mtgnn_wgrad": _gated_wgrad}


class Calls(list):
    """the names of the ``ops`` entries called, in order; ``which``: per GLU wingemm call, whether a winner index was handed in"""

    def __init__(self):
        super().__init__()
        self.which = []


@pytest.fixture
def stand_ins(monkeypatch):
    calls = Calls()

    def rec(name, fn):
        def f(*a, **k):
            calls.append(name)
            if name == "stsgcn_wingemm" and "best" in k:
                calls.which.append(k["which"] is not None)
            return fn(*a, **k)
        return f
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, rec(name, fn))
    for mod in (stsgcn_hip, stfgnn_hip):
        monkeypatch.setattr(mod, "supported", lambda model, x: True)
        monkeypatch.setattr(mod._C, "lib", lambda: None)
    return calls


# ---- the two predictors ----------------------------------------------------------------------------------------------------------------
def _stsgcn(backend, N, T, layers, module_type="individual"):
    return STSGCN(su.model_args(N, T=T, P=2, width=C, layers=layers, module_type=module_type), "cpu", C, 2, backend=backend)


def _stfgnn(backend, N, T, layers):
    return STFGNN(fu.model_args(N, T=T, P=2, width=C, layers=layers), "cpu", C, backend=backend)


def _pair(make, util, seed, *cfg):
    torch.manual_seed(seed)
    a = make("hip", *cfg)
    util.randomize_embeddings_(a)
    a = a.double().train()
    b = make("torch", *cfg).double().train()
    b.load_state_dict(a.state_dict(), strict=True)
    return a, b


def _layers(m):
    return [lay.layer for lay in m.stsgcl_layers] if isinstance(m, STSGCN) else list(m.STSGCLS)


CASES = [("stsgcn individual T5 L1", _stsgcn, su, 4, (7, 5, 1)),
         ("stsgcn individual T6 L2", _stsgcn, su, 4, (9, 6, 2)),
         ("stsgcn sharing T6 L2", _stsgcn, su, 4, (5, 6, 2, "sharing")),
         ("stfgnn T4 L1", _stfgnn, fu, 4, (6, 4, 1)),
         ("stfgnn T7 L2", _stfgnn, fu, 4, (8, 7, 2))]


@pytest.mark.parametrize("name,make,util,seed,cfg", CASES, ids=[c[0] for c in CASES])
def test_hip_module_on_stand_ins_equals_autograd(stand_ins, name, make, util, seed, cfg):
    a, b = _pair(make, util, seed, *cfg)
    N, T, L = cfg[:3]
    x = torch.randn(2, T, N, C, dtype=torch.float64)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    cands = []
    with util.recorded_candidates(b, cands):
        yb = b(xb)
    assert len(cands) == L and all(su.ambiguous(c) == (0, c[0].numel()) for c in cands)           # no winner that rounding could change
    ya = a(xa)
    assert (a.backend_used, b.backend_used) == ("hip", "torch") and _rel(ya, yb) < TOL
    w = torch.randn_like(yb)
    (ya * w).sum().backward()
    (yb * w).sum().backward()
    span, gate = (3, 0) if make is _stsgcn else (4, 1)
    # per layer of three operations: 3 mixes and 3 GEMMs forward; 3 gate backwards, 3 weight gradients, 3 mirrored GEMMs, 3 adjoint mixes
    mix = "stsgcn_mix" if make is _stsgcn else "stfgnn_mix"
    assert [stand_ins.count(k) for k in (mix, "stsgcn_wingemm", "stsgcn_gate_bwd", "stsgcn_winwgrad")] == [6 * L, 6 * L, 3 * L, 3 * L]
    assert stand_ins.count("mtgnn_tapgemm") == 2 * L * gate and stand_ins.which == [True] * (3 * L)
    assert _rel(xa.grad, xb.grad) < TOL
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    assert set(ga) == set(gb)
    for k in ga:
        assert ga[k].grad.shape == gb[k].grad.shape and float(gb[k].grad.abs().max()) > 0 and _rel(ga[k].grad, gb[k].grad) < TOL, k
    if "sharing" in name:                                                  # the summed-windows branch ran: one weight, four and two windows
        assert [tuple(t.shape) for t in _layers(a)[0].stacked(0)] == [(1, 2 * C, C), (1, 2 * C)] and T - span + 1 == 4


SMALL = [("stsgcn", _stsgcn, su, (7, 5, 1)), ("stfgnn", _stfgnn, fu, (6, 5, 1))]


def _freeze(ps):
    for p in ps:
        p.requires_grad_(False)
        p.grad = None


@pytest.mark.parametrize("name,make,util,cfg", SMALL, ids=[c[0] for c in SMALL])
def test_backward_stops_where_the_layer_input_needs_no_gradient(stand_ins, name, make, util, cfg):
    a, _ = _pair(make, util, 3, *cfg)
    mix = name + "_mix"
    x = torch.randn(2, cfg[1], cfg[0], C, dtype=torch.float64)
    a(x).square().sum().backward()                                         # the layer's input carries the first embedding's gradient
    full = [stand_ins.count(k) for k in (mix, "stsgcn_wingemm", "stsgcn_gate_bwd", "stsgcn_winwgrad", "mtgnn_tapgemm")]
    del stand_ins[:]
    lay = _layers(a)[0]
    emb = list(lay.position_embedding.parameters()) if make is _stsgcn else [lay.temporal_embedding, lay.spatial_embedding]
    _freeze(list((a.first_layer_embedding if make is _stsgcn else a.First_FC).parameters()) + emb)
    a(x).square().sum().backward()
    cut = [stand_ins.count(k) for k in (mix, "stsgcn_wingemm", "stsgcn_gate_bwd", "stsgcn_winwgrad", "mtgnn_tapgemm")]
    gate = int(make is _stfgnn)
    assert full == [6, 6, 3, 3, 2 * gate] and cut == [5, 5, 3, 3, gate]
    tail = stand_ins[len(stand_ins) - 1 - stand_ins[::-1].index("stsgcn_winwgrad"):]            # operation 0 ends at its weight gradient
    assert mix not in tail and "stsgcn_wingemm" not in tail
    assert all(p.grad is not None for p in a.parameters() if p.requires_grad) and lay.stacked(0)[0].requires_grad


@pytest.mark.parametrize("name,make,util,cfg", SMALL, ids=[c[0] for c in SMALL])
def test_frozen_stacked_weights_form_no_weight_gradient_and_dx_is_bit_equal(stand_ins, name, make, util, cfg):
    a, _ = _pair(make, util, 3, *cfg)
    x = torch.randn(2, cfg[1], cfg[0], C, dtype=torch.float64)
    x1 = x.clone().requires_grad_(True)
    a(x1).square().sum().backward()
    n_full = stand_ins.count("stsgcn_winwgrad")
    del stand_ins[:]
    lay = _layers(a)[0]
    ops_ = [m.layers for m in lay.gcms] if make is _stsgcn else [m.gcn_operations for m in lay.STSGCMS]
    _freeze([p for window in ops_ for op in window for p in op.parameters()])
    x2 = x.clone().requires_grad_(True)
    a(x2).square().sum().backward()
    assert n_full == 3 and stand_ins.count("stsgcn_winwgrad") == 0 and stand_ins.count("stsgcn_gate_bwd") == 3
    assert torch.equal(x1.grad, x2.grad) and all(t.grad is None and not t.requires_grad for j in range(3) for t in lay.stacked(j))
    assert (a.first_layer_embedding if make is _stsgcn else a.First_FC).weight.grad is not None


@pytest.mark.parametrize("name,make,util,cfg", SMALL, ids=[c[0] for c in SMALL])
def test_no_grad_and_eval_keep_nothing(stand_ins, name, make, util, cfg):
    a, b = _pair(make, util, 3, *cfg)
    x = torch.randn(2, cfg[1], cfg[0], C, dtype=torch.float64)
    with torch.no_grad():
        y = a(x)
    assert y.grad_fn is None and _rel(y, b(x)) < TOL
    y = a.eval()(x.clone().requires_grad_(True))
    assert y.grad_fn is None and a.backend_used == "hip"
    assert stand_ins.which == [False] * 6 and not any("bwd" in k or "wgrad" in k for k in stand_ins)
