"""predictors/msdr_hip.py without a GPU: every ``ops`` entry it calls is replaced by its formula in torch (the formulas tests/test_gpu_msdr_hip.py
holds the kernels to), and the module's HIP forward — the packing, the four recurrences with their hoisted halves, the hand-written backward
of ``_CellFn`` with its ring of state gradients — is held to autograd on the torch ops of the same module, in fp64 at 1e-9, for y, dx and every
parameter gradient: one and two fixed supports, a padded width, T < K (initial states still among the final ones), horizon < seq_len, one
layer, pre_k = 1.  ``attlinear.bias`` gets exactly 0 where autograd leaves rounding noise."""
import pytest
import torch
import torch.nn.functional as F

import msdr_util as gu
from gptst_amd import graph, ops
from gptst_amd.predictors import MSDR, msdr_hip as H

GROUPS = 3


def groups(N, B, tiles=0):
    return GROUPS


def nodemix(Lp, In, N, c, reduce, res=None):
    ks = Lp.shape[0]
    L = Lp[:, :N, :N]
    units = In.shape[0] // N
    if not reduce:
        x = In.view(units, N, c)
        return torch.cat([torch.matmul(L[k], x) for k in range(ks)], dim=-1).reshape(units * N, ks * c)
    x = In.view(units, N, ks, c)
    out = sum(torch.matmul(L[k], x[:, :, k]) for k in range(ks)).reshape(units * N, c)
    return out + res if res is not None else out


def tapgemm(X, W, bias, taps, act, T, N, res=None, res_w=0, keep=False):
    assert tuple(taps) == (0,) and act == 0 and res is None
    y = X @ W.t()
    return y + bias if bias is not None else y


def wgrad(D, X, taps, T, N, want_bias=True):
    return D.t() @ X, (D.sum(0) if want_bias else None)


def graphgrad(D, X, N, c, ks, dcol0=0):
    units = X.shape[0] // N
    out = []
    for k in range(ks):
        d = D[:, dcol0 + k * c: dcol0 + (k + 1) * c].reshape(units, N, c)
        out.append(torch.einsum("uvc,uwc->vw", d, X.view(units, N, c)))
    return torch.stack(out)


def fwd_step(Lp, Wh, W2, bvec, R, w, wr, Gx, Hs, sig, t, B, T, N, w2=None, sig2=None, c=None, z=None, a=None, tiles=0):
    K, Hp, ks = R.shape[0], Hs.shape[2], Lp.shape[0]
    L = Lp[:, :N, :N]
    e = sig[t:t + K].sum(-1).t() + wr
    att = torch.softmax(e, 1)
    h = Hs[t + K - 1]
    M = torch.cat([h] + [torch.matmul(L[k], h.view(B, N, Hp)).reshape(B * N, Hp) for k in range(ks)], 1)
    rows = slice(t * B * N, (t + 1) * B * N)
    cc = F.leaky_relu(M @ Wh.t() + Gx[rows])
    xs = Hs[t:t + K].view(K, B, N, Hp) + R[:, None]
    o = (cc @ W2.t()).view(B, N, Hp) + bvec + (att.t()[:, :, None, None] * xs).sum(0)
    Hs[t + K] = o.view(B * N, Hp)
    s = (o * w).sum((1, 2))
    sig[t + K] = s[:, None] / GROUPS
    if sig2 is not None:
        sig2[t + K] = (o * w2).sum((1, 2))[:, None] / GROUPS
    if c is not None:
        c[rows] = cc
    if z is not None:
        z[rows] = M
    if a is not None:
        a[t] = att


def bwd_pre(W, R, Hs, dH, c, dpre, pa, t, B, T, N, tiles=0):
    K, Hp = R.shape[0], Hs.shape[2]
    rows = slice(t * B * N, (t + 1) * B * N)
    dO = dH[K + t]
    dpre[rows] = (dO @ W.t()) * torch.where(c[rows] > 0, 1.0, 0.01)
    xs = Hs[t:t + K].view(K, B, N, Hp) + R[:, None]
    dA = (dO.view(1, B, N, Hp) * xs).sum((2, 3)).t()
    pa.zero_()
    pa[:, 0, :K] = dA


def bwd_state(LpT, WhT, w, a, pa, dpre, dH, de, t, B, T, N, tiles=0):
    K, Hp, ks = a.shape[2], dH.shape[2], LpT.shape[0]
    LT = LpT[:, :N, :N]
    rows = slice(t * B * N, (t + 1) * B * N)
    dA = pa[:, :, :K].sum(1)
    d = a[t] * (dA - (a[t] * dA).sum(1, keepdim=True))
    de[t] = d
    dp = dpre[rows]
    M = torch.cat([dp] + [torch.matmul(LT[k], dp.view(B, N, Hp)).reshape(B * N, Hp) for k in range(ks)], 1)
    dh = M @ WhT.t()
    dO = dH[K + t].view(B, N, Hp).clone()
    for k in range(K):
        dH[t + k] += (a[t][:, k, None, None] * dO + d[:, k, None, None] * w).view(B * N, Hp)
    dH[t + K - 1] += dh


@pytest.fixture
def stand_ins(monkeypatch):
    for name, fn in (("msdr_groups", groups), ("stgcn_nodemix", nodemix), ("stgcn_tapgemm", tapgemm), ("stgcn_wgrad", wgrad),
                     ("mtgnn_graphgrad", graphgrad), ("msdr_fwd_step", fwd_step), ("msdr_bwd_pre", bwd_pre), ("msdr_bwd_state", bwd_state)):
        monkeypatch.setattr(ops, name, fn)

    class Tap:                                                                 # rows_hip.TapFn: y = x W^T + b, autograd's own backward
        @staticmethod
        def apply(x, W, b, res, taps, act, res_w, T, N, keep):
            return x @ W.t() + b
    monkeypatch.setattr(H, "TapFn", Tap)


CASES = [(2, 5, 3, 7, 16, 12, 2, 2, 3, "dual_random_walk"), (2, 2, 2, 6, 16, 16, 1, 2, 4, "2000"), (1, 4, 4, 9, 32, 20, 1, 1, 1, "random_walk")]


@pytest.mark.parametrize("B,T,P,N,C,d,out,layers,K,ft", CASES)
def test_hip_forward_and_backward_equal_autograd_on_the_torch_ops(B, T, P, N, C, d, out, layers, K, ft, stand_ins):
    torch.manual_seed(0)
    ap = gu.model_args(N, graph.msdr_supports(gu.adjacency(N), ft), T=T, horizon=P, d=d, layers=layers, K=K, out=out)
    m = gu.perturb_(MSDR(ap, "cpu", C)).double().train()
    x, w = torch.randn(B, T, N, C, dtype=torch.float64), torch.randn(B, P, N, out, dtype=torch.float64)

    def run(fn):
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        y = fn(xi)
        (y * w).sum().backward()
        return y.detach(), xi.grad, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    ref, got = run(m), run(lambda xi: H.forward(m, xi, keep=True))
    err = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))      # noqa: E731
    assert err(got[0], ref[0]) < 1e-9 and err(got[1], ref[1]) < 1e-9 and set(got[2]) == set(ref[2]) and len(ref[2]) == 4 + 18 * layers
    for k, g in ref[2].items():
        if K == 1 and "attlinear" in k:                                       # one kept state: its weight is 1 whatever the logit
            assert not bool(g.any()) and float(got[2][k].abs().max()) < 1e-12, k
        elif k.endswith("attlinear.bias"):
            assert not bool(got[2][k].any()) and float(g.abs().max()) < 1e-9 * float(ref[2][k[:-4] + "weight"].abs().max()), k
        else:
            assert float(g.abs().max()) > 0 and err(got[2][k], g) < 1e-9, k
    with torch.no_grad():
        assert err(H.forward(m, x, keep=False), ref[0]) < 1e-9                # nothing kept: the same values


def test_pack_pads_with_zeros_and_places_theta_by_matrix():
    torch.manual_seed(1)
    m = MSDR(gu.model_args(6, graph.msdr_supports(gu.adjacency(6), "2000"), T=2, horizon=2, d=20), "cpu", 16)
    cell = m.cells()[0]
    Px, Ph, beta, W2, b, R, w = H.pack(cell, 20, 32, 3)
    assert Px.shape == Ph.shape == (32, 96) and beta.shape == (32,) and W2.shape == (32, 32) and b.shape == w.shape == (6, 32) and R.shape == (4, 6, 32)
    th = cell.theta                                                            # row = channel * 3 + matrix; channels [0, 20) the input, [20, 40) the state
    assert float(Px[5, 1 * 32 + 7].detach()) == float(th[7 * 3 + 1, 5].detach()) and float(Ph[5, 2 * 32 + 7].detach()) == float(th[(20 + 7) * 3 + 2, 5].detach())
    for t in (Px.view(32, 3, 32)[20:], Px.view(32, 3, 32)[:, :, 20:], Ph.view(32, 3, 32)[20:], Ph.view(32, 3, 32)[:, :, 20:], beta[20:], W2[20:], W2[:, 20:],
              b[:, 20:], R[..., 20:], w[:, 20:]):
        assert not bool(t.any())
    assert torch.equal(W2[:20, :20], cell.W.t()) and torch.equal(beta[:20], torch.ones(20))
