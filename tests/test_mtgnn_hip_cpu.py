"""``MTGNN(..., backend="hip")`` without a GPU: the switch, the fallback on CPU tensors, the command-line option, and the algebra the HIP path
rests on — the packed zero-filled inception weight, the M1 / M2 graph polynomials with both ``mlp``s as one GEMM, the skip accumulation with
the output_dim 2 broadcast, the repacked LayerNorm weights — restated in plain torch from the helpers of ``mtgnn_hip`` and compared with the
module in fp64."""
import types

import pytest
import torch
import torch.nn.functional as F

from gptst_amd.config import FINETUNE_DEFAULTS, make_args, parse_args
from gptst_amd.predictors import MTGNN, mtgnn_hip as H

CFG = dict(num_nodes=20, input_window=12, output_window=12, gcn_true=True, buildA_true=True, gcn_depth=2, dropout=0.3,
           subgraph_size=8, node_dim=40, dilation_exponential=1, conv_channels=16, residual_channels=16, skip_channels=32, end_channels=32,
           layers=3, propalpha=0.05, tanhalpha=3, layer_norm_affline=True, use_curriculum_learning=True, task_level=0, adj_mx=None)
DIM_IN = 16


def _model(backend="torch", out=2, **kw):
    return MTGNN(types.SimpleNamespace(output_dim=out, **{**CFG, **kw}), "cpu", DIM_IN, out, backend=backend)


def test_backend_switch_and_fallback_on_cpu_tensors():
    torch.manual_seed(0)
    mh, mt = _model("hip"), _model()
    mt.load_state_dict(mh.state_dict(), strict=True)
    assert (mh.backend, mh.backend_used, mt.backend) == ("hip", None, "torch")
    x = torch.randn(2, 12, 20, DIM_IN)
    assert not H.supported(mh, x)
    torch.manual_seed(5)
    yh = mh(x)                                                          # training mode, dropout 0.3: the same stream, the same masks
    torch.manual_seed(5)
    yt = mt(x)
    assert mh.backend_used == "torch" and mt.backend_used == "torch" and torch.equal(yh, yt) and yh.requires_grad
    with pytest.raises(ValueError):
        _model("eager")


def test_mtgnn_backend_option():
    base = ["-dataset", "PEMS08", "-mode", "eval", "-model", "MTGNN"]
    a = parse_args("cpu", base)
    assert (a.mtgnn_backend, a.tgcn_backend, a.stgcn_backend, a.model) == ("torch", "torch", "torch", "MTGNN")
    a = parse_args("cpu", base + ["-mtgnn_backend", "hip"])
    assert (a.mtgnn_backend, a.tgcn_backend, a.stgcn_backend) == ("hip", "torch", "torch")
    assert make_args("PEMS08", mode="eval").mtgnn_backend == "torch" and FINETUNE_DEFAULTS["mtgnn_backend"] == "torch"
    with pytest.raises(SystemExit):
        parse_args("cpu", base + ["-mtgnn_backend", "eager"])


def _tapgemm(X, W, b, offs, B, Tsrc, Tdst, N):
    """rows (b, t, n): Y[b, to, n] = sum_j X[b, to + offs[j], n] W_j + b, W (co, len(offs) * ci) tap-major"""
    Xv = X.view(B, Tsrc, N, -1)
    cols = torch.cat([Xv[:, o:o + Tdst] for o in offs], -1)
    return cols.reshape(B * Tdst * N, -1) @ W.t() + b


def _restated(m, x, masks):
    """mtgnn_hip.forward in torch ops: the same packed weights, graphs and buffers, every kernel replaced by its definition"""
    B, T, N, Cin = x.shape
    Tt, S = m.total_window, m.skip_channels
    xr = F.pad(x, (0, 0, 0, 0, Tt - T, 0)).reshape(B * Tt * N, Cin)
    L5 = torch.cat([torch.eye(N, dtype=x.dtype)[None], H.mix_graphs(m.adjacency(), m.propalpha)])

    def conv(c, h, Tsrc):
        W, b, offs = H.time_weight(c)
        return _tapgemm(h, W, b, offs, B, Tsrc, Tsrc - len(offs) + 1, N)

    skip = conv(m.skip0, xr * masks["in"].reshape(xr.shape), Tt)
    h = conv(m.start_conv, xr, Tt)
    for i in range(m.layers):
        Tsrc, Tdst = m.frames[i], m.frames[i + 1]
        Wg, bg, offs = H.inception_weight(m.filter_convs[i], m.gate_convs[i])
        C = Wg.shape[0] // 2
        pre = _tapgemm(h, Wg, bg, offs, B, Tsrc, Tdst, N)
        g = torch.tanh(pre[:, :C]) * torch.sigmoid(pre[:, C:]) * masks["l%d" % i].reshape(-1, C)
        skip = conv(m.skip_convs[i], g, Tdst) + skip
        Z = torch.einsum("kvw,uwc->uvkc", L5, g.view(B * Tdst, N, C)).reshape(B * Tdst * N, 5 * C)
        Wm, bm = H.mix_weight(m.gconv1[i], m.gconv2[i])
        y = Z @ Wm.t() + bm + h.view(B, Tsrc, N, -1)[:, Tsrc - Tdst:].reshape(B * Tdst * N, -1)
        gamma, beta = H.norm_weight(m.norm[i], Tdst * N * y.shape[1], y)
        h = F.layer_norm(y.view(B, -1), (gamma.numel(),), gamma, beta, m.norm[i].eps).view_as(y)
    To = m.frames[-1] - m.skipE.kernel_size[1] + 1
    z = F.relu(conv(m.skipE, h, m.frames[-1]).view(B, To, N, S) + skip.view(B, 1, N, S)).view(B * To * N, S)
    e1, e2 = m.end_conv_1, m.end_conv_2
    z = F.relu(z @ e1.weight.view(e1.out_channels, -1).t() + e1.bias)
    return (z @ e2.weight.view(e2.out_channels, -1).t() + e2.bias).view(B, To, N, -1).permute(0, 3, 2, 1)


@pytest.mark.parametrize("out,dil", [(2, 1), (1, 1), (1, 2)])
def test_packing_algebra(out, dil):
    """output_dim 2: T = 20 -> 14 -> 8 -> 2 and the skip sum broadcasts; dilation_exponential 2 (two layers): dilated taps"""
    torch.manual_seed(1)
    m = _model(out=out, dilation_exponential=dil, layers=3 if dil == 1 else 2).double().train()
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.startswith("norm.") or k.endswith(".bias"):
                p.add_(0.2 * torch.randn_like(p))
    B, N = 2, 20
    x = torch.randn(B, 12, N, DIM_IN, dtype=torch.float64, requires_grad=True)
    w = torch.randn(B, 12, N, out, dtype=torch.float64)
    # one set of dropout multipliers in the rows' layout (B, T, N, C); the module's layout is (B, C, N, T)
    shapes = {"in": (B, m.total_window, N, DIM_IN), **{"l%d" % i: (B, m.frames[i + 1], N, 16) for i in range(m.layers)}}
    masks = {k: (torch.rand(s, dtype=torch.float64) > 0.3).double() / 0.7 for k, s in shapes.items()}
    m._keep = lambda tag, like: masks[tag].permute(0, 3, 2, 1)
    y = m(x)
    (y * w).sum().backward()
    want = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    want["dx"] = x.grad.clone()
    m.zero_grad()
    x.grad = None
    # the packed inception weight: 7 taps, zeros where a kernel has no tap, filter rows then gate rows
    Wg, bg, offs = H.inception_weight(m.filter_convs[0], m.gate_convs[0])
    W7 = Wg.view(32, 7, 16)
    assert offs == tuple(range(7)) and Wg.shape == (32, 7 * 16) and bg.shape == (32,)
    for half in (0, 16):
        for q, kern in enumerate((2, 3, 6, 7)):
            blk = W7[half + 4 * q:half + 4 * q + 4]
            assert bool((blk[:, :7 - kern] == 0).all()) and bool((blk[:, 7 - kern:] != 0).all())
    if dil == 2:
        assert H.inception_weight(m.filter_convs[1], m.gate_convs[1])[2] == (0, 2, 4, 6, 8, 10, 12)
    # M1, M2: h1 = M1 x, h2 = M2 x of a MixProp
    adp = m.adjacency().detach()
    L4 = H.mix_graphs(adp, m.propalpha)
    g = torch.randn(3, 16, N, 5, dtype=torch.float64)
    a = m.gconv1[0].normalised(adp)
    h1 = 0.05 * g + 0.95 * torch.einsum("ncwl,vw->ncvl", g, a)
    h2 = 0.05 * g + 0.95 * torch.einsum("ncwl,vw->ncvl", h1, a)
    assert float((torch.einsum("ncwl,vw->ncvl", g, L4[0]) - h1).abs().max()) < 1e-13
    assert float((torch.einsum("ncwl,vw->ncvl", g, L4[1]) - h2).abs().max()) < 1e-13
    assert float((L4[2] - (0.05 * torch.eye(N, dtype=torch.float64) + 0.95 * m.gconv1[0].normalised(adp.t()))).abs().max()) < 1e-15
    # the LayerNorm weights in the rows' order
    gamma, _ = H.norm_weight(m.norm[0], 0, None)
    T1 = m.frames[1]
    assert gamma.shape == (T1 * N * 16,) and torch.equal(gamma.view(T1, N, 16)[3, 7, 5], m.norm[0].weight[5, 7, 3])
    # the whole restated forward, and every gradient through the packing
    y2 = _restated(m, x, masks)
    assert y2.shape == y.shape == (B, 12, N, out)
    assert float((y2 - y).detach().abs().max()) < 1e-10 * float(y.detach().abs().max())
    (y2 * w).sum().backward()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    got["dx"] = x.grad
    assert set(got) == set(want) and not any(k.startswith("residual_convs.") for k in got)
    for k in want:
        assert float((got[k] - want[k]).abs().max()) <= 1e-10 * float(want[k].abs().max()), k
