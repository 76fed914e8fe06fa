"""``ASTGCN(..., backend="hip")`` without a GPU: the switch and the fallback on CPU tensors, the command-line option, the predictor's argument
set for the four datasets, the xavier pass of the eval wiring, and the algebra the HIP path rests on — the score chains without x_TAt, the masked
mix as one contraction, the packed Theta, the tap form of the two convolutions — restated in plain torch from the helpers of ``astgcn_hip`` and
compared with the module in fp64."""
import pytest
import torch
import torch.nn.functional as F

import astgcn_util as au
from gptst_amd.config import FINETUNE_DEFAULTS, apply_predictor_overrides, make_args, parse_args, predictor_args
from gptst_amd.predictors import ASTGCN, astgcn_hip as H


def _model(n=20, backend="torch", out=1, dim_in=32, seed=0, **kw):
    torch.manual_seed(seed)
    G = torch.randn(kw.get("K", 3), n, n) * 0.3                         # non-symmetric "polynomials": the algebra does not need real ones
    m = ASTGCN(au.model_args(n, G, **kw), "cpu", dim_in, out, backend=backend)
    au.xavier_pass_(m)
    au.move_score_vectors_(m)
    return m


def test_backend_switch_and_fallback_on_cpu_tensors():
    mh, mt = _model(backend="hip"), _model()
    mt.load_state_dict(mh.state_dict(), strict=True)
    assert (mh.backend, mh.backend_used, mt.backend) == ("hip", None, "torch")
    x = torch.randn(2, 12, 20, 32)
    assert not H.supported(mh, x)
    yh, yt = mh(x), mt(x)
    assert mh.backend_used == "torch" and mt.backend_used == "torch" and torch.equal(yh, yt) and yh.requires_grad


def test_astgcn_backend_option():
    base = ["-dataset", "PEMS08", "-mode", "eval", "-model", "ASTGCN"]
    a = parse_args("cpu", base)
    assert (a.astgcn_backend, a.mtgnn_backend, a.tgcn_backend, a.stgcn_backend, a.model) == ("torch", "torch", "torch", "torch", "ASTGCN")
    a = parse_args("cpu", base + ["-astgcn_backend", "hip"])
    assert (a.astgcn_backend, a.mtgnn_backend, a.tgcn_backend, a.stgcn_backend) == ("hip", "torch", "torch", "torch")
    assert make_args("PEMS08", mode="eval").astgcn_backend == "torch" and FINETUNE_DEFAULTS["astgcn_backend"] == "torch"
    with pytest.raises(SystemExit):
        parse_args("cpu", base + ["-astgcn_backend", "eager"])


@pytest.mark.parametrize("ds,nodes,seed", [("PEMS08", 170, 12), ("METR_LA", 207, 0), ("NYC_BIKE", 250, 12), ("NYC_TAXI", 266, 52)])
def test_predictor_args_restate_the_reference_confs(ds, nodes, seed):
    p = predictor_args(ds, "ASTGCN")
    assert (p.num_nodes, p.len_input, p.num_for_predict, p.nb_block, p.K, p.nb_chev_filter, p.nb_time_filter, p.time_strides) == \
        (nodes, 12, 12, 2, 3, 64, 64, 1)
    assert (p.seed, p.seed_mode, p.xavier, p.loss_func) == (seed, True, True, "mask_mae")
    assert predictor_args(ds, "ASTGCN", ["--K", "2"]).K == 2
    a = apply_predictor_overrides(make_args(ds, mode="eval"), p)
    assert a.xavier is True and a.seed == seed and a.epochs == 100
    with pytest.raises(ValueError):
        predictor_args(ds, "GWN")


def _attmix(Tk, S, x4):
    """the definition of ops.astgcn_attmix (expand): Z[b,t,n,k,ch] = sum_m T_k[m,n] S[b,m,n] x[b,t,m,ch]"""
    return torch.einsum("kmn,bmn,btmc->btnkc", Tk, S, x4)


_tap = au.tap


def _restated(m, x):
    """astgcn_hip.forward in torch ops: the same helpers and packed weights, every kernel replaced by its definition"""
    B, T, N, _ = x.shape
    h = x
    for blk in m.BlockList:
        S = H.attention(blk, h)
        Z = _attmix(m.cheb, S, h).reshape(B, T, N, -1)
        g = F.relu(_tap(Z, H.pack_theta(blk), None, (0,)))
        rc = blk.residual_conv
        R = _tap(h, rc.weight.view(rc.out_channels, rc.in_channels), rc.bias, (0,))
        y = F.relu(_tap(g, H.pack_time_conv(blk), blk.time_conv.bias, (-1, 0, 1)) + R)
        h = F.layer_norm(y, (y.shape[-1],), blk.ln.weight, blk.ln.bias, blk.ln.eps)
    return H.head(m, h)


@pytest.mark.parametrize("n,K,out", [(20, 3, 1), (13, 2, 2)])
def test_hip_path_algebra_equals_the_module(n, K, out):
    m = _model(n=n, out=out, K=K, seed=3).double().train()
    with torch.no_grad():
        for k, p in m.named_parameters():
            if ".ln." in k or k.endswith(".bias"):
                p.add_(0.2 * torch.randn_like(p))
    x = torch.randn(2, 12, n, 32, dtype=torch.float64, requires_grad=True)
    w = torch.randn(2, 12, n, out, dtype=torch.float64)
    zs = []
    with au.recorded_sigmoids(zs):
        y = m(x)
    (y * w).sum().backward()
    want = {k: p.grad.clone() for k, p in m.named_parameters()}
    au.assert_condition(zs, want)
    want["dx"] = x.grad.clone()
    m.zero_grad()
    x.grad = None
    # the packed weights: Theta stacks theta_k as column blocks, the time conv is tap-major
    blk = m.BlockList[0]
    Th, Wt = H.pack_theta(blk), H.pack_time_conv(blk)
    assert Th.shape == (64, K * 32) and torch.equal(Th[5, 32 + 7], blk.cheb_conv_SAt.Theta[1][7, 5])
    assert Wt.shape == (64, 3 * 64) and torch.equal(Wt[5, 2 * 64 + 9], blk.time_conv.weight[5, 9, 0, 2])
    # the attention without x_TAt equals the modules'
    xr = x.detach().permute(0, 2, 3, 1)
    e = blk.TAt(xr)
    s_mod = blk.SAt(torch.matmul(xr.reshape(2, -1, 12), e).reshape(xr.shape))
    assert float((H.attention(blk, x.detach()) - s_mod).detach().abs().max()) < 1e-12
    # the whole restated forward, and every gradient through the packing, back in the reference's layout
    y2 = _restated(m, x)
    assert y2.shape == y.shape == (2, 12, n, out)
    assert float((y2 - y).detach().abs().max()) < 1e-10 * float(y.detach().abs().max())
    (y2 * w).sum().backward()
    got = {k: p.grad for k, p in m.named_parameters()}
    got["dx"] = x.grad
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and float((got[k] - want[k]).abs().max()) <= 1e-10 * float(want[k].abs().max()), k


def test_padded_graph_and_supported():
    m = _model(n=20, backend="hip")
    tp = H.padded_graph(m)
    assert tp.shape == (3, 32, 32) and torch.equal(tp[:, :20, :20], m.cheb) and float(tp[:, 20:].abs().max()) == 0 and float(tp[:, :, 20:].abs().max()) == 0
    assert H.padded_graph(m) is tp
    m.cheb.mul_(2)
    assert H.padded_graph(m) is not tp
    x = torch.randn(2, 12, 20, 32)
    assert not H.supported(m, x)                                        # a CPU tensor


@pytest.mark.parametrize("finetune", [False, True])
def test_xavier_pass_of_the_eval_wiring_leaves_the_encoder_alone(finetune):
    from gptst_amd.enhance import EnhanceFrontEnd, xavier_downstream_
    args = make_args("PEMS08", mode="eval", num_nodes=8)
    torch.manual_seed(0)
    pred = ASTGCN(au.model_args(8, torch.randn(3, 8, 8)), "cpu", args.hidden_dim, args.output_dim)
    with torch.no_grad():
        for p in pred.parameters():
            p.fill_(7.0)                                                # uninitialised memory otherwise: give "untouched" a meaning
    model = EnhanceFrontEnd(args, predictor=pred, finetune_encoder=finetune)
    with torch.no_grad():
        for p in model.pretrain_model.parameters():                     # (some of the encoder's parameters are uninitialised memory until a load)
            p.uniform_(-1, 1)
    enc = {k: v.clone() for k, v in model.pretrain_model.state_dict().items()}
    assert any(p.requires_grad for p in model.pretrain_model.parameters()) == finetune
    before = {k: p.detach().clone() for k, p in model.named_parameters() if not k.startswith("pretrain_model.")}
    torch.manual_seed(1)
    xavier_downstream_(model)
    assert all(torch.equal(v, enc[k]) for k, v in model.pretrain_model.state_dict().items())
    after = dict(model.named_parameters())
    assert len(before) == 6 + 2 + 40 and all(not torch.equal(after[k], v) for k, v in before.items())
    # what the reference's pass draws, in named_parameters order
    torch.manual_seed(1)
    for k, v in before.items():
        want = torch.empty_like(v)
        torch.nn.init.xavier_uniform_(want) if want.dim() > 1 else torch.nn.init.uniform_(want)
        assert torch.equal(after[k].detach(), want), k
