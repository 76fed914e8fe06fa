"""Fine-tuning the pretrained encoder downstream (``-mode eval -finetune_encoder True``) on the GPU: the gate's backward with the gradient of
the embedding (gptst_fusion_gate_bwd_df), the encoder's autograd node (model._EncoderFn) against the fp64 oracle, and the whole chain
encoder -> gate -> STGCN against the same computation in fp64 on the CPU, then a few optimiser steps through EvalTrainer."""
import functools
import logging
from types import SimpleNamespace

import pytest
import torch

from gptst_amd import synth
from gptst_amd.config import make_args
from oracle import gptst_oracle as O
from test_gpu_kernels import close          # 1e-4 of the tensor's scale (and element-wise): the gate test's own bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_TOL = 1e-4        # every parameter gradient, of its tensor's max (test_gpu_shapes.py)
FWD_TOL = 1e-5         # forward outputs (test_gpu_shapes.py)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _grad_sd(sd, dtype=torch.float64):
    """oracle state dict in `dtype`, every parameter a leaf that takes a gradient"""
    return {k: (v.to(dtype) if k.endswith("mask_template") else v.to(dtype).requires_grad_(True)) for k, v in sd.items()}


# ---- 1. the gate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,base", [((3, 12, 37), 2), ((1, 5, 7), 1), ((2, 12, 170), 1)])
def test_fusion_gate_returns_the_embedding_gradient(shape, base):
    """fusion_gate with an embedding that requires a gradient: output, dF and the eight parameter gradients against the torch Fusion + Linear
    modules in fp64 on the CPU; and gptst_fusion_gate_bwd_df's dpre, dxd, Hm, xt bit-identical to gptst_fusion_gate_bwd's."""
    from gptst_amd.enhance import Fusion
    from gptst_amd.fusion import fusion_gate
    from gptst_amd.ops import _call, _p
    torch.manual_seed(5)
    C = 64
    fus, lin = Fusion(C), torch.nn.Linear(base, C)
    F = torch.randn(*shape, C) * 0.7
    src = torch.randn(*shape, base + 2)
    go = torch.randn(*shape, C)
    fus64, lin64 = Fusion(C).double(), torch.nn.Linear(base, C).double()
    fus64.load_state_dict(fus.state_dict()); lin64.load_state_dict(lin.state_dict())
    F64 = F.double().requires_grad_(True)
    ref = fus64(F64, lin64(src.double()[..., :base]))
    (ref * go.double()).sum().backward()
    want = {n: p.grad for n, p in list(fus64.named_parameters()) + [("lin." + k, v) for k, v in lin64.named_parameters()]}
    fus_d, lin_d = fus.to(DEV), lin.to(DEV)
    Fd, sd_ = F.to(DEV).requires_grad_(True), src.to(DEV)
    out = fusion_gate(Fd, sd_, fus_d, lin_d, base)
    close(out, ref.detach(), what="fusion gate out")
    (out * go.to(DEV)).sum().backward()
    assert Fd.grad is not None
    close(Fd.grad, F64.grad, what="fusion gate dF")
    got = {n: p.grad for n, p in list(fus_d.named_parameters()) + [("lin." + k, v) for k, v in lin_d.named_parameters()]}
    assert len(want) == 8
    for n in want:
        close(got[n], want[n], what="fusion gate d" + n)
    # both C entries on the same inputs
    rows = F.numel() // C
    Fr, sr, dout = Fd.detach().view(rows, C), sd_.view(rows, base + 2), go.to(DEV).view(rows, C).contiguous()
    w = {k: v.detach().contiguous() for k, v in list(fus_d.named_parameters()) + [("lin." + k, v) for k, v in lin_d.named_parameters()]}
    z, o2 = torch.empty_like(Fr), torch.empty_like(Fr)
    _call("gptst_fusion_gate_fwd", _p(Fr), _p(sr), base + 2, base, _p(w["HS_fc.weight"]), _p(w["HS_fc.bias"]), _p(w["HT_fc.weight"]),
          _p(w["HT_fc.bias"]), _p(w["output_fc.weight"]), _p(w["output_fc.bias"]), _p(w["lin.weight"]), _p(w["lin.bias"]), _p(o2), _p(z), rows, C)
    a = [torch.full_like(Fr, float("nan")) for _ in range(4)]
    b = [torch.full_like(Fr, float("nan")) for _ in range(5)]
    _call("gptst_fusion_gate_bwd", _p(dout), _p(Fr), _p(z), _p(sr), base + 2, base, _p(w["output_fc.weight"]), _p(w["lin.weight"]), _p(w["lin.bias"]),
          *[_p(t) for t in a], rows, C)
    _call("gptst_fusion_gate_bwd_df", _p(dout), _p(Fr), _p(z), _p(sr), base + 2, base, _p(w["output_fc.weight"]), _p(w["lin.weight"]),
          _p(w["lin.bias"]), _p(w["HS_fc.weight"]), *[_p(t) for t in b], rows, C)
    for name, x, y in zip(("dpre", "dxd", "Hm", "xt"), a, b):
        assert torch.equal(x, y), name
    assert torch.equal(b[4], Fd.grad.view(rows, C))


def test_fusion_gate_bwd_df_refuses_other_widths():
    from gptst_amd import _C
    t = torch.zeros(16, 128, device=DEV)
    p = t.data_ptr()
    assert _C.lib().value("gptst_fusion_gate_bwd_df", p, p, p, p, 3, 1, p, p, p, p, p, p, p, p, p, 16, 128, None) == _C.ESHAPE
    assert _C.lib().value("gptst_fusion_gate_bwd_df", p, p, p, p, 7, 5, p, p, p, p, p, p, p, p, p, 16, 64, None) == _C.ESHAPE


# ---- 2. the encoder's node against the fp64 oracle ------------------------------------------------------------------------------------------
CASES = {
    "hs2": ("NYC_TAXI", dict(HS=2, num_nodes=61)),                                  # base 2
    "hs5": ("PEMS08", dict(HS=5, num_nodes=50)),
    "c128": ("PEMS08", dict(hidden_dim=128, num_nodes=40, embed_dim=8)),           # the encoder alone: the gate has no C = 128 path
}


def _encoder_case(name, B=2):
    ds, over = CASES[name]
    args = make_args(ds, mode="eval", scaler_zeros=synth.scaler_zeros(), **over)
    sd = O.init_state_dict(args, 11)
    src = synth.make_batch(B, 12, args.num_nodes, args.input_base_dim, interval=args.interval, seed=21)
    go = torch.randn(B, 12, args.num_nodes, args.hidden_dim, generator=torch.Generator().manual_seed(7))
    return args, sd, src, go


@functools.lru_cache(maxsize=None)
def _encoder_reference(name):
    """fp64 oracle: embedding and the gradients of (emb * go).sum() — computed once per case"""
    args, sd, src, go = _encoder_case(name)
    sd64 = _grad_sd(sd)
    emb = O.forward_eval(sd64, args, src.double())
    (emb * go.double()).sum().backward()
    return emb.detach(), {k: v.grad for k, v in sd64.items() if v.requires_grad}


def _finetune_model(args, sd):
    from gptst_amd.model import GPTST_Model
    model = GPTST_Model(args)
    model.load_state_dict(sd)
    model.finetune = True
    return model.to(DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_encoder_gradients_vs_fp64_oracle(name, parity):
    args, sd, src, go = _encoder_case(name)
    emb_r, grads_r = _encoder_reference(name)
    model = _finetune_model(args, sd)
    srcd = src.to(DEV)
    emb = model(srcd, None)[0]
    assert emb.requires_grad
    e = _rel(emb, emb_r)
    parity("fwd_emb", e)
    print(name, "embedding rel err %.2e" % e)
    model.finetune = False
    frozen = model(srcd, None)[0]
    model.finetune = True
    assert not frozen.requires_grad and torch.equal(emb.detach(), frozen)
    (emb * go.to(DEV)).sum().backward()
    errs, on_path = {}, 0
    for k, pm in model.named_parameters():
        gr = grads_r[k]
        if gr is None or float(gr.abs().max()) == 0.0:
            assert pm.grad is None or float(pm.grad.abs().max()) == 0.0, k
            continue
        on_path += 1
        assert pm.grad is not None, k
        errs[k] = _rel(pm.grad, gr)
    worst = max(errs, key=errs.get)
    parity("grad_worst", errs[worst])
    print(name, "worst grad rel err %.2e (%s) over %d tensors" % (errs[worst], worst, on_path))
    assert on_path == 58
    assert e < FWD_TOL, (name, e)
    over = {k: v for k, v in errs.items() if not v < GRAD_TOL}
    assert not over, (name, over)


# ---- 3. two forwards, one backward -----------------------------------------------------------------------------------------------------------
def test_two_forwards_one_backward_sum_their_gradients():
    """every backward node takes a fresh gradient buffer (GPTST_Model._grad_buffer): two forwards of one fine-tuning model, one backward over
    the sum of their losses = the sum of the two separate backwards, to 1e-6 of scale.  (The node runs its reductions in the library's
    fixed-order mode: with the default float atomics two backwards of the SAME batch differed by 1.8e-6 in time_feature1.)"""
    args = make_args("PEMS08", mode="eval", num_nodes=23, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros())
    model = _finetune_model(args, O.init_state_dict(args, 11))
    B, N, C = 2, args.num_nodes, args.hidden_dim
    batches = [(synth.make_batch(B, 12, N, 1, seed=s).to(DEV), torch.randn(B, 12, N, C, generator=torch.Generator().manual_seed(s)).to(DEV))
               for s in (21, 22)]
    loss = lambda src, go: (model(src, None)[0] * go).sum()      # noqa: E731
    sep = []
    for src, go in batches:
        model.zero_grad(set_to_none=True)
        loss(src, go).backward()
        sep.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    assert len(sep[0]) == 58 and sep[0].keys() == sep[1].keys()
    assert any(not torch.equal(sep[0][k], sep[1][k]) for k in sep[0])
    model.zero_grad(set_to_none=True)
    (loss(*batches[0]) + loss(*batches[1])).backward()
    for k in sep[0]:
        want = sep[0][k].double() + sep[1][k].double()
        got = dict(model.named_parameters())[k].grad
        assert _rel(got, want.cpu()) < 1e-6, (k, _rel(got, want.cpu()))


# ---- 4. the whole chain ------------------------------------------------------------------------------------------------------------------
N4, B4 = 20, 2


def _chain(tmp_path, finetune, encoder_lr_scale=1.0):
    """EnhanceFrontEnd + STGCN at PEMS08, 20 nodes, on the GPU, its EvalTrainer, one batch and its target; and the oracle's encoder weights"""
    from gptst_amd import graph
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    from gptst_amd.predictors import STGCN
    args = make_args("PEMS08", mode="eval", num_nodes=N4, scaler_zeros=synth.scaler_zeros(), log_dir=str(tmp_path), debug=True,
                     model="STGCN_test", encoder_lr_scale=encoder_lr_scale, lr_init=1e-3)
    sd = O.init_state_dict(args, 11)
    ap = SimpleNamespace(Ks=3, Kt=3, num_nodes=N4, G=graph.stgcn_graph(graph.synthetic_adjacency(N4, 2)), blocks1=[64, 32, 128], drop_prob=0,
                         outputl_ks=3)
    torch.manual_seed(0)
    model = EnhanceFrontEnd(args, predictor=STGCN(ap, DEV, args.hidden_dim, args.output_dim), finetune_encoder=finetune).to(DEV)
    model.load_pretrained_model(sd)
    tr = EvalTrainer(model, args, None, None, None, synth.SCALER_MEAN, synth.SCALER_STD)
    tr.logger.setLevel(logging.WARNING)
    src = synth.make_batch(B4, 12, N4, 1, interval=args.interval, seed=21)
    target = synth.make_batch(B4, 12, N4, 1, interval=args.interval, seed=22, start_slot=12)
    return args, sd, ap, model, tr, src, target


def _steps(model, tr, src, target, n):
    losses = []
    model.train()
    for _ in range(n):
        tr.opt.zero_grad()
        loss = tr._loss(model(src, target)[0], target)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.requires_grad], tr.args.max_grad_norm)
        tr.opt.step()
        losses.append(float(loss))
    return losses


def test_whole_chain_gradients_and_training(tmp_path, parity):
    """encoder -> gate -> STGCN with the encoder fine-tuned: loss and every trainable gradient against the same computation in fp64 on the CPU
    (oracle eval forward -> torch Fusion / lin_test -> the same STGCN module in double), then 8 Adam steps through EvalTrainer's optimiser."""
    from gptst_amd.enhance import Fusion
    from gptst_amd.eval_trainer import masked_mae
    from gptst_amd.predictors import STGCN
    args, sd, ap, model, tr, src, target = _chain(tmp_path, True, encoder_lr_scale=0.1)
    C = args.hidden_dim
    # ---- the reference ----
    state = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    sd64 = _grad_sd(sd)
    fus, lin = Fusion(C).double(), torch.nn.Linear(1, C).double()
    pred = STGCN(ap, "cpu", C, args.output_dim).double()
    fus.load_state_dict({k[len("fusion."):]: v for k, v in state.items() if k.startswith("fusion.")})
    lin.load_state_dict({k[len("lin_test."):]: v for k, v in state.items() if k.startswith("lin_test.")})
    pred.load_state_dict({k[len("predictor."):]: v for k, v in state.items() if k.startswith("predictor.")})
    s64 = src.double()
    out_r = pred(fus(O.forward_eval(sd64, args, s64), lin(s64[..., :1])))
    loss_r = masked_mae(out_r, target.double()[..., :args.output_dim], synth.SCALER_MEAN, synth.SCALER_STD, args.mape_thresh)
    loss_r.backward()
    want = {"pretrain_model." + k: v.grad for k, v in sd64.items() if v.requires_grad and v.grad is not None and float(v.grad.abs().max()) > 0}
    for pfx, m in (("fusion.", fus), ("lin_test.", lin), ("predictor.", pred)):
        want.update({pfx + k: p.grad for k, p in m.named_parameters()})
    # ---- the product ----
    srcd, tgtd = src.to(DEV), target.to(DEV)
    model.train()
    loss = tr._loss(model(srcd, tgtd)[0], tgtd)
    el = abs(float(loss) - float(loss_r)) / abs(float(loss_r))
    parity("loss", el)
    print("whole chain: loss %.6f vs %.6f (rel %.2e)" % (float(loss), float(loss_r), el))
    loss.backward()
    named = dict(model.named_parameters())
    trainable = {k for k, p in named.items() if p.requires_grad}
    assert trainable == set(want), (sorted(trainable ^ set(want)))
    errs = {k: _rel(named[k].grad, want[k]) for k in sorted(trainable)}
    for grp in ("pretrain_model.", "fusion.", "lin_test.", "predictor."):
        ks = [k for k in errs if k.startswith(grp)]
        worst = max(ks, key=errs.get)
        parity("grad_worst:" + grp, errs[worst])
        print("whole chain: worst grad rel err of %s %.2e (%s)" % (grp, errs[worst], worst))
    assert el < 2e-6, (float(loss), float(loss_r))
    over = {k: v for k, v in errs.items() if not v < GRAD_TOL}
    assert not over, over
    # ---- 8 Adam steps on this batch ----
    assert [g["lr"] for g in tr.opt.param_groups] == [args.lr_init, 0.1 * args.lr_init]
    assert {id(p) for p in tr.opt.param_groups[1]["params"]} == {id(p) for k, p in named.items() if k.startswith("pretrain_model.") and p.requires_grad}
    before = {k: p.detach().clone() for k, p in named.items()}
    losses = _steps(model, tr, srcd, tgtd, 8)
    print("whole chain: losses", ["%.4f" % v for v in losses])
    assert losses[7] < losses[0], losses
    for k, p in named.items():
        if p.requires_grad:
            assert not torch.equal(p.detach(), before[k]), k
        else:
            assert k.startswith("pretrain_model.") and torch.equal(p.detach(), before[k]), k


def test_whole_chain_without_the_switch_leaves_the_encoder_alone(tmp_path):
    args, sd, ap, model, tr, src, target = _chain(tmp_path, False)
    assert len(tr.opt.param_groups) == 1 and tr.opt.param_groups[0]["lr"] == args.lr_init
    before = {k: p.detach().clone() for k, p in model.pretrain_model.named_parameters()}
    losses = _steps(model, tr, src.to(DEV), target.to(DEV), 8)
    assert losses[7] < losses[0], losses
    for k, p in model.pretrain_model.named_parameters():
        assert p.grad is None and torch.equal(p.detach(), before[k]), k


def test_best_state_carries_the_finetuned_encoder(tmp_path):
    """EvalTrainer.train() with the encoder fine-tuned: the best state dict it keeps (and loads back at the end) holds pretrain_model.* with the
    encoder path moved away from the loaded checkpoint and everything else of the pretrained model as loaded"""
    from gptst_amd import data as gdata, graph
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    from gptst_amd.predictors import STGCN
    N = 20
    args = make_args("PEMS08", mode="eval", num_nodes=N, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros(), batch_size=8, epochs=2,
                     early_stop=False, log_dir=str(tmp_path), debug=True, model="STGCN_test", encoder_lr_scale=0.1)
    sd = O.init_state_dict(args, 4)
    raw = synth.make_series(N, 3, days=6, seed=3)
    train, val, test, scaler, _, _ = gdata.get_dataloader(args, device=DEV, raw=raw, generator=torch.Generator().manual_seed(1))
    ap = SimpleNamespace(Ks=3, Kt=3, num_nodes=N, G=graph.stgcn_graph(graph.synthetic_adjacency(N, 2)), blocks1=[64, 32, 128], drop_prob=0,
                         outputl_ks=3)
    torch.manual_seed(0)
    model = EnhanceFrontEnd(args, predictor=STGCN(ap, DEV, args.hidden_dim, args.output_dim), finetune_encoder=True).to(DEV)
    model.load_pretrained_model(sd)
    tr = EvalTrainer(model, args, train, val, test, float(scaler.mean), float(scaler.std))
    tr.logger.setLevel(logging.WARNING)
    best, rows = tr.train()
    assert best is not None and bool(torch.isfinite(rows[:, :3]).all())
    trained = {k for k, p in model.pretrain_model.named_parameters() if p.requires_grad}
    assert len(trained) == 58
    for k, v in sd.items():
        same = torch.equal(best["pretrain_model." + k].cpu(), v)
        assert same != (k in trained), k
    now = model.state_dict()
    assert all(torch.equal(now[k], best[k]) for k in best)
