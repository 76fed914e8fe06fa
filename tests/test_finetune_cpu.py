"""Fine-tuning the pretrained encoder downstream (``-mode eval -finetune_encoder True``): the switches, without a GPU.  What is trainable is
checked against the oracle: exactly the tensors its eval forward has a gradient for."""
import torch

from gptst_amd import synth
from gptst_amd.config import make_args, parse_args
from oracle import gptst_oracle as O


def test_finetune_flags_parse_with_their_defaults():
    a = parse_args("cpu", ["-dataset", "PEMS08", "-mode", "eval"])
    assert a.finetune_encoder is False and a.encoder_lr_scale == 1.0
    a = parse_args("cpu", ["-dataset", "PEMS08", "-mode", "eval", "-finetune_encoder", "True", "-encoder_lr_scale", "0.1"])
    assert a.finetune_encoder is True and a.encoder_lr_scale == 0.1
    m = make_args("PEMS08", mode="eval")
    assert m.finetune_encoder is False and m.encoder_lr_scale == 1.0


def _oracle_trained_keys(args, B=2):
    """the state-dict keys the oracle's eval embedding has a non-zero gradient for"""
    sd = {k: (v.clone() if k.endswith("mask_template") else v.clone().requires_grad_(True)) for k, v in O.init_state_dict(args, 11).items()}
    src = synth.make_batch(B, 12, args.num_nodes, args.input_base_dim, interval=args.interval, seed=21)
    emb = O.forward_eval(sd, args, src)
    go = torch.randn(emb.shape, generator=torch.Generator().manual_seed(7))
    (emb * go).sum().backward()
    return {k for k, v in sd.items() if v.requires_grad and v.grad is not None and bool(v.grad.abs().max() > 0)}


def test_finetune_encoder_marks_what_the_oracle_differentiates():
    from gptst_amd.enhance import EnhanceFrontEnd
    for ds, over in (("PEMS08", dict(num_nodes=20, embed_dim=8, HS=5, HT=6)), ("NYC_TAXI", dict(num_nodes=17, HS=2))):
        args = make_args(ds, mode="eval", scaler_zeros=synth.scaler_zeros(), **over)
        want = _oracle_trained_keys(args)
        assert len(want) == 58
        fe = EnhanceFrontEnd(args, finetune_encoder=True)
        assert fe.pretrain_model.finetune is True
        got = {k for k, p in fe.pretrain_model.named_parameters() if p.requires_grad}
        assert got == want, (sorted(got - want), sorted(want - got))
        frozen = {k for k, p in fe.pretrain_model.named_parameters() if not p.requires_grad}
        assert all(k.startswith(("encoder.MLP_RL.", "encoder.teb4mask.", "decoder.")) or k == "encoder.neb4mask" for k in frozen), sorted(frozen)
        assert all(p.requires_grad for p in list(fe.fusion.parameters()) + list(fe.lin_test.parameters()))


def test_default_front_end_keeps_the_encoder_frozen():
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    args = make_args("PEMS08", mode="eval", num_nodes=20, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros())
    fe = EnhanceFrontEnd(args)
    assert fe.pretrain_model.finetune is False
    assert not any(p.requires_grad for p in fe.pretrain_model.parameters())
    # one plain parameter list, as before the switch existed; two groups once the encoder is trained
    groups = EvalTrainer.param_groups(fe, args)
    assert all(torch.is_tensor(p) for p in groups) and len(groups) == 8
    args.encoder_lr_scale = 0.1
    g2 = EvalTrainer.param_groups(EnhanceFrontEnd(args, finetune_encoder=True), args)
    assert [len(g["params"]) for g in g2] == [8, 58] and "lr" not in g2[0] and g2[1]["lr"] == args.lr_init * 0.1
