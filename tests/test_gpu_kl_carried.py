"""GPU: the KL path's backward carried as guest workgroups of the forward's hyperTem chain launches (engine.KlCarry,
gptst_hypertem_chain_fwd_kl) against the same step with the three stand-alone launches (GPTST_CARRY_KL=0)."""
import pytest
import torch

from gptst_amd import synth
from gptst_amd.config import make_args
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUIDE = ("encoder.MLP_RL.",)
# (the embeddings teb4mask / neb4mask collect their gradients with float atomics outside deterministic mode — gptst_pool_jobs kind 2,
#  gptst_timefeat_jobs — so two runs of the SAME launches already differ in their last bits there: compared to rounding below)
GUIDE_EMB = ("encoder.teb4mask.", "encoder.neb4mask")


def _args(dataset, **over):
    return make_args(dataset, **dict(dict(scaler_zeros=synth.scaler_zeros(), epochs=30, change_epoch=3), **over))


def _step(args, B, carry, epoch, deterministic=False, record=False):
    """one fused step from the seed-3 state with injected noise -> (gradient views, losses, mask, launch names, stepper)"""
    from gptst_amd import engine, ops
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    sd = O.init_state_dict(args, 3)
    model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
    st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B, use_graph=False, deterministic=deterministic)
    N = args.num_nodes
    M = B * 12 * N
    src = synth.make_batch(B, 12, N, 1, seed=11).to(DEV)
    keep = engine.CARRY_KL
    engine.CARRY_KL = carry
    try:
        for _ in range(2):                           # the first step sizes the zero arena; the second is the one compared
            ops.TIMER = [] if record else None
            if epoch <= args.change_epoch:
                st.step(src, epoch, noise=synth.make_noise(M, 21).to(DEV))
            else:
                st.step(src, epoch, noise_a=synth.make_noise(M, 22).to(DEV), noise_r=synth.make_noise(M, 23).to(DEV),
                        list_c=synth.class_order(args.HS, 4))
            names = [r[0] for r in ops.TIMER] if record else None
            ops.TIMER = None
            model.load_state_dict(sd)                # (the second step starts from the same weights)
            st.m.zero_(); st.v.zero_()
        torch.cuda.synchronize()
    finally:
        engine.CARRY_KL = keep
        ops.TIMER = None
    grads = {k: v.detach().clone() for k, v in st.g.items()}
    return grads, st.losses(), st.last_mask.clone(), names, st


SHAPES = [("PEMS08", 32, {}), ("METR_LA", 8, {}), ("PEMS08", 2, dict(num_nodes=24, embed_dim=8, HS=6, HT=8))]


@pytest.mark.parametrize("dataset,B,over", SHAPES, ids=["bench_N170_B32", "metr_la_N207", "small_N24"])
def test_carried_kl_path_equals_standalone_launches(dataset, B, over):
    args = _args(dataset, **over)
    assert args.hidden_dim == 64
    g0, l0, m0, n0, _ = _step(args, B, False, 20, record=True)
    g1, l1, m1, n1, _ = _step(args, B, True, 20, record=True)
    # the carried form really ran: three chain launches with a guest stage each, and the three stand-alone launches are gone
    assert n1.count("gptst_hypertem_chain_fwd_kl") == 3 and "gptst_tail_kl" in n0 and "gptst_guide_in_bwd" in n0
    assert "gptst_tail_kl" not in n1 and "gptst_guide_in_bwd" not in n1
    assert len(n1) == len(n0) - 3
    assert torch.equal(m0, m1), "mask"
    assert l0 == l1, (l0, l1)                        # MAE and KL statistics: bit-identical
    for k in g0:
        if k.startswith(GUIDE):
            assert torch.equal(g0[k], g1[k]), k      # the guide's gradients: same kernels, same reduction jobs in the same order
        elif k.startswith(GUIDE_EMB):
            torch.testing.assert_close(g1[k], g0[k], rtol=1e-5, atol=1e-6, msg=k)
        else:
            torch.testing.assert_close(g1[k], g0[k], rtol=2e-3, atol=1e-5, msg=k)


@pytest.mark.parametrize("epoch,deterministic", [(1, False), (20, True)], ids=["phase0", "deterministic_phase1"])
def test_other_steps_enqueue_the_same_launches(epoch, deterministic):
    args = _args("PEMS08", num_nodes=24, embed_dim=8, HS=6, HT=8)
    _, l0, m0, n0, _ = _step(args, 2, False, epoch, deterministic=deterministic, record=True)
    _, l1, m1, n1, _ = _step(args, 2, True, epoch, deterministic=deterministic, record=True)
    assert n0 == n1 and "gptst_hypertem_chain_fwd_kl" not in n1
    assert torch.equal(m0, m1) and l0 == l1
