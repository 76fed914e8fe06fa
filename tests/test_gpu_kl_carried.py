"""GPU: the KL path's backward carried as guest workgroups of the forward's hyperTem chain launches (engine.KlCarry,
gptst_hypertem_chain_fwd_kl) against the same step with the three stand-alone launches (GPTST_CARRY_KL=0)."""
import pytest
import torch

from gptst_amd import synth
from gptst_amd.config import make_args
from step_grad_util import noise_inject, one_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUIDE = ("encoder.MLP_RL.",)
# (the embeddings teb4mask / neb4mask collect their gradients with float atomics outside deterministic mode — gptst_pool_jobs kind 2,
#  gptst_timefeat_jobs — so two runs of the SAME launches already differ in their last bits there: compared to rounding below)
GUIDE_EMB = ("encoder.teb4mask.", "encoder.neb4mask")


def _args(dataset, **over):
    return make_args(dataset, **dict(dict(scaler_zeros=synth.scaler_zeros(), epochs=30, change_epoch=3), **over))


def _step(args, B, carry, epoch, deterministic=False, record=False):
    """one fused step from the seed-3 state with injected noise (step_grad_util.one_step), the carried form switched by `carry`
    -> (gradient views, losses, mask, launch names, stepper)"""
    from gptst_amd import engine
    keep = engine.CARRY_KL
    engine.CARRY_KL = carry
    try:
        grads, _, mask, names, st = one_step(args, B, epoch, deterministic=deterministic, sd_seed=3, inject=noise_inject(args, B, epoch))
    finally:
        engine.CARRY_KL = keep
    return grads, st.losses(), mask, names if record else None, st


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
