"""GPU: the fused optimisation step (fwd + loss + bwd + clip + Adam as HIP kernels, eager and hipGraph replay) against
the reference's step sequence (golden) and the pinned oracle."""
import numpy as np
import pytest
import torch

from golden_util import load, t
from gptst_amd import synth
from gptst_amd.config import make_args
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _args():
    return make_args("PEMS08", num_nodes=20, embed_dim=8, HS=5, HT=6, num_route=2, scaler_zeros=synth.scaler_zeros(),
                     epochs=30, change_epoch=3)


@pytest.mark.parametrize("use_graph", [False, True])
def test_step_sequence_vs_reference(use_graph):
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    fx = load("steps.npz")
    args = _args()
    sd = O.init_state_dict(args, int(fx["sd_seed"]))
    model = GPTST_Model(args)
    model.load_state_dict(sd)
    model = model.to(DEV)
    st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=4, use_graph=use_graph)
    losses = fx["losses"]
    for step in range(losses.shape[0]):
        epoch = int(fx["st%d.epoch" % step])
        src = synth.make_batch(4, 12, 20, 1, seed=500 + step, start_slot=17 * step).to(DEV)
        tag = "st%d" % step
        ref_masked = t(fx, tag + ".mask")                       # reference's 1 - final_mask (1 = masked)
        if epoch <= args.change_epoch:
            st.step(src, epoch, noise=t(fx, tag + ".noise0").to(DEV))
            vis = st.last_mask.view(4, 12, 20, 1)
            assert torch.equal((1 - vis).cpu().to(torch.int8), ref_masked), "mask bit-exact, step %d" % step
        else:
            # Adaptive phase: the mask depends on argmax of the fp32 classifier output, which can flip between devices at
            # round-off level once training sharpens/blurs the clusters.  Check the free-running device mask
            # (same budget, overwhelmingly the same cells), then teacher-force the reference mask to keep the trajectories aligned.
            model.set_mask_inputs(noise_a=t(fx, tag + ".noise0"), noise_r=t(fx, tag + ".noise1"),
                                  list_c=[int(i) for i in fx[tag + ".list_c"]])
            with torch.no_grad():
                from gptst_amd import engine
                prob0, _ = engine.guide_fwd(model.param_views(), src, model._tidx(src), model._dims(src), 1)
                free = model.make_mask(src, prob0, epoch).cpu()
            assert int((free == 0).sum()) == int(ref_masked.sum())
            agree = float(((1 - free).view(-1) == ref_masked.view(-1).float()).float().mean())
            assert agree > 0.9, (step, agree)
            st.step(src, epoch, forced_mask=(1 - ref_masked.float()).to(DEV))
        got = st.losses()
        # total / flow loss: 1e-4 (north-star loss-curve bound is 1e-3); the KL term is a small difference of logs and
        # amplifies fp32 round-off of the classifier (observed 4.5e-4 at step 7), so it gets the 1e-3-class bound.
        np.testing.assert_allclose(got[:2], losses[step][:2], rtol=1e-4 if step < 10 else 2e-3, err_msg="step %d" % step)
        np.testing.assert_allclose(got[2], losses[step][2], rtol=5e-3, err_msg="step %d (KL)" % step)
    for k, v in model.state_dict().items():
        key = "sdN." + k
        ref = t(fx, key).reshape(-1) if key in fx.files else t(fx, key + "::sub")
        val = v.detach().cpu().reshape(-1) if key in fx.files else v.detach().cpu().reshape(-1)[::13]
        rel = float((val - ref).norm() / ref.norm().clamp_min(1e-12))
        # Adam maps a sign flip of a round-off-level gradient (e.g. cap.t_adj early on) to a +-lr move per step, so single
        # tensors are chaotic across devices; 0.1 still catches a wrong optimiser (>=0.3).  Exact Adam/clip arithmetic is
        # pinned separately by test_clip_adam_matches_torch (2e-6).
        from conftest import record_current
        record_current("param_rel_l2_after_12_steps", rel)
        assert rel < 0.1, (k, rel)
    assert (st.tA, st.tB) == (12, 6)


def test_graph_replay_equals_eager_and_random_noise_changes():
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = _args()
    sd = O.init_state_dict(args, 1)
    res = []
    for use_graph in (False, True):
        model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
        st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=4, use_graph=use_graph)
        ls = []
        for i in range(4):
            src = synth.make_batch(4, 12, 20, 1, seed=i).to(DEV)
            st.step(src, 1 if i < 2 else 20, noise=synth.make_noise(960, i).to(DEV), noise_a=synth.make_noise(960, i).to(DEV),
                    noise_r=synth.make_noise(960, 9 + i).to(DEV), list_c=[3, 1, 0, 4, 2])
            ls.append(st.losses())
        res.append((ls, model.flat.clone()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5)
    assert float((res[0][1] - res[1][1]).abs().max()) < 1e-5
    # free-running noise inside the graph: masks differ between replays, budget is exact
    model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
    st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=4, use_graph=True)
    src = synth.make_batch(4, 12, 20, 1, seed=0).to(DEV)
    masks = []
    for i in range(3):
        st.step(src, 1)
        masks.append(st.last_mask.clone())
        assert int((masks[-1] == 0).sum()) == int(960 * 0.25)
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2])


class _FakeDP:
    """Stands in for dist.DataParallel on one GPU: the peers' labels / counts are injected, the gradient all-reduce is a no-op."""

    def __init__(self, rank, world, labels, counts):
        self.rank, self.world, self.labels, self.counts = rank, world, labels, counts

    def gather_labels(self, local, out=None):
        assert torch.equal(local, self.labels[self.rank])           # the step's own labels = what the peers would receive
        out.copy_(torch.cat(self.labels))
        return out

    def sum_counts_(self, counts):
        counts.copy_(sum(self.counts))
        return counts

    def rows_of(self, flat, per_rank):
        return flat[self.rank * per_rank:(self.rank + 1) * per_rank]

    def allreduce_(self, buf):
        return buf


@pytest.mark.parametrize("use_graph", [False, True])
def test_dp_global_mask_equals_single_process_global_batch(use_graph):
    """under data parallelism the mask is ONE selection over the global batch (GPTST.py:316-321,351-404).  Two
    ranks with B=2 each (emulated one after the other on this GPU) must cut exactly their rows out of the mask a single
    process generates for B=4 — random phase (no exchange) and adaptive phase (label all-gather + count all-reduce) — and
    the oracle on the global batch agrees bit for bit."""
    from gptst_amd import engine, ops
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = _args()
    sd = O.init_state_dict(args, 1)
    W, Bl, Mg = 2, 2, 4 * 12 * 20
    M = Mg // W
    src_g = synth.make_batch(4, 12, 20, 1, seed=11).to(DEV)
    n0, na, nr = (synth.make_noise(Mg, s).to(DEV) for s in (1, 2, 3))
    list_c = [3, 1, 0, 4, 2]

    def fresh(B, dp=None):
        model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
        return model, PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B, use_graph=use_graph, dp=dp)

    # per-rank labels / counts, as the ranks compute them (guide forward + argmax on their own rows)
    model, _ = fresh(4)
    labels, counts = [], []
    for r in range(W):
        src = src_g[r * Bl:(r + 1) * Bl].contiguous()
        engine.CTX.ARENA = engine.ZeroArena(torch.device(DEV)); engine.CTX.ARENA.begin()
        prob, _ = engine.guide_fwd(model.param_views(), src, src[:, :, 0, 1:3].contiguous(), (Bl, 12, 20, args.hidden_dim), 1)
        lab, cnt = ops.mask_labels(prob)
        engine.CTX.ARENA = None
        labels.append(lab.clone()); counts.append(cnt.clone())
    for epoch in (1, 20):
        _, st = fresh(4)
        st.step(src_g, epoch, noise=n0, noise_a=na, noise_r=nr, list_c=list_c)
        mask_ref = st.last_mask.clone()
        # the oracle on the global batch (integer path: bit exact given the labels)
        if epoch == 1:
            want = O.random_mask(n0.cpu(), args.mask_ratio)
        else:
            ada, rnd = O.adaptive_counts(Mg, args.mask_ratio, epoch, args.change_epoch, args.epochs, args.ada_mask_ratio)
            want = O.adaptive_mask(torch.cat(labels).cpu().long(), list_c, na.cpu(), nr.cpu(), ada, rnd, args.ada_type)[2]
        assert torch.equal(mask_ref.cpu().long(), want.reshape(-1).long())
        for r in range(W):
            _, sr = fresh(Bl, dp=_FakeDP(r, W, labels, counts))
            assert sr.gmask
            for _ in range(2 if epoch == 1 else 1):              # (the optimiser moves the guide, so labels are compared once)
                sr.step(src_g[r * Bl:(r + 1) * Bl].contiguous(), epoch, noise=n0, noise_a=na, noise_r=nr, list_c=list_c)
                torch.cuda.synchronize()
                assert torch.equal(sr.last_mask, mask_ref[r * M:(r + 1) * M]), (epoch, r)


class _TailDP(_FakeDP):
    """Two ranks of a padded tail round, one after the other on this GPU: the first records what it sends into the all-reduce, the second
    receives it (sum of the two contributions)."""

    def __init__(self, rank, peer_sent=None):
        super().__init__(rank, 2, None, None)
        self.sent, self.peer_sent = None, peer_sent

    def allreduce_(self, buf):
        self.sent = buf.clone()
        if self.peer_sent is not None:
            buf.add_(self.peer_sent)
        return buf


@pytest.mark.parametrize("epoch", [1, 20])
def test_padded_tail_round_of_a_data_parallel_epoch(epoch):
    """r04 (the tail of a data-parallel epoch is kept): a rank without a batch of its own steps on padding with rank_weight 0 — its gradient
    AND loss statistics are zeroed before the all-reduce.  With per-rank masks the round must then be exactly the single-process step on the
    real batch: same losses, same weights on BOTH ranks (the replicas stay identical), whatever the padding rank computed."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = _args()
    sd = O.init_state_dict(args, 4)
    M = 4 * 12 * 20
    real, pad = synth.make_batch(4, 12, 20, 1, seed=31).to(DEV), synth.make_batch(4, 12, 20, 1, seed=32).to(DEV)
    kw = dict(noise=synth.make_noise(M, 5).to(DEV)) if epoch == 1 else dict(
        noise_a=synth.make_noise(M, 6).to(DEV), noise_r=synth.make_noise(M, 7).to(DEV), list_c=[2, 0, 4, 1, 3])

    def run(src, dp, weight):
        model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
        st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=4, use_graph=False, dp=dp, global_mask=False, deterministic=True)
        st.rank_weight = weight
        st.step(src, epoch, **kw)
        torch.cuda.synchronize()
        return st.losses(), {k: v.detach().clone() for k, v in model.state_dict().items()}

    l_plain, w_plain = run(real, None, 1.0)
    dp0 = _TailDP(0)
    l0, w0 = run(real, dp0, 1.0)
    assert float(dp0.sent.abs().max()) > 0
    dp1 = _TailDP(1, peer_sent=dp0.sent)
    l1, w1 = run(pad, dp1, 0.0)
    assert float(dp1.sent.abs().max()) == 0.0, "the padding rank must contribute nothing (gradient and statistics)"
    np.testing.assert_allclose(l0, l_plain, rtol=1e-6)
    np.testing.assert_allclose(l1, l_plain, rtol=1e-6)                 # the job's loss is the real batch's, on every rank
    for k in w_plain:
        assert torch.equal(w1[k], w0[k]), k                            # the replicas stay bit-identical
        # vs the plain stepper: the data-parallel form sums the loss gradient and divides by the kept-cell count in the optimiser (one rounding apart)
        assert float((w0[k] - w_plain[k]).abs().max()) <= 2e-6 * max(float(w_plain[k].abs().max()), 1e-3) + 1e-9, k


@pytest.mark.parametrize("use_graph", [False, True])
def test_unsynced_queue_equals_synced_steps(use_graph):
    """50 steps enqueued back to back with NO host sync (what bench.py does) must see the same per-step host scalars (Adam bias
    corrections, class order, mask budgets) on the device as 50 steps with a sync after each: the pinned host slots are a ring
    guarded by events — a single reused pinned buffer is overwritten before its H2D copy has run (ADVICE r1, step.py)."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = _args()
    sd = O.init_state_dict(args, 2)
    src = synth.make_batch(4, 12, 20, 1, seed=77).to(DEV)
    M = 4 * 12 * 20
    noise = [synth.make_noise(M, 100 + i).to(DEV) for i in range(50)]
    noise_r = [synth.make_noise(M, 200 + i).to(DEV) for i in range(50)]
    orders = [synth.class_order(5, 300 + i) for i in range(50)]
    outs = []
    for sync in (True, False):
        model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
        st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=4, use_graph=use_graph)
        seen = []
        for i in range(50):
            epoch = 1 + (i * 29) // 50                      # crosses change_epoch = 3 -> both phases, tB lags tA
            if epoch <= args.change_epoch:
                st.step(src, epoch, noise=noise[i])
            else:
                st.step(src, epoch, noise_a=noise[i], noise_r=noise_r[i], list_c=orders[i])
            seen.append((st.hyper.clone(), st.ctrl.clone()))        # stream-ordered snapshots of what step i ran with
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        outs.append((seen, model.flat.clone()))
    for i, ((h0, c0), (h1, c1)) in enumerate(zip(outs[0][0], outs[1][0])):
        assert torch.equal(h0, h1), "step %d ran with another step's Adam bias corrections" % i
        assert torch.equal(c0, c1), "step %d ran with another step's class order / mask budgets" % i
    # (the final parameters are NOT compared: float atomics make two runs differ at round-off level and 50 Adam steps at lr 3e-3
    # with free-running adaptive masks amplify that to O(0.2) relative — the device-side snapshots above are the exact check)
    assert torch.isfinite(outs[1][1]).all()


@pytest.mark.parametrize("use_graph,N,over", [(False, 20, {}), (True, 20, {}), (False, 300, dict(hidden_dim=128, HS=10))],
                         ids=["eager", "graph", "c128_streaming_cap"])
def test_deterministic_mode_is_bit_reproducible(use_graph, N, over):
    """GPTST_DETERMINISTIC / PretrainStep(deterministic=True): two runs of the same 12 steps (both phases, injected noise, free-running
    adaptive masks) end in bit-identical parameters and optimiser state — no float atomics are left on the path.  c128_streaming_cap:
    the C = 128 kernels (apply128 / wgrad128 / tmix_bwd) and the capflow passes (N = 300 does not fit LDS at C = 128)."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = make_args("PEMS08", **dict(dict(num_nodes=N, embed_dim=8, HS=5, HT=6, num_route=2, scaler_zeros=synth.scaler_zeros(),
                                           epochs=30, change_epoch=3), **over))
    sd = O.init_state_dict(args, 2)
    Bt = 4 if N == 20 else 2
    src = [synth.make_batch(Bt, 12, N, 1, seed=70 + i).to(DEV) for i in range(12)]
    M = Bt * 12 * N
    outs = []
    for rep in range(2):
        model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
        st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=Bt, use_graph=use_graph, deterministic=True)
        losses = []
        for i in range(12):
            epoch = 1 + i // 2                               # change_epoch = 3: steps 6.. are adaptive + KL
            na, nr = synth.make_noise(M, 500 + i).to(DEV), synth.make_noise(M, 600 + i).to(DEV)
            if epoch <= args.change_epoch:
                st.step(src[i], epoch, noise=na)
            else:
                st.step(src[i], epoch, noise_a=na, noise_r=nr, list_c=synth.class_order(args.HS, i))
            losses.append(st.losses())
        outs.append((model.flat.clone(), st.m.clone(), st.v.clone(), losses))
    assert outs[0][3] == outs[1][3], "losses differ between two deterministic runs"
    for a, b, nm in zip(outs[0][:3], outs[1][:3], ("parameters", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), "%s differ between two deterministic runs" % nm


def test_step_group_equals_single_steps():
    """PretrainStep.step_group: K consecutive steps in ONE graph replay (one H2D copy of the K steps' host scalars) leave the same
    parameters, optimiser state and per-step losses as K step() calls — bit for bit in deterministic mode, both mask phases, free-running
    Philox noise (keyed by the step counter, so the two runs draw the same masks)."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = _args()
    sd = O.init_state_dict(args, 2)
    K = 4
    srcs = [synth.make_batch(4, 12, 20, 1, seed=900 + i).to(DEV) for i in range(4 * K)]
    orders = [synth.class_order(5, 40 + i) for i in range(4 * K)]
    outs = []
    for grouped in (False, True):
        model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
        st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=4, use_graph=True, deterministic=True)
        losses = []
        for blk in range(4):
            epoch = 2 if blk < 2 else 5                      # change_epoch = 3: two groups per phase (the second replays the captured graph)
            ss, oo = srcs[blk * K:(blk + 1) * K], orders[blk * K:(blk + 1) * K]
            if grouped:
                assert st.group_ok(epoch)
                st.step_group(ss, epoch, list_cs=oo)
                losses += st.losses_group()
                assert st.losses() == losses[-1]
            else:
                for s_, o_ in zip(ss, oo):
                    st.step(s_, epoch, list_c=o_)
                    losses.append(st.losses())
        outs.append((model.flat.clone(), st.m.clone(), st.v.clone(), losses, (st.tA, st.tB)))
    assert outs[0][4] == outs[1][4] == (16, 8)
    assert outs[0][3] == outs[1][3], (outs[0][3], outs[1][3])
    for a, b, nm in zip(outs[0][:3], outs[1][:3], ("parameters", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), "%s differ between grouped and single steps" % nm
    # a single step after a group continues the same sequence
    st.step(srcs[0], 5, list_c=orders[0])
    assert st.losses()[0] > 0


def test_lost_handoff_skips_the_update_and_the_step_is_rerun():
    """r05: an expired in-launch hand-off used to end the run in NaN.  Now the optimiser SKIPS the update of such a step
    (weights, moments untouched; stats_out[5] > 0), losses() / losses_group() notice, the stepper re-captures its graphs without hand-off launches
    and re-runs the skipped steps.  An expiry is put on record with the testing hook gptst_handoff_inject before a single step and before a group:
    the run ends bit-identical (deterministic mode) to one that never lost a hand-off."""
    from gptst_amd import _C
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = _args()
    sd = O.init_state_dict(args, 2)
    K = 4
    srcs = [synth.make_batch(4, 12, 20, 1, seed=900 + i).to(DEV) for i in range(3 * K)]
    orders = [synth.class_order(5, 40 + i) for i in range(3 * K)]
    lib = _C.lib()
    outs = []
    try:
        for lose in (False, True):
            model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
            st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=4, use_graph=True, deterministic=True)
            losses = []
            # block 0: single steps in the random-mask phase; the hand-off is "lost" in front of the third one
            for i in range(K):
                if lose and i == 2:
                    torch.cuda.synchronize()
                    before = model.flat.clone()
                    lib.call("gptst_handoff_inject", 1)
                st.step(srcs[i], 2, list_c=orders[i])
                if lose and i == 2:
                    torch.cuda.synchronize()
                    assert torch.equal(model.flat, before), "the update of a step with a lost hand-off must be skipped"
                    assert float(st.stats_out[5]) == 1.0
                losses.append(st.losses())                       # notices, re-captures without hand-offs, re-runs the step
                if lose and i == 2:
                    assert st.safe_mode and st.lost_steps == 1 and not torch.equal(model.flat, before)
            # blocks 1, 2: groups in the adaptive phase; in the second run the expiry is on record before block 2 (in safe mode already: the
            # recovery path is the same — every update of the group is skipped, losses_group() re-runs all K steps)
            for blk in (1, 2):
                ss, oo = srcs[blk * K:(blk + 1) * K], orders[blk * K:(blk + 1) * K]
                if lose and blk == 2:
                    torch.cuda.synchronize()
                    lib.call("gptst_handoff_inject", 2)
                st.step_group(ss, 5, list_cs=oo)
                losses += st.losses_group()
            assert not lose or st.lost_steps == 1 + K
            outs.append((model.flat.clone(), st.m.clone(), st.v.clone(), losses, (st.tA, st.tB)))
    finally:
        lib.call("gptst_handoff_reset")
    assert outs[0][4] == outs[1][4] == (3 * K, 2 * K)
    assert outs[0][3] == outs[1][3], (outs[0][3], outs[1][3])
    for a, b, nm in zip(outs[0][:3], outs[1][:3], ("parameters", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), "%s differ after the recovery from a lost hand-off" % nm
    n = __import__("ctypes").c_int(-1)
    lib.call("gptst_handoff_timeouts", __import__("ctypes").byref(n))
    assert n.value == 0


def test_lost_handoff_with_several_steps_enqueued_before_the_host_looks():
    """the optimiser's guard skips EVERY update while an expiry is on record, and a caller may enqueue several step()s before one losses()
    (bench loops) or run a group that fell back to single steps.  The device counts the skipped updates (stats_out[6]); losses() takes all of them
    back (Adam's bias-correction counters, the Philox step key) and repeats the last one — the earlier batches are gone and are reported as such;
    the fallen-back group keeps its sources and repeats every skipped step.  Both end bit-identical (deterministic mode) to runs that stepped on
    exactly the batches that were applied."""
    from gptst_amd import _C
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = _args()
    sd = O.init_state_dict(args, 2)
    srcs = [synth.make_batch(4, 12, 20, 1, seed=930 + i).to(DEV) for i in range(9)]
    orders = [synth.class_order(5, 60 + i) for i in range(9)]
    lib = _C.lib()

    def fresh(group_fails=False):
        model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
        st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=4, use_graph=True, deterministic=True)
        st._group_failed = group_fails
        return model, st
    try:
        # (a) steps 0, 1 seen; the hand-off is lost in front of step 2; steps 2, 3, 4 enqueued, then ONE losses()
        m0, s0 = fresh()
        for i in (0, 1, 4):
            s0.step(srcs[i], 5, list_c=orders[i]); l0 = s0.losses()
        m1, s1 = fresh()
        for i in (0, 1):
            s1.step(srcs[i], 5, list_c=orders[i]); s1.losses()
        torch.cuda.synchronize()
        lib.call("gptst_handoff_inject", 1)
        for i in (2, 3, 4):
            s1.step(srcs[i], 5, list_c=orders[i])
        l1 = s1.losses()
        assert s1.safe_mode and s1.lost_steps == 3 and s1.lost_batches == 2 and (s1.tA, s1.tB) == (s0.tA, s0.tB) == (3, 3)
        assert l1 == l0 and torch.equal(m1.flat, m0.flat) and torch.equal(s1.m, s0.m) and torch.equal(s1.v, s0.v)
        # (b) a group that runs as single steps (capture refused): expiry in front of its third step -> steps 2, 3 repeated from the kept sources
        m2, s2 = fresh(group_fails=True)
        s2.step_group(srcs[5:9], 5, list_cs=orders[5:9]); l2 = s2.losses_group()
        m3, s3 = fresh(group_fails=True)
        s3.step_group(srcs[5:7], 5, list_cs=orders[5:7]); l3 = s3.losses_group()
        torch.cuda.synchronize()
        lib.call("gptst_handoff_inject", 1)
        s3.step_group(srcs[5:9], 5, list_cs=orders[5:9])          # (its first two steps are skipped too: they repeat steps 5, 6 on top — compare with the same sequence)
        l3b = s3.losses_group()
        m4, s4 = fresh(group_fails=True)
        s4.step_group(srcs[5:7], 5, list_cs=orders[5:7]); s4.losses_group()
        s4.step_group(srcs[5:9], 5, list_cs=orders[5:9]); l4 = s4.losses_group()
        assert s3.lost_steps == 4 and (s3.tA, s3.tB) == (s4.tA, s4.tB) == (6, 6)
        assert l3b == l4 and torch.equal(m3.flat, m4.flat) and torch.equal(s3.m, s4.m)
        assert len(l2) == 4
        # (c) TWO graph-replayed groups enqueued before one look, the expiry in front of the first: all eight updates are skipped; the last group is repeated,
        # the first group's four steps are taken back and reported lost -> the state of a run that stepped on the second group only
        m5, s5 = fresh()
        s5.step_group(srcs[1:5], 5, list_cs=orders[1:5]); s5.losses_group()          # (captures the group graph; four applied steps)
        m6, s6 = fresh()
        s6.step_group(srcs[1:5], 5, list_cs=orders[1:5]); s6.losses_group()
        torch.cuda.synchronize()
        lib.call("gptst_handoff_inject", 1)
        s6.step_group(srcs[5:9], 5, list_cs=orders[5:9])
        s6.step_group(srcs[0:4], 5, list_cs=orders[0:4])
        l6 = s6.losses_group()
        s5.step_group(srcs[0:4], 5, list_cs=orders[0:4]); l5 = s5.losses_group()
        assert s6.lost_batches == 4 and s6.lost_steps == 8 and (s6.tA, s6.tB) == (s5.tA, s5.tB) == (8, 8)
        assert l6 == l5 and torch.equal(m6.flat, m5.flat) and torch.equal(s6.m, s5.m)
    finally:
        lib.call("gptst_handoff_reset")


def _handoff_case(seed):
    """shape and setup of the lost-hand-off tests: B=4, T=12, N=20, base 1, deterministic -> (fresh, batches, class orders)"""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = _args()
    sd = O.init_state_dict(args, 2)

    def fresh(group_fails=False):
        model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
        st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=4, use_graph=True, deterministic=True)
        st._group_failed = group_fails
        return model, st
    return fresh, [synth.make_batch(4, 12, 20, 1, seed=seed + i).to(DEV) for i in range(10)], [synth.class_order(5, 60 + i) for i in range(10)]


def _assert_same_state(got, want):
    (m1, s1, l1), (m0, s0, l0) = got, want
    assert l1 == l0, (l1, l0)
    assert torch.equal(m1.flat, m0.flat) and torch.equal(s1.m, s0.m) and torch.equal(s1.v, s0.v)
    assert (s1.tA, s1.tB) == (s0.tA, s0.tB)


def test_lost_handoff_in_fallen_back_groups_enqueued_before_one_look():
    """Groups that run as single steps, SEVERAL of them before one look: group A (2 steps) is seen, the expiry goes on record, groups B and C
    (4 steps each) are enqueued, then ONE losses_group().  All eight updates were skipped: eight optimiser steps are taken back (Adam's bias
    corrections and the Philox step key follow the device again), C is repeated from the stepper's own buffers, B's batches are gone — the
    state of a run that stepped on A and then on C.
    (Before the ledger the fallback branch took back C's four steps only: tA = tB = 10, and every later step ran with the wrong bias corrections
    and mask noise.)"""
    from gptst_amd import _C
    fresh, srcs, orders = _handoff_case(960)
    A, B_, C = slice(0, 2), slice(2, 6), slice(6, 10)
    lib = _C.lib()
    try:
        m0, s0 = fresh(group_fails=True)
        s0.step_group(srcs[A], 5, list_cs=orders[A]); s0.losses_group()
        s0.step_group(srcs[C], 5, list_cs=orders[C]); l0 = s0.losses_group()
        m1, s1 = fresh(group_fails=True)
        s1.step_group(srcs[A], 5, list_cs=orders[A]); s1.losses_group()
        torch.cuda.synchronize()
        lib.call("gptst_handoff_inject", 1)
        s1.step_group(srcs[B_], 5, list_cs=orders[B_])
        s1.step_group(srcs[C], 5, list_cs=orders[C])
        l1 = s1.losses_group()
        assert s1.safe_mode and s1.lost_steps == 8 and s1.lost_batches == 4 and (s1.tA, s1.tB) == (6, 6)
        assert len(l1) == 4
        _assert_same_state((m1, s1, l1), (m0, s0, l0))
    finally:
        lib.call("gptst_handoff_reset")


def test_lost_handoff_in_a_fallen_back_group_whose_caller_reuses_its_tensors():
    """step_group() promises that the caller's tensors are free once it returns — also when the group runs as single steps: the batches are
    repeated from the stepper's own buffers, not from tensors the caller has overwritten (stream-ordered behind the steps) in the meantime."""
    from gptst_amd import _C
    fresh, srcs, orders = _handoff_case(980)
    lib = _C.lib()
    try:
        m0, s0 = fresh(group_fails=True)
        s0.step_group(srcs[:4], 5, list_cs=orders[:4]); l0 = s0.losses_group()
        m1, s1 = fresh(group_fails=True)
        mine = [t.clone() for t in srcs[:4]]
        torch.cuda.synchronize()
        lib.call("gptst_handoff_inject", 1)
        s1.step_group(mine, 5, list_cs=orders[:4])
        for t in mine:
            t.zero_()
        l1 = s1.losses_group()
        assert s1.safe_mode and s1.lost_steps == 4 and s1.lost_batches == 0
        _assert_same_state((m1, s1, l1), (m0, s0, l0))
    finally:
        lib.call("gptst_handoff_reset")


def test_step_group_falls_back_to_single_steps_when_the_capture_fails(monkeypatch):
    """A runtime that cannot record K steps in one graph (e.g. collectives) raises at capture time: the group then runs as K single steps —
    counters not advanced twice, later groups do not retry — and gives the results of K step() calls."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = _args()
    sd = O.init_state_dict(args, 2)
    srcs = [synth.make_batch(4, 12, 20, 1, seed=950 + i).to(DEV) for i in range(4)]
    outs = []
    for broken in (False, True):
        model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
        st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=4, use_graph=True, deterministic=True)
        if broken:
            def boom(*a, **k):
                raise RuntimeError("operation not permitted when stream is capturing")
            monkeypatch.setattr(st, "_capture_group", boom)
        st.step_group(srcs, 2)
        st.step_group(srcs, 2)
        assert st.tA == 8 and bool(getattr(st, "_group_failed", False)) == broken
        outs.append((model.flat.clone(), st.losses(), st.losses_group()))
    assert outs[0][1] == outs[1][1]
    assert torch.equal(outs[0][0], outs[1][0])
    # the fallback reports one loss triple PER STEP, like the grouped path (the trainer's epoch average and best-model selection use them)
    assert len(outs[1][2]) == 4 and outs[0][2] == outs[1][2]


def test_weight_trajectory_is_as_close_to_fp64_as_the_fp32_oracle(parity):
    """r04 (replaces the rel-L2 < 0.1 weight bound of test_step_sequence_vs_reference as THE trajectory check): the same 12 optimiser steps
    (6 random-mask, 6 adaptive-mask + KL; every mask teacher-forced from the fp64 run so that no argmax flip separates the runs) are taken
    by the oracle in fp64, by the oracle in fp32 and by the HIP stepper.  Adam at lr 3e-3 amplifies round-off, so no fp32 implementation
    tracks another one tightly — but both fp32 runs must sit at the SAME distance from the fp64 trajectory: a 5 % optimiser or gradient
    error would put the HIP run orders of magnitude further out than the fp32 oracle is."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    args = _args()
    sd = O.init_state_dict(args, 11)
    K, B = 12, 4
    M = B * 12 * 20
    srcs = [synth.make_batch(B, 12, 20, 1, seed=700 + i, start_slot=13 * i) for i in range(K)]
    epochs = [1] * 6 + [20] * 6

    def inj(i, dt):
        if epochs[i] <= args.change_epoch:
            return dict(noise=synth.make_noise(M, 70 + i).to(dt))
        return dict(noise_a=synth.make_noise(M, 70 + i).to(dt), noise_r=synth.make_noise(M, 170 + i).to(dt), list_c=synth.class_order(5, 7 + i))

    st64 = O.Stepper({k: v.double() for k, v in sd.items()}, args, synth.SCALER_MEAN, synth.SCALER_STD)
    masks, l64 = [], []
    for i in range(K):
        r = st64.step(srcs[i].double(), epochs[i], **inj(i, torch.float64))
        masks.append((1 - r[3][2]).float().contiguous())           # 1 = visible
        l64.append(r[:3])
    st32 = O.Stepper(sd, args, synth.SCALER_MEAN, synth.SCALER_STD)
    l32 = [st32.step(srcs[i], epochs[i], forced_mask=masks[i])[:3] for i in range(K)]
    model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
    st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B, use_graph=True, deterministic=True)
    lh = []
    for i in range(K):
        st.step(srcs[i].to(DEV), epochs[i], forced_mask=masks[i].to(DEV))
        lh.append(st.losses())
    got = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    trained = [k for k, v in st64.sd.items() if v.requires_grad and v.grad is not None and not k.startswith("decoder.time_feature")]
    cat = lambda d: torch.cat([d[k].detach().double().reshape(-1) for k in trained])          # noqa: E731
    w64, w32, wh = cat(st64.sd), cat(st32.sd), cat(got)
    d32 = float((w32 - w64).norm() / w64.norm())
    dh = float((wh - w64).norm() / w64.norm())
    moved = float((w64 - cat({k: v.double() for k, v in sd.items()})).norm() / w64.norm())
    import os
    if os.environ.get("GPTST_TRAJ_DEBUG"):
        rows = []
        for k in trained:
            a, b, c = st64.sd[k].detach().double(), st32.sd[k].detach().double(), got[k]
            rows.append((float((c - a).norm()), float((b - a).norm()), float(a.norm()), float((a - sd[k].double()).norm()), k))
        for r in sorted(rows, reverse=True)[:25]:
            print("%-55s |hip-64| %.3e  |o32-64| %.3e  |w| %.3e  moved %.3e" % (r[4], r[0], r[1], r[2], r[3]))
        for i in range(K):
            print("step %d loss64 %.8f o32 %.3e hip %.3e" % (i, l64[i][0], abs(l32[i][0] - l64[i][0]) / abs(l64[i][0]), abs(lh[i][0] - l64[i][0]) / abs(l64[i][0])))
    parity("traj_fp32oracle_vs_fp64", d32)
    parity("traj_hip_vs_fp64", dh)
    parity("traj_hip_over_fp32oracle", dh / max(d32, 1e-12))
    assert moved > 50 * max(dh, d32), (moved, dh, d32)                 # the 12 steps moved the weights far more than the runs differ
    # The yardstick (no literal multiple): how far do VALID fp32 runs of these 12 steps land from the fp64 trajectory?  Adam normalises
    # per element, so the 1e-7-of-max rounding of a weight gradient is a 10 % change of the update of its smallest elements, and one run is one draw of a
    # lottery: the fp32 oracle itself reads 4.9e-7 on one host and 2.0e-5 on another (its reductions split by thread count).  The draws are taken HERE, from
    # the oracle: its two associations of the cap algebra, the batch in other sample orders (every sum over the batch re-associated), and initial states one
    # ulp apart — the size two fp32 implementations of one forward differ by.  The HIP run must not be further out than 1.5x the worst of them; an optimiser
    # or gradient defect is (r04: 1.55e-4, 317x the oracle, when Adam formed 1 - beta2 in fp32) — GPTST_TRAJ_DEBUG=1 lists the tensors.
    def o32(sd0, m5d=True, perm=None):
        so = O.Stepper(sd0, args, synth.SCALER_MEAN, synth.SCALER_STD, materialize_5d=m5d)
        for i in range(K):
            s_, m_ = srcs[i], masks[i]
            if perm is not None:
                s_, m_ = s_[perm].contiguous(), m_.view(B, -1)[perm].reshape(m_.shape).contiguous()
            so.step(s_, epochs[i], forced_mask=m_)
        return float((cat(so.sd) - w64).norm() / w64.norm())
    gen = torch.Generator().manual_seed(5)
    draws = [d32, o32(sd, m5d=False)] + [o32(sd, perm=torch.tensor(p_)) for p_ in ([1, 0, 3, 2], [3, 2, 1, 0], [2, 3, 0, 1])]
    for _ in range(5):
        sdp = {k_: (torch.nextafter(v_, v_ + (torch.randint(0, 2, v_.shape, generator=gen) * 2 - 1).to(v_.dtype)) if v_.is_floating_point() else v_)
               for k_, v_ in sd.items()}
        draws.append(o32(sdp))
    print("fp32 oracle draws (distance to the fp64 trajectory): %s; HIP %.2e" % (["%.2e" % v_ for v_ in draws], dh))
    parity("traj_hip_over_worst_fp32_draw", dh / max(draws))
    assert dh <= 1.5 * max(draws), (dh, draws)                          # HIP is as close to the fp64 trajectory as valid fp32 runs are
    # losses: the fp32 runs against fp64, step by step — the HIP run within twice the fp32 oracle's own deviation (+ 2e-6 floor)
    for i in range(K):
        e32 = abs(l32[i][0] - l64[i][0]) / abs(l64[i][0])
        eh = abs(lh[i][0] - l64[i][0]) / abs(l64[i][0])
        assert eh <= 3.0 * e32 + 2e-6, (i, eh, e32)


def test_handoff_soak_with_a_second_process_on_the_same_gpu():
    """the in-launch hand-offs (hyperTem backward pairs, cross-time role) under GPU sharing — a second PROCESS keeps the same GPU
    busy (time slicing between processes is what made the 0.25 s bound of round 4 expire) while this one enqueues 2000 graph replays of the step at
    the bench shape.  Either no bounded wait expires, or the stepper recovers (lost steps re-run without hand-off launches): the weights stay finite
    and no expiry is left on record."""
    import ctypes
    import os
    import subprocess
    import sys
    import time
    from gptst_amd import _C
    from gptst_amd.model import GPTST_Model, init_seed, xavier_init_
    from gptst_amd.step import PretrainStep
    args = make_args("PEMS08", scaler_zeros=synth.scaler_zeros(), device=DEV)
    init_seed(args.seed)
    B, T, N = 32, 12, args.num_nodes
    model = xavier_init_(GPTST_Model(args)).to(DEV)
    st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B, use_graph=True, seed=7)
    src = synth.make_batch(B, T, N, args.input_base_dim, interval=args.interval, seed=2024).to(DEV)
    hog = subprocess.Popen([sys.executable, "-c",
                            "import torch,time\n"
                            "a=torch.randn(8192,8192,device='cuda:0');t=time.time()\n"
                            "while time.time()-t<60:\n"
                            "    for _ in range(20): b=a@a\n"
                            "    torch.cuda.synchronize()\n"], env=dict(os.environ))
    try:
        time.sleep(8.0)                                  # let the other process get onto the GPU
        K, lib = 4, _C.lib()
        srcs = st.group_sources(K)
        for s_ in srcs:
            s_.copy_(src)
        nrep = 500                                       # x K = 2000 steps, one graph replay each group of four
        for r in range(nrep):
            st.step_group(srcs, 200)
            if r % 50 == 49:
                ls = st.losses_group()                   # sync + recovery point, as the trainer's logging is
                assert all(l[0] == l[0] and l[0] > 0 for l in ls), ls
        ls = st.losses_group()
        torch.cuda.synchronize()
        n = ctypes.c_int(-1)
        lib.call("gptst_handoff_timeouts", ctypes.byref(n))
        assert bool(torch.isfinite(model.flat).all()), "weights went non-finite"
        assert n.value == 0, "an expiry is still on record after the last recovery point"
        print("soak: %d steps, lost (re-run) steps %d, safe_mode %s" % (st.tA, st.lost_steps, st.safe_mode))
        assert st.tA == nrep * K
    finally:
        hog.kill()
        hog.wait()
        _C.lib().call("gptst_handoff_reset")
