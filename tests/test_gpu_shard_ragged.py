"""Node shards of unequal width (gpt-st_amd/shard.py node_ranges, model.py node_capacity): ranks emulated by threads on this GPU must
reproduce the unsharded step — same global masks (bit exact), same losses, same parameter update — with the protocol of
tests/test_gpu_shard.py::test_node_shards_equal_unsharded_step; and the forward-only evaluation of a sharded run (ShardedPretrainStep.evaluate,
Trainer.test in shard mode) must report what the unsharded Trainer.test reports."""
import logging
import threading

import pytest
import torch

from gptst_amd import synth
from gptst_amd.config import make_args
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SMALL = dict(embed_dim=8, HS=5, HT=6)
CONFIG4 = dict(hidden_dim=128)              # BASELINE configs[4] dims: C = 128
CLIP = 0.5                                  # max_grad_norm of the parity steps: below every step's gradient norm, so that the clip acts


def _args(n, over=SMALL, **kw):
    return make_args("PEMS08", num_nodes=n, num_route=2, scaler_zeros=synth.scaler_zeros(), epochs=30, change_epoch=3, **over, **kw)


def _threads(W, rank_main):
    """rank_main(r, group) on W threads sharing this GPU -> [result of rank r]"""
    from gptst_amd import ops
    from gptst_amd.shard import ThreadNodeGroup
    shared = ThreadNodeGroup.Shared(W)
    ops.CALL_LOCK = threading.Lock()
    out, errs = [None] * W, []

    def run(r):
        try:
            out[r] = rank_main(r, ThreadNodeGroup(r, shared))
        except BaseException as e:              # noqa: BLE001 - surface the failure in the main thread
            errs.append(e)
            shared.barrier.abort()

    try:
        ths = [threading.Thread(target=run, args=(r,)) for r in range(W)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(900)
    finally:
        ops.CALL_LOCK = None
    assert not errs, errs
    return out


def _local_model(sd, N, W, r, over, **kw):
    from gptst_amd.model import GPTST_Model
    from gptst_amd.shard import node_ranges, shard_state_dict
    ranges = node_ranges(N, W)
    n0, n1 = ranges[r]
    args_l = _args(n1 - n0, over, node_capacity=max(b - a for a, b in ranges), **kw)
    m = GPTST_Model(args_l)
    m.load_state_dict(shard_state_dict(sd, n0, n1))
    return m.to(DEV), args_l, (n0, n1), ranges


@pytest.mark.parametrize("W,N,B,over", [(8, 170, 2, SMALL), (3, 40, 2, SMALL), (3, 1000, 1, CONFIG4)],
                         ids=["w8_n170", "w3_n40", "w3_n1000_c128"])
def test_unequal_node_shards_equal_unsharded_step(W, N, B, over, parity, monkeypatch):
    """170 over 8 ranks: shards of 22 and 21 nodes (PEMS08's node count); 40 over 3: 14, 13, 13; 1000 over 3 at C = 128: 334, 333, 333.
    The gradient is clipped in every step (max_grad_norm = CLIP): a rank whose clip norm saw other values than its peers' would move the shared
    parameters differently.  Besides the unsharded comparison, every rank's shared parameters must agree, and the node_capacity padding of the
    narrower ranks must still be zero in weights, Adam moments and gradient."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.shard import ShardedPretrainStep, is_node_local, unshard_state_dicts
    from gptst_amd.step import PretrainStep
    monkeypatch.setenv("GPTST_DETERMINISTIC", "1")
    args_g = _args(N, over, max_grad_norm=CLIP)
    sd = O.init_state_dict(args_g, 5)
    Mg = B * 12 * N
    steps = [(1, 0), (20, 1), (25, 2)]                     # (epoch, seed): random phase, then adaptive + KL twice
    srcs = [synth.make_batch(B, 12, N, 1, seed=40 + s).to(DEV) for _, s in steps]
    noise = [tuple(synth.make_noise(Mg, 10 * s + i).to(DEV) for i in range(3)) for _, s in steps]
    list_c = synth.class_order(args_g.HS, 9)

    model = GPTST_Model(args_g); model.load_state_dict(sd); model = model.to(DEV)
    st = PretrainStep(model, args_g, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B, use_graph=False)
    ref_loss, ref_mask = [], []
    for (epoch, _), src, (n0, na, nr) in zip(steps, srcs, noise):
        st.step(src, epoch, noise=n0, noise_a=na, noise_r=nr, list_c=list_c)
        ref_loss.append(st.losses()); ref_mask.append(st.last_mask.clone())
    ref_sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    del st, model

    def rank_main(r, group):
        m, args_l, (a, b), _ = _local_model(sd, N, W, r, over, max_grad_norm=CLIP)
        s = ShardedPretrainStep(m, args_l, N, group, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B)
        assert (s.n0, s.n1) == (a, b)
        losses, masks, gnorms = [], [], []
        for (epoch, _), src, (n0, na, nr) in zip(steps, srcs, noise):
            s.step(src[:, :, a:b].contiguous(), epoch, noise=n0, noise_a=na, noise_r=nr, list_c=list_c)
            losses.append(s.losses()); masks.append(s.last_mask_global.clone())
            gnorms.append(float(s.stats_out[4]) ** 0.5)                  # the global gradient norm the optimiser clipped with
        torch.cuda.synchronize()
        pad = torch.ones(m.flat.numel(), dtype=torch.bool, device=DEV)    # elements no parameter owns: capacity padding, alignment
        for k, t in m.named_parameters():
            pad[m._offs[k]:m._offs[k] + t.numel()] = False
        npad = sum(m._slot_numel[k] - t.numel() for k, t in m.named_parameters())
        padmax = max(float(x[pad].abs().max()) if bool(pad.any()) else 0.0 for x in (m.flat, s.m, s.v, s.gflat))
        return (losses, masks, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, gnorms, npad, padmax)

    out = _threads(W, rank_main)
    got_sd = unshard_state_dicts([out[r][2] for r in range(W)])
    assert all(min(o[3]) > CLIP for o in out), [o[3] for o in out]         # clipped in every step
    assert sum(1 for o in out if o[4] > 0) == W - (N % W or W), [o[4] for o in out]   # the narrower ranks carry capacity padding ...
    assert all(o[5] == 0.0 for o in out), [o[5] for o in out]             # ... and it is zero in weights, m, v and gradient
    shared_diff = max(float((out[r][2][k] - out[0][2][k]).abs().max()) for r in range(1, W) for k in out[0][2] if not is_node_local(k))
    parity("shared_param_max_abs_diff_across_ranks", shared_diff)
    assert shared_diff <= 1e-6, shared_diff
    parity("clip_norm_over_max_grad_norm_min", min(min(o[3]) for o in out) / CLIP)
    worst_loss = 0.0
    for i in range(len(steps)):
        for r in range(W):
            assert torch.equal(out[r][1][i], ref_mask[i]), "global mask differs at step %d on rank %d" % (i, r)
            for a, b in zip(out[r][0][i], ref_loss[i]):
                worst_loss = max(worst_loss, abs(a - b) / max(abs(b), 1e-3))
                assert abs(a - b) <= 2e-4 * max(abs(b), 1e-3), (i, r, out[r][0][i], ref_loss[i])
    parity("loss_rel", worst_loss)
    worst = worst_raw = 0.0
    for k, v in ref_sd.items():
        if not v.dtype.is_floating_point:
            continue
        assert got_sd[k].shape == v.shape, k
        upd = v - sd[k]
        d = (got_sd[k] - v).abs().flatten()
        err = float(d.norm() / upd.norm().clamp_min(1e-6))
        worst_raw = max(worst_raw, err)
        worst = max(worst, err if not k.endswith(".t_adj") else 0.0)
        assert float(d.max()) <= 2.5 * args_g.lr_init, "%s: element update off by %.3e (lr %.1e)" % (k, float(d.max()), args_g.lr_init)
        assert err < (4e-3 if k.endswith(".t_adj") else 1.5e-3), "%s: update differs, rel-L2 of the update error %.3e" % (k, err)
    parity("update_rel_l2_worst", worst)
    parity("update_rel_l2_worst_incl_t_adj", worst_raw)


def test_sharded_evaluation_equals_unsharded_trainer_test(tmp_path, parity):
    """W = 3, N = 40 (shards 14, 13, 13), batches of 2 and 1 samples: evaluate() gives the unsharded forward's output and visibility mask on
    this rank's columns, and Trainer.test in shard mode (per-node sums in this rank's rows, ONE group all-reduce) reports the unsharded rows."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.trainer import Trainer
    W, N = 3, 40
    args_g = _args(N)
    args_g.log_dir = str(tmp_path)
    sd = O.init_state_dict(args_g, 6)
    epoch = args_g.epochs                                   # Trainer.test evaluates at the last epoch: adaptive masks
    sizes = (2, 1)
    srcs = [synth.make_batch(b, 12, N, 1, seed=70 + j, start_slot=11 * j).to(DEV) for j, b in enumerate(sizes)]
    inj = [dict(noise_a=synth.make_noise(b * 12 * N, 200 + j).to(DEV), noise_r=synth.make_noise(b * 12 * N, 300 + j).to(DEV),
                list_c=synth.class_order(args_g.HS, 400 + j)) for j, b in enumerate(sizes)]

    model = GPTST_Model(args_g); model.load_state_dict(sd); model = model.to(DEV)
    ref_out = []
    with torch.no_grad():
        for src, kw in zip(srcs, inj):
            model.set_mask_inputs(**kw)
            out, _, masked, _, _ = model(src, None, None, epoch)
            ref_out.append((out.clone(), (1 - masked).to(torch.float32)))
    tr = Trainer(model, args_g, lambda e: [], synth.SCALER_MEAN, synth.SCALER_STD, batch_size=2)
    tr.logger.setLevel(logging.WARNING)

    def injected():
        for src, kw in zip(srcs, inj):
            model.set_mask_inputs(**kw)
            yield src
    ref_rows = tr.test(injected())
    del tr, model

    def rank_main(r, group):
        m, args_l, (a, b), ranges = _local_model(sd, N, W, r, SMALL)
        args_l.log_dir = str(tmp_path)
        t = Trainer(m, args_l, lambda e: [], synth.SCALER_MEAN, synth.SCALER_STD, batch_size=2, shard=(group, ranges))
        res = []
        for src, kw in zip(srcs, inj):
            out, vis = t.step.evaluate(src[:, :, a:b], epoch, **kw)
            res.append((out.clone(), vis.clone()))
        calls = iter(inj)
        plain = t.step.evaluate
        t.step.evaluate = lambda s_, ep: plain(s_, ep, **next(calls))
        rows = t.test(src[:, :, a:b].contiguous() for src in srcs)
        return (a, b), res, rows

    out = _threads(W, rank_main)
    worst_out = worst_rows = 0.0
    for (a, b), res, rows in out:
        for (o, v), (ro, rv) in zip(res, ref_out):
            assert torch.equal(v, rv[:, :, a:b]), "visibility mask differs on nodes [%d, %d)" % (a, b)
            e = float((o - ro[:, :, a:b]).abs().max() / ro.abs().max())
            worst_out = max(worst_out, e)
            assert e < 1e-4, (a, b, e)
        e = float(((rows - ref_rows).abs() / ref_rows.abs().clamp_min(1e-6)).max())
        worst_rows = max(worst_rows, e)
        assert e < 1e-4, (rows, ref_rows)
    parity("eval_out_rel", worst_out)
    parity("report_rows_rel", worst_rows)


def test_native_group_reduces_float64_without_fp32_rounding():
    """The closing report's metric sums are float64 and go through the group's all-reduce; on the C-ABI communicator (fp32 only) they travel
    as hi + lo fp32 words, one contributor per element, and keep ~48 bits (a cast to fp32 kept 24).  One rank here: the path, not the sum."""
    from gptst_amd.dist import NativeComm
    from gptst_amd.shard import NativeNodeGroup
    comm = NativeComm(rank=0, world=1)
    try:
        g = NativeNodeGroup(comm)
        x = (torch.arange(1, 4097, dtype=torch.float64, device=DEV) * (1.0 + 1e-9)) ** 2 + 1.0 / 3.0     # not representable in fp32
        t = x.clone().view(64, 64)
        g.all_reduce_(t)
        torch.cuda.synchronize()
        e = float(((t.view(-1) - x).abs() / x).max())
        assert e < 1e-13, e
    finally:
        comm.close()
