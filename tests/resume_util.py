"""Shared by tests/test_resume_cpu.py and tests/test_gpu_resume.py: the smallest shapes that reach every route of a resumed run, steppers on
one GPU or on thread-emulated node shards, and the comparisons of two runs (bit-exact, or the bounds tests/test_gpu_shard.py holds a sharded
run to against the unsharded one)."""
import io
import threading

import torch

from gptst_amd import synth
from gptst_amd.config import make_args

DEV = "cuda:0"
B, T = 2, 12
EPOCHS = (1, 1, 1, 3, 3, 3, 3, 3)                # change_epoch = 2: tB grows and the class-order stream is consumed from the fourth step on


def small_args(n, **kw):
    over = dict(num_route=2, embed_dim=8, HS=5, HT=6, epochs=8, change_epoch=2, scaler_zeros=synth.scaler_zeros())
    over.update(kw)
    return make_args("PEMS08", num_nodes=n, **over)


def init_sd(args, seed=5):
    from oracle import gptst_oracle as O
    return O.init_state_dict(args, seed)


def batches(n, count, dev=DEV):
    return [synth.make_batch(B, T, n, 1, seed=40 + i, start_slot=7 * i).to(dev) for i in range(count)]


def through_buffer(sd):
    """torch.save / torch.load through memory, as a file would carry it"""
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, map_location="cpu", weights_only=True)


def same_tree(a, b):
    """nested dicts / sequences equal, tensors by torch.equal"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_tree(x, y) for x, y in zip(a, b))
    return a == b


# ---- one GPU ----------------------------------------------------------------------------------------------------------------------
def new_stepper(args, sd, use_graph=False, deterministic=True):
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(DEV)
    return PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B, use_graph=use_graph, deterministic=deterministic)


def snapshot(st):
    """what two runs that are 'the same run' must agree on, bit for bit"""
    loss = st.losses()
    return dict(flat=st.model.flat.detach().cpu().clone(), m=st.m.cpu().clone(), v=st.v.cpu().clone(), mask=st.last_mask.cpu().clone(),
                loss=loss, tA=st.tA, tB=st.tB)


def assert_same_run(a, b, what=""):
    for k in ("flat", "m", "v", "mask"):
        assert torch.equal(a[k], b[k]), "%s: %s differs (max |d| %.3e)" % (what, k, float((a[k] - b[k]).abs().max()))
    assert a["loss"] == b["loss"], (what, a["loss"], b["loss"])
    assert (a["tA"], a["tB"]) == (b["tA"], b["tB"]), (what, a["tA"], a["tB"], b["tA"], b["tB"])


# ---- thread-emulated node shards ---------------------------------------------------------------------------------------------------
def run_ranks(W, rank_main):
    """rank_main(r, group) on W threads sharing this GPU, each with the library's fixed-order reductions on (the sharded stepper has no switch of
    its own, and the launch mode is per thread) -> [result of rank r]"""
    from gptst_amd import ops
    from gptst_amd.shard import ThreadNodeGroup
    shared = ThreadNodeGroup.Shared(W)
    ops.CALL_LOCK = threading.Lock()
    out, errs = [None] * W, []

    def run(r):
        try:
            ops.set_deterministic(True)
            out[r] = rank_main(r, ThreadNodeGroup(r, shared))
        except BaseException as e:              # noqa: BLE001 - surface the failure in the main thread
            errs.append(e)
            shared.barrier.abort()
        finally:
            ops.set_deterministic(False)

    try:
        ths = [threading.Thread(target=run, args=(r,)) for r in range(W)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(600)
    finally:
        ops.CALL_LOCK = None
    assert not errs, errs
    return out


def local_stepper(sd, N, W, r, group):
    """rank r's model (its node range of the global `sd`, node_capacity = the widest shard) and stepper"""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.shard import ShardedPretrainStep, node_ranges, shard_state_dict
    ranges = node_ranges(N, W)
    n0, n1 = ranges[r]
    args_l = small_args(n1 - n0, node_capacity=max(b - a for a, b in ranges))
    m = GPTST_Model(args_l)
    m.load_state_dict(shard_state_dict(sd, n0, n1))
    m = m.to(DEV)
    return ShardedPretrainStep(m, args_l, N, group, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B), (n0, n1)


def padding_max(st):
    """largest |value| in what no parameter owns (capacity padding, alignment) of the weights and both moments, and how many such elements"""
    m = st.model
    pad = torch.ones(m.flat.numel(), dtype=torch.bool, device=m.flat.device)
    for k, t in m.named_parameters():
        pad[m._offs[k]:m._offs[k] + t.numel()] = False
    npad = sum(m._slot_numel[k] - t.numel() for k, t in m.named_parameters())
    worst = max(float(x[pad].abs().max()) for x in (m.flat, st.m, st.v)) if bool(pad.any()) else 0.0
    return worst, npad


def shard_snapshot(st):
    loss = st.losses()
    torch.cuda.synchronize()
    return dict(flat=st.model.flat.detach().cpu().clone(), m=st.m.cpu().clone(), v=st.v.cpu().clone(), mask=st.last_mask_global.cpu().clone(),
                loss=loss, tA=st.tA, tB=st.tB, sd={k: v.detach().cpu().clone() for k, v in st.model.state_dict().items()})


def assert_within_shard_bounds(got_sd, ref_sd, sd0, lr_init, what=""):
    """tests/test_gpu_shard.py's bounds on a sharded run against the unsharded one: per tensor, the error of the update under 1.5e-3 of the
    update's norm (cap*.t_adj 4e-3), no element off by more than 2.5 x lr_init"""
    for k, v in ref_sd.items():
        if not v.dtype.is_floating_point:
            continue
        assert got_sd[k].shape == v.shape, (what, k)
        upd = v - sd0[k]
        d = (got_sd[k] - v).abs().flatten()
        err = float(d.norm() / upd.norm().clamp_min(1e-6))
        assert float(d.max()) <= 2.5 * lr_init, "%s %s: element update off by %.3e (lr %.1e)" % (what, k, float(d.max()), lr_init)
        assert err < (4e-3 if k.endswith(".t_adj") else 1.5e-3), "%s %s: update differs, rel-L2 of the update error %.3e" % (what, k, err)


def assert_losses_close(a, b, what=""):
    for x, y in zip(a, b):
        assert abs(x - y) <= 2e-4 * max(abs(y), 1e-3), (what, a, b)
