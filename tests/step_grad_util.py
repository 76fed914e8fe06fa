"""Helpers of the fused step's gradient checks (tests/test_gpu_step_grads.py, tests/test_gpu_kl_carried.py, tests/test_step_grad_compare_cpu.py):
one fused PretrainStep with its gradient views kept, the same step through the oracle's autograd in a chosen precision, and the comparator.

What PretrainStep.g holds after a step: on path A (the reconstruction loss; flat offsets [0, nA)) the gradient of the SUM loss — the optimiser
divides it by the kept count in stats_out[1] (hyper[9]); on path B (the KL term; [nA, nA + nB)) the gradient as it is, 0.1 weight applied; behind
that the decoder's never-trained time features, which stay zero."""
import time

import torch

from gptst_amd import synth
from oracle import gptst_oracle as O

GRAD_TOL = 1e-4          # the project's whole-model gradient bound (tests/test_gpu_shapes.py)
ORC_FACTOR = 1.5         # past it: no further from the fp64 oracle than 1.5x the fp32 oracle's own distance (same file)
SRC_SEED = 11


def make_src(args, B, seed=SRC_SEED):
    return synth.make_batch(B, args.lag, args.num_nodes, args.input_base_dim, interval=getattr(args, "interval", 5), seed=seed)


def noise_inject(args, B, epoch, seeds=(21, 22, 23, 4)):
    """the injected mask inputs of one step on the CPU: random phase noise=, adaptive phase noise_a= / noise_r= / list_c="""
    M = B * args.lag * args.num_nodes
    if epoch <= args.change_epoch:
        return dict(noise=synth.make_noise(M * args.input_base_dim, seeds[0]))
    return dict(noise_a=synth.make_noise(M, seeds[1]), noise_r=synth.make_noise(M, seeds[2]), list_c=synth.class_order(args.HS, seeds[3]))


def one_step(args, B, epoch, *, deterministic=False, safe_mode=False, use_graph=False, sd_seed, inject, src=None, dev="cuda:0"):
    """one fused step from the seed-`sd_seed` state -> (gradient views cloned, stats_out, mask, launch names, stepper).
    Two steps are taken from the same weights (state dict reloaded, m and v zeroed in between): the first sizes the zero arena, the second is
    the one returned, with ops.TIMER recording its launches (none under use_graph: a replay enqueues nothing through ops).
    inject: noise= | noise_a= / noise_r= / list_c= | forced_mask= (1 = visible), CPU tensors."""
    from gptst_amd import ops
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    sd = O.init_state_dict(args, sd_seed)
    model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(dev)
    st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B, use_graph=use_graph, deterministic=deterministic)
    if safe_mode:
        st.safe_mode = True                          # _part2 under engine.no_handoffs()
    src = (make_src(args, B) if src is None else src).to(dev)
    inj = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inject.items()}
    names = None
    try:
        for i in range(2):                           # the first step sizes the zero arena; the second is the one compared
            ops.TIMER = [] if i == 1 else None
            st.step(src, epoch, **inj)
            if i == 1:
                names = [r[0] for r in ops.TIMER]
            ops.TIMER = None
            torch.cuda.synchronize()
            if i == 0:
                model.load_state_dict(sd)            # (the second step starts from the same weights)
                st.m.zero_(); st.v.zero_()
    finally:
        ops.TIMER = None
    grads = {k: v.detach().clone() for k, v in st.g.items()}
    return grads, st.stats_out.clone(), st.last_mask.clone(), names, st


def kept_count(args, src, visible):
    """cells the masked MAE averages over, in fp32 as the loss computes them: masked cells (1 - visible) whose de-normalised label exceeds mape_thresh"""
    base = args.input_base_dim
    lm = 1.0 - visible.reshape(src.shape[:3] + (base,)).to(torch.float32)
    y = (src[..., :base].float() * synth.SCALER_STD + synth.SCALER_MEAN) * lm
    return int((y > args.mape_thresh).sum())


def oracle_grads(args, sd, src, epoch, inject, dtype):
    """the same step's loss through the oracle's forward and torch autograd in `dtype` (no clipping: O.Stepper.step would clip .grad in place)
    -> ({key: gradient or None}, (loss, loss_flow, loss_s), final mask (B,T,N,base) float32 with 1 = visible, kept count)"""
    cast = lambda v: v.to(dtype) if torch.is_tensor(v) and v.dtype.is_floating_point else v      # noqa: E731
    st = O.Stepper({k: cast(v) for k, v in sd.items()}, args, synth.SCALER_MEAN, synth.SCALER_STD, materialize_5d=False)
    srcd = cast(src)
    outs, aux = O.forward_pretrain(st.sd, args, srcd, epoch, materialize_5d=False, **{k: cast(v) for k, v in inject.items()})
    loss, lf, ls = O.pretrain_loss(outs, srcd, args, epoch, synth.SCALER_MEAN, synth.SCALER_STD)
    loss.backward()
    grads = {k: (v.grad.detach() if torch.is_tensor(v) and v.requires_grad and v.grad is not None else None) for k, v in st.sd.items()
             if not k.endswith("mask_template")}
    final = aux["final_mask"].to(torch.float32).contiguous()
    label = srcd[..., :args.output_dim]
    y = (label * synth.SCALER_STD + synth.SCALER_MEAN) * outs[2]
    return grads, tuple(float(v.detach()) for v in (loss, lf, ls)), final, int((y > args.mape_thresh).sum())


def layout_of(args):
    """(model._offs, nA, nB) of the flat parameter buffer (built on the CPU: no kernel runs)"""
    from gptst_amd.model import GPTST_Model
    m = GPTST_Model(args)
    return dict(m._offs), int(m.nA), int(m.nB)


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def compare(got, stats_out, ref64, ref32_fn, record, layout):
    """Every tensor of a step's gradient views `got` against the fp64 oracle's gradients `ref64` -> {key: (e_hip, e_orc)} of the tensors that
    passed only under the fp32-oracle allowance; raises AssertionError naming every tensor that failed.
    Path A tensors are divided by the kept count stats_out[1] first, path B tensors are taken as stored (module docstring); the path of a key
    is read from the flat layout (`layout` = layout_of(args)).  A parameter without an oracle gradient must be exactly zero.
    Per tensor e = max|a - b| / max|b| < GRAD_TOL; past it the tensor passes only if e <= 1.5 x the fp32 oracle's own distance to fp64
    (ref32_fn() -> its gradients, called at most once and only then).  record(key, value) gets every e."""
    offs, nA, nB = layout
    cnt = max(float(stats_out[1]), 1.0)
    ref32, allowed, bad = None, {}, []
    for k, g in got.items():
        g = g.detach().cpu().double()
        r = ref64.get(k)
        if r is None:
            if float(g.abs().max()) != 0.0:
                bad.append((k, "no oracle gradient, but max|g| = %.3e" % float(g.abs().max())))
            continue
        o = offs[k]
        if o < nA:
            a = g / cnt
        elif o < nA + nB:
            a = g
        else:
            bad.append((k, "an oracle gradient on a never-trained parameter"))
            continue
        if a.shape != r.shape:
            bad.append((k, "shape %s against %s" % (tuple(a.shape), tuple(r.shape))))
            continue
        e = rel(a, r)
        record("grad:" + k, e)
        if e < GRAD_TOL:
            continue
        if ref32 is None:
            ref32 = ref32_fn()
        e_orc = rel(ref32[k], r)
        record("grad_oracle32:" + k, e_orc)
        if e <= ORC_FACTOR * e_orc:
            allowed[k] = (e, e_orc)
        else:
            bad.append((k, "e_hip %.3e, e_orc %.3e" % (e, e_orc)))
    missing = [k for k, r in ref64.items() if r is not None and k not in got]
    assert not missing, ("oracle gradients without a view in the step", missing)
    assert not bad, bad
    return allowed


def grad_norm(ref):
    """the norm clip_grad_norm_ would see: over every oracle gradient"""
    return float(torch.sqrt(sum((v.double() ** 2).sum() for v in ref.values() if v is not None)))


# ---- the case table of tests/test_gpu_step_grads.py ---------------------------------------------------------------------------------
_SCHED = dict(epochs=30, change_epoch=3)        # the schedule tests/test_gpu_kl_carried.py steps under: epoch 1 random, epoch 20 adaptive
_SMALL = dict(num_nodes=24, embed_dim=8, HS=6, HT=8)
CASES = {
    # the benchmark shape: carried KL, hyperTem pairs and the cross-time role all on
    "bench_rand": dict(ds="PEMS08", over=_SCHED, B=32, epoch=1),
    "bench_ada": dict(ds="PEMS08", over=_SCHED, B=32, epoch=20),
    # ada_type 'half'; HS * N is not a multiple of 4
    "metr_la": dict(ds="METR_LA", over={}, B=8, epoch=200),
    # base = 2: encin_ok is false, mape_thresh 0.001, two channels through tail_mae
    "nyc_taxi_rand": dict(ds="NYC_TAXI", over={}, B=4, epoch=3),
    "nyc_taxi_ada": dict(ds="NYC_TAXI", over={}, B=4, epoch=150),
    # HS = 20: fused_tails_ok is false — the unfused loss kernels, no carried KL
    "hs20": dict(ds="PEMS08", over=dict(HS=20, num_nodes=45), B=2, epoch=100),
    # the capsule matrix beyond LDS: the streaming cap inside the step
    "n600": dict(ds="PEMS08", over=dict(num_nodes=600, embed_dim=8), B=1, epoch=100),
    # the C = 128 forms of the dPre chain
    "n260_c128": dict(ds="PEMS08", over=dict(num_nodes=260, hidden_dim=128, embed_dim=8), B=1, epoch=100),
    # small ragged tiles
    "small_rand": dict(ds="PEMS08", over=dict(_SCHED, **_SMALL), B=2, epoch=1),
    "small_ada": dict(ds="PEMS08", over=dict(_SCHED, **_SMALL), B=2, epoch=20),
    # variants of the benchmark shape at B = 8, both phases
    "det_rand": dict(ds="PEMS08", over=_SCHED, B=8, epoch=1, step=dict(deterministic=True)),
    "det_ada": dict(ds="PEMS08", over=_SCHED, B=8, epoch=20, step=dict(deterministic=True)),
    "safe_rand": dict(ds="PEMS08", over=_SCHED, B=8, epoch=1, step=dict(safe_mode=True)),
    "safe_ada": dict(ds="PEMS08", over=_SCHED, B=8, epoch=20, step=dict(safe_mode=True)),
    "graph_rand": dict(ds="PEMS08", over=_SCHED, B=8, epoch=1, step=dict(use_graph=True)),
    "graph_ada": dict(ds="PEMS08", over=_SCHED, B=8, epoch=20, step=dict(use_graph=True)),
}
SD_SEED = 3


def case_args(name):
    from gptst_amd.config import make_args
    c = CASES[name]
    return make_args(c["ds"], **dict(dict(scaler_zeros=synth.scaler_zeros()), **c["over"]))


# ---- the scaled forms of the step: node shards (shard.py) and data parallelism (dist.py), ranks emulated by threads on one GPU -----------
# (tests/test_gpu_dist_step_grads.py; the assembling and checking code below is proven on the CPU by tests/test_dist_step_grad_compare_cpu.py)
SMALL_DIST = dict(embed_dim=8, HS=5, HT=6)      # the small dims of tests/test_gpu_shard*.py
NORM_TOL = 1e-4                                  # every rank's clip norm against the fp64 oracle's global gradient norm
# ... and against the fp64 norm of the gradient the ranks themselves hold.  That leaves only the fp32 summation of the squares: terms >= 0, no
# cancellation, so the relative error is at most (additions an element passes through) x 2^-24 — a few per thread, then trees of 64, 4, 256
# and 4 partials in clip_adam, the like in torch's sum for the shards' correction: under 40.  1e-5 is 170 roundings.  (The node-local
# gradients are 5e-5 of the squared norm at N = 40: a rank that leaves out its peers' part is 2.5e-5 .. 4e-5 off, under NORM_TOL.)
NORM_SELF_TOL = 1e-5


def dist_args(ds="PEMS08", **over):
    from gptst_amd.config import make_args
    return make_args(ds, **dict(dict(scaler_zeros=synth.scaler_zeros()), **dict(_SCHED, **over)))


def _local_args(args_global, width, capacity):
    from types import SimpleNamespace
    a = SimpleNamespace(**vars(args_global))
    a.num_nodes, a.node_capacity = width, capacity
    return a


class _Env:
    """os.environ entries set while a stepper is built and run, put back afterwards"""

    def __init__(self, env):
        self.env, self.old = dict(env or {}), {}

    def __enter__(self):
        import os
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        import os
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Names:
    """the names of the C-ABI launches enqueued while a thread has `on` set (ops.TIMER records nothing under ops.CALL_LOCK): ops._call wrapped"""

    def __init__(self):
        import threading
        self.names, self.tl = set(), threading.local()

    def __enter__(self):
        from gptst_amd import ops
        self.orig = ops._call

        def call(name, *a, **k):
            if getattr(self.tl, "on", False):
                self.names.add(name)
            return self.orig(name, *a, **k)
        ops._call = call
        return self

    def __exit__(self, *exc):
        from gptst_amd import ops
        ops._call = self.orig


def _rank_threads(W, shared, rank_main, timeout=120):
    """rank_main(r) on W threads sharing this GPU -> [result of rank r].  One C-ABI call at a time (ops.CALL_LOCK); a rank's exception aborts
    the barrier the others wait in.  All joins share ONE deadline.  A thread that outlives it may still be enqueueing launches, and nothing
    can stop a thread: the lock stays set and the process ends there, rather than go on to other tests with a rank loose on the GPU."""
    import os
    import sys
    import threading
    from gptst_amd import ops
    out, errs = [None] * W, []

    def run(r):
        try:
            out[r] = rank_main(r)
        except BaseException as e:              # noqa: BLE001 - surface the failure in the main thread
            errs.append(e)
            shared.barrier.abort()

    ops.CALL_LOCK = threading.Lock()
    try:
        ths = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(W)]
        deadline = time.monotonic() + timeout
        for t in ths:
            t.start()
        for t in ths:
            t.join(max(0.0, deadline - time.monotonic()))
        alive = [r for r, t in enumerate(ths) if t.is_alive()]
        if alive:
            shared.barrier.abort()
            for t in ths:
                t.join(5.0)                     # (ranks that only waited in the barrier end here)
            alive = [r for r, t in enumerate(ths) if t.is_alive()]
        if alive:
            print("step_grad_util: rank threads %s still run %d s after their start (errors so far: %r): ending the process"
                  % (alive, timeout + 5, errs), file=sys.stderr, flush=True)
            os._exit(70)
    finally:
        ops.CALL_LOCK = None
    assert not errs, errs
    return out


def _two_steps(st, model, sd_local, step_fn, names):
    """the protocol of one_step: the first step sizes the arena; weights reloaded, m and v zeroed; the second is the one returned, its launches named"""
    step_fn()
    torch.cuda.synchronize()
    model.load_state_dict(sd_local)
    st.m.zero_(); st.v.zero_()
    torch.cuda.synchronize()
    names.tl.on = True
    try:
        step_fn()
    finally:
        names.tl.on = False
    torch.cuda.synchronize()


def _rank_result(st, model, mask, local_keys=()):
    """what a rank leaves behind: gradient views, statistics, mask, post-step weights, and the WHOLE slot (capacity padding included) of every
    node-local key in gradient and weights"""
    res = dict(g={k: v.detach().cpu().clone() for k, v in st.g.items()}, stats=st.stats_out.detach().cpu().clone(), mask=mask.detach().cpu().clone(),
               w={k: v.detach().cpu().clone() for k, v in model.state_dict().items() if v.dtype.is_floating_point},
               kl=bool(st.tB and st.phase_kl), slots_g={}, slots_w={})
    for k in local_keys:
        o, n = model._offs[k], model._slot_numel[k]
        res["slots_g"][k] = st.gflat[o:o + n].detach().cpu().clone()
        res["slots_w"][k] = model.flat[o:o + n].detach().cpu().clone()
    return res


def sharded_one_step(args_global, W, B, epoch, *, sd_seed, inject, src, env=None, group="thread", dev="cuda:0"):
    """one ShardedPretrainStep per rank from the seed-`sd_seed` GLOBAL state -> ([per rank: dict(g, stats, mask, slots_g, slots_w, w, kl)],
    node ranges, union of the launch names of the compared step).  group "thread": W ranks as threads on this GPU over ThreadNodeGroup, shards
    from shard.node_ranges, models built at node_capacity = the widest shard.  "world1_graph": W = 1 over DistNodeGroup(0, 1), the step captured
    in a hipGraph (a replay enqueues nothing through ops).  src and the injected noise cover the GLOBAL cells."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.shard import DistNodeGroup, ShardedPretrainStep, ThreadNodeGroup, is_node_local, node_ranges, shard_state_dict
    assert group in ("thread", "world1_graph") and (group == "thread" or W == 1)
    N = args_global.num_nodes
    sd = O.init_state_dict(args_global, sd_seed)
    ranges = node_ranges(N, W)
    cap = max(b - a for a, b in ranges)
    src = src.to(dev)
    inj = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inject.items()}
    shared = ThreadNodeGroup.Shared(W)

    def rank_main(r):
        a, b = ranges[r]
        args_l = _local_args(args_global, b - a, cap)
        sd_l = shard_state_dict(sd, a, b)
        m = GPTST_Model(args_l); m.load_state_dict(sd_l); m = m.to(dev)
        if group == "thread":
            s = ShardedPretrainStep(m, args_l, N, ThreadNodeGroup(r, shared), synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B)
        else:
            s = ShardedPretrainStep(m, args_l, N, DistNodeGroup(0, 1), synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B, use_graph=True)
            assert s.shard_graph
        assert (s.n0, s.n1) == (a, b)
        mine = src[:, :, a:b].contiguous()
        _two_steps(s, m, sd_l, lambda: s.step(mine, epoch, **inj), names)
        return _rank_result(s, m, s.last_mask_global, [k for k, _ in m.named_parameters() if is_node_local(k)])

    with _Env(env), _Names() as names:
        out = _rank_threads(W, shared, rank_main) if group == "thread" else [rank_main(0)]
    return out, ranges, sorted(names.names)


class ThreadDP:
    """Stands in for dist.DataParallel between `world` threads of one process sharing one GPU stream, on ThreadNodeGroup's barrier pattern:
    a barrier separates 'everybody has enqueued its contribution' from the sum.  Every rank sums the slots in rank order, so the replicas
    receive bit-identical buffers.  Not capturable: the step is enqueued eagerly, the all-reduce and the optimiser behind it (step.py)."""
    capturable = False

    def __init__(self, rank, shared):
        self.rank, self.world, self.sh = rank, shared.world, shared

    def allreduce_(self, buf):
        sh = self.sh
        sh.slots[self.rank] = buf
        sh.barrier.wait()
        total = sh.slots[0].clone()
        for r in range(1, self.world):
            total += sh.slots[r]
        sh.barrier.wait()                      # everybody has read every slot
        buf.copy_(total)
        sh.barrier.wait()
        return buf

    sum_counts_ = allreduce_

    def gather_labels(self, local, out=None):
        sh = self.sh
        sh.slots[self.rank] = local
        sh.barrier.wait()
        cat = torch.cat([sh.slots[r].reshape(-1) for r in range(self.world)])
        sh.barrier.wait()
        if out is None:
            return cat
        out.copy_(cat)
        return out

    def rows_of(self, flat_global, per_rank):
        return flat_global[self.rank * per_rank:(self.rank + 1) * per_rank]


def rank_rows(inject, r, W):
    """rank r's rows of injected noise that covers the global batch (per-rank masks: global_mask=False)"""
    out = {}
    for k, v in inject.items():
        if torch.is_tensor(v):
            n = v.numel() // W
            out[k] = v.reshape(-1)[r * n:(r + 1) * n]
        else:
            out[k] = v
    return out


def dp_one_step(args, W, B_local, epoch, *, sd_seed, inject, src_global, global_mask=True, rank_weights=None, env=None, deterministic=None,
                dev="cuda:0"):
    """one eager PretrainStep(dp=ThreadDP) per thread; rank r steps on rows [r * B_local, (r + 1) * B_local) of src_global.  The injected noise
    covers the GLOBAL cells: with global masks every rank gets all of it, with per-rank masks its rows of it.
    -> ([per rank: dict(g, stats, mask, w, kl, ...)], union of the launch names); mask is the global one under global masks, else the rank's."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.shard import ThreadNodeGroup
    from gptst_amd.step import PretrainStep
    assert src_global.shape[0] == W * B_local
    sd = O.init_state_dict(args, sd_seed)
    src_global = src_global.to(dev)
    shared = ThreadNodeGroup.Shared(W)

    def rank_main(r):
        m = GPTST_Model(args); m.load_state_dict(sd); m = m.to(dev)
        s = PretrainStep(m, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B_local, use_graph=False, dp=ThreadDP(r, shared),
                         global_mask=global_mask, deterministic=deterministic)
        assert s.gmask == (bool(global_mask) and W > 1)
        if rank_weights is not None:
            s.rank_weight = float(rank_weights[r])
        inj = inject if s.gmask else rank_rows(inject, r, W)
        inj = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inj.items()}
        mine = src_global[r * B_local:(r + 1) * B_local].contiguous()
        _two_steps(s, m, sd, lambda: s.step(mine, epoch, **inj), names)
        return _rank_result(s, m, s.last_mask_global if s.gmask else s.last_mask)

    with _Env(env), _Names() as names:
        out = _rank_threads(W, shared, rank_main)
    return out, sorted(names.names)


def _node_axis(key):
    return -1 if key.endswith(".adj") else 0


def assemble_sharded(per_rank, ranges, args_global, what="g"):
    """The ranks' tensors (what = "g": gradient views, "w": post-step weights) as ONE {key: tensor} in the global model's shapes: node-local keys
    concatenated from the ranks' [0, width) parts in rank order (last axis for cap*.adj, first otherwise), shared keys from rank 0.
    -> (tensors, report); report["pad_max"]: the largest absolute value in any rank's capacity padding (the part of a node-local key's slot behind
    its tensor), report["pad_worst"]: (rank, key) where, report["shared_identical"]: {shared key: all ranks hold it bit-identically}.
    Raises AssertionError naming the key if a rank's node-local tensor is not its slot's head, or has another width than its range."""
    from gptst_amd.model import GPTST_Model
    from gptst_amd.shard import is_node_local
    shapes = {k: tuple(v.shape) for k, v in GPTST_Model(args_global).state_dict().items()}
    out, rep = {}, dict(pad_max=0.0, pad_worst=None, shared_identical={})
    for k, v0 in per_rank[0][what].items():
        if not is_node_local(k):
            out[k] = v0
            rep["shared_identical"][k] = all(torch.equal(p[what][k], v0) for p in per_rank[1:])
            continue
        ax, parts = _node_axis(k), []
        for r, (p, (a, b)) in enumerate(zip(per_rank, ranges)):
            t, slot = p[what][k], p["slots_" + what][k]
            assert t.shape[ax] == b - a, (k, "rank %d holds %d nodes of its range [%d, %d)" % (r, t.shape[ax], a, b))
            assert torch.equal(slot[:t.numel()], t.reshape(-1)), (k, "rank %d: the tensor is not the head of its slot" % r)
            pad = float(slot[t.numel():].abs().max()) if slot.numel() > t.numel() else 0.0
            if pad > rep["pad_max"]:
                rep["pad_max"], rep["pad_worst"] = pad, (r, k)
            parts.append(t)
        out[k] = torch.cat(parts, dim=ax)
        assert tuple(out[k].shape) == shapes[k], (k, tuple(out[k].shape), shapes[k])
    return out, rep


def held_norm(got, stats, layout):
    """fp64 norm of the gradient views `got` as the optimiser sees them: path A divided by the kept count, path B as stored"""
    offs, nA, nB = layout
    cnt = max(float(stats[1]), 1.0)
    return float(torch.sqrt(sum((v.double() / (cnt if offs[k] < nA else 1.0)).pow(2).sum() for k, v in got.items() if offs[k] < nA + nB)))


def check_kept(per_rank, kept):
    """every rank's kept count (stats_out[1]) is `kept`, exactly"""
    for r, p in enumerate(per_rank):
        got = float(p["stats"][1])
        assert got == float(kept), ("kept count", "rank %d: %.1f, the global batch keeps %d cells" % (r, got, kept))


def check_norm(per_rank, gnorm64, held, record):
    """every rank's clip norm (stats_out[4] ** 0.5) is within NORM_TOL of the fp64 oracle's global norm and within NORM_SELF_TOL of `held`,
    the norm of the gradient the ranks hold"""
    for r, p in enumerate(per_rank):
        n = float(p["stats"][4]) ** 0.5
        e = abs(n - gnorm64) / gnorm64
        record("grad_norm", e)
        assert e < NORM_TOL, ("clip norm", "rank %d: %.6e against %.6e, off by %.3e" % (r, n, gnorm64, e))
        e = abs(n - held) / held
        record("grad_norm_vs_held_gradient", e)
        assert e < NORM_SELF_TOL, ("clip norm", "rank %d: %.6e, but the gradient held has %.6e, off by %.3e" % (r, n, held, e))


def check_sharded(per_rank, ranges, args_global, g64, ref32_fn, kept, record):
    """Assertions on what sharded_one_step returned, against the fp64 oracle of the GLOBAL problem: the assembled gradient per tensor (compare),
    shared gradients and post-step shared weights bit-identical on all ranks, capacity padding exactly zero in gradient and weights, kept count
    and clip norm on every rank -> compare's allowance dict."""
    got, rep = assemble_sharded(per_rank, ranges, args_global, "g")
    _, rep_w = assemble_sharded(per_rank, ranges, args_global, "w")
    record("pad_max_grad", rep["pad_max"])
    record("pad_max_weights", rep_w["pad_max"])
    assert rep["pad_max"] == 0.0, ("gradient padding", rep["pad_worst"], rep["pad_max"])
    assert rep_w["pad_max"] == 0.0, ("weight padding", rep_w["pad_worst"], rep_w["pad_max"])
    drift = [k for k, same in rep["shared_identical"].items() if not same]
    assert not drift, ("shared gradients differ between the ranks", drift)
    drift = [k for k, same in rep_w["shared_identical"].items() if not same]
    record("shared_weight_max_abs_diff_across_ranks",
           max([float((p["w"][k] - per_rank[0]["w"][k]).abs().max()) for k in drift for p in per_rank[1:]] or [0.0]))
    record("shared_weight_keys_that_differ", len(drift))
    assert not drift, ("shared weights differ between the ranks after the step", drift[:4], "%d keys in all" % len(drift))
    layout = layout_of(args_global)
    check_kept(per_rank, kept)
    allowed = compare(got, per_rank[0]["stats"], g64, ref32_fn, record, layout)
    check_norm(per_rank, grad_norm(g64), held_norm(got, per_rank[0]["stats"], layout), record)
    return allowed


def check_dp(per_rank, args, g64, ref32_fn, kept, record):
    """The same for dp_one_step: EVERY rank's gradient views against fp64 (the all-reduce left the global sum on each), gradients and post-step
    weights bit-identical on all ranks, kept count and clip norm on every rank -> the union of compare's allowance dicts."""
    for what in ("g", "w"):
        drift = [k for k, v in per_rank[0][what].items() if not all(torch.equal(p[what][k], v) for p in per_rank[1:])]
        assert not drift, ("%s differ between the ranks" % ("gradients" if what == "g" else "weights after the step"), drift)
    layout, allowed = layout_of(args), {}
    check_kept(per_rank, kept)
    for p in per_rank:
        allowed.update(compare(p["g"], p["stats"], g64, ref32_fn, record, layout))
    check_norm(per_rank, grad_norm(g64), held_norm(per_rank[0]["g"], per_rank[0]["stats"], layout), record)
    return allowed


def label_margin(args, sd, src):
    """the fp64 guide classifier's smallest top-2 probability margin over the cells of `src`"""
    with torch.no_grad():
        top2 = torch.topk(O.guide_probability({k: (v.double() if torch.is_tensor(v) and v.dtype.is_floating_point else v) for k, v in sd.items()},
                                              src.double(), args.input_base_dim), 2, dim=-1)[0]
    return float((top2[..., 0] - top2[..., 1]).min())


def losses_of(stats, kl):
    """(loss, loss_flow, loss_s) from a statistics snapshot, as PretrainStep.losses() reports them"""
    from gptst_amd.step import PretrainStep
    return PretrainStep._stats_row(stats, kl)
