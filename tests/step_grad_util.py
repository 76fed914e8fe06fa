"""Helpers of the fused step's gradient checks (tests/test_gpu_step_grads.py, tests/test_gpu_kl_carried.py, tests/test_step_grad_compare_cpu.py):
one fused PretrainStep with its gradient views kept, the same step through the oracle's autograd in a chosen precision, and the comparator.

What PretrainStep.g holds after a step: on path A (the reconstruction loss; flat offsets [0, nA)) the gradient of the SUM loss — the optimiser
divides it by the kept count in stats_out[1] (hyper[9]); on path B (the KL term; [nA, nA + nB)) the gradient as it is, 0.1 weight applied; behind
that the decoder's never-trained time features, which stay zero."""
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
