"""Which C-ABI calls does a pretraining step make, in which order — and what do three steps compute, bit for bit?

    python tools/launch_trace.py [config ...] > trace.txt

For every configuration below (the no_* ones switch one of the engine's module attributes off after import): the ordered (name, tag) of every call through ops._call (ops.TIMER) in one eager random-mask step and one eager
adaptive-mask + KL step, then a SHA-256 of the weights after three steps (epochs 1, 20, 25) from a fixed seed with injected mask noise and the
library's fixed-order reductions (deterministic=True; the paths that have no such switch run under ops.set_deterministic(True)).  The graphed module
path has no optimiser: its hash is the flat gradient of one forward / backward; the eager autograd node is traced only (see autograd_node).  Two builds of the Python side agree on what a step does exactly when
their outputs are identical line for line (the library is chosen with GPTST_LIB).  One process, a few seconds of GPU time per configuration.
"""
import hashlib
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gptst_amd import engine, module_graph, ops, synth  # noqa: E402
from gptst_amd.config import make_args  # noqa: E402
from gptst_amd.model import GPTST_Model, init_seed, xavier_init_  # noqa: E402
from gptst_amd.shard import DistNodeGroup, ShardedPretrainStep  # noqa: E402
from gptst_amd.step import PretrainStep  # noqa: E402

DEV = "cuda:0"
EPOCHS = (1, 20, 25)                          # random-mask phase, then adaptive + KL twice (change_epoch = 3)
BENCH = dict(ds="PEMS08", over={}, B=32)
C128 = dict(ds="PEMS08", over=dict(hidden_dim=128, num_nodes=40, embed_dim=8), B=2)      # tests/test_gpu_shapes.py "c128"


def traced(fn):
    """-> [(name, tag)] of the calls fn makes"""
    ops.TIMER = []
    try:
        fn()
        torch.cuda.synchronize()
        return [rec[:2] for rec in ops.TIMER]
    finally:
        ops.TIMER = None


def traced_threads(fn):
    """-> {thread name: [(name, tag)]}.  Emulated ranks enqueue side by side under ops.CALL_LOCK, which bypasses ops.TIMER: the calls are
    recorded one level up, around ops._call, per thread."""
    calls, inner = {}, ops._call

    def call(name, *args, tag="", nbytes=0):
        calls.setdefault(threading.current_thread().name, []).append((name, tag))
        return inner(name, *args, tag=tag, nbytes=nbytes)
    ops._call = call
    try:
        fn()
        torch.cuda.synchronize()
        return calls
    finally:
        ops._call = inner


def show(title, calls):
    print("-- %s: %d calls" % (title, len(calls)))
    for name, tag in calls:
        print("   %s %s" % (name, tag))


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def build(shape):
    args = make_args(shape["ds"], scaler_zeros=synth.scaler_zeros(), epochs=30, change_epoch=3, **shape["over"])
    init_seed(args.seed)
    return args, xavier_init_(GPTST_Model(args)).to(DEV)


def inputs(args, B, N=None):
    N, base = N or args.num_nodes, args.input_base_dim
    M = B * 12 * N
    srcs = [synth.make_batch(B, 12, N, base, seed=40 + i).to(DEV) for i in range(3)]
    noise = [tuple(synth.make_noise(M * (base if i == 0 else 1), 10 * s + i).to(DEV) for i in range(3)) for s in range(3)]
    return srcs, noise, synth.class_order(args.HS, 9)


def run_steps(make, args, B, N=None):
    """trace of epochs 1 and 20 on the configured stepper; hash after EPOCHS on a fresh deterministic one"""
    srcs, noise, list_c = inputs(args, B, N)
    st, _ = make(None)
    for epoch, src, (n0, na, nr) in list(zip(EPOCHS, srcs, noise))[:2]:
        calls = traced(lambda: st.step(src, epoch, noise=n0, noise_a=na, noise_r=nr, list_c=list_c))
        show("phase %d step" % (0 if epoch == 1 else 1), calls)
    st, model = make(True)
    for epoch, src, (n0, na, nr) in zip(EPOCHS, srcs, noise):
        st.step(src, epoch, noise=n0, noise_a=na, noise_r=nr, list_c=list_c)
    print("-- sha256 of the weights after 3 steps: %s" % sha(model.flat))


def plain(shape, env=None, deterministic=False, safe=False, attrs=None):
    """attrs: engine module attributes switched after import, for this configuration only"""
    def make(det):
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:
            args, model = build(shape)
            st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=shape["B"], use_graph=False,
                              deterministic=deterministic if det is None else det)
        finally:
            for k in (env or {}):
                del os.environ[k]
        st.safe_mode = safe
        return st, model
    keep = {k: getattr(engine, k) for k in attrs or {}}
    for k, v in (attrs or {}).items():
        setattr(engine, k, v)
    try:
        run_steps(make, build(shape)[0], shape["B"])
    finally:
        for k, v in keep.items():
            setattr(engine, k, v)


def shard_one_rank():
    def make(det):
        args, model = build(BENCH)
        st = ShardedPretrainStep(model, args, args.num_nodes, DistNodeGroup(0, 1), synth.SCALER_MEAN, synth.SCALER_STD, batch_size=32, use_graph=False)
        return st, model
    ops.set_deterministic(True)        # (the sharded step has no deterministic switch of its own: the library's mode, set from outside)
    try:
        run_steps(make, build(BENCH)[0], 32)
    finally:
        ops.set_deterministic(False)


def shard_threads(W=2, N=40, B=2):
    """the thread-emulated ranks of tests/test_gpu_shard.py, through its helper"""
    from oracle import gptst_oracle as O
    from tests import test_gpu_shard as T
    args = T._args(N)
    sd = O.init_state_dict(args, 5)
    srcs, noise, list_c = inputs(args, B)
    step = ShardedPretrainStep.step

    def det_step(self, *a, **k):       # the library's launch mode is per thread: every emulated rank sets it for itself
        ops.set_deterministic(True)
        return step(self, *a, **k)
    ShardedPretrainStep.step = det_step
    try:
        out = []
        per_rank = traced_threads(lambda: out.extend(T._run_sharded(W, N, B, T.SMALL, [(e, i) for i, e in enumerate(EPOCHS)], srcs, noise, list_c, sd)))
    finally:
        ShardedPretrainStep.step = step
    ranks = sorted(k for k in per_rank if k != "MainThread")        # "Thread-<n> (rank_main)": numbered in start order = rank order
    for r, k in enumerate(ranks):
        show("rank %d, 3 steps" % r, per_rank[k])
    for r in range(W):
        print("-- sha256 of rank %d's weights after 3 steps: %s" % (r, sha(*out[r][2].values())))


def graphed(has_kl):
    args, model = build(BENCH)
    torch.manual_seed(11)
    gp = module_graph.GraphedPretrain(model, (32, 12, args.num_nodes, args.input_base_dim + 2), 1 if has_kl else 0)
    g = torch.Generator().manual_seed(3)
    gp.src.copy_(synth.make_batch(32, 12, args.num_nodes, args.input_base_dim, seed=40))
    gp.d_out.copy_(torch.randn(gp.d_out.shape, generator=g))
    gp.d_prob.copy_(torch.randn(gp.d_prob.shape, generator=g))

    def body():
        torch.manual_seed(12)
        with torch.no_grad():
            gp._fwd_body()
            gp._bwd_body(has_kl)
    show("_fwd_body + _bwd_body(has_kl=%s)" % has_kl, traced(body))
    ops.set_deterministic(True)
    try:
        body()
    finally:
        ops.set_deterministic(False)
    print("-- sha256 of the flat gradient: %s" % sha(gp.gflat))


def autograd_node():
    args, model = build(BENCH)
    module_graph.ENABLED = False
    srcs, noise, list_c = inputs(args, 32)

    def body():
        model.set_mask_inputs(noise_a=noise[1][1], noise_r=noise[1][2], list_c=list_c)
        out, dec, _, prob, _ = model(srcs[0], None, epoch=20)
        (out.abs().sum() + 0.5 * dec.sum() + (prob * prob).sum()).backward()
    show("_PretrainFn forward + backward", traced(body))
    # (no hash: the eager node's gradient is not reproducible from run to run even under ops.set_deterministic(True) — four runs of one build
    #  gave four hashes — so a hash would say nothing about two builds)


CONFIGS = {
    "plain": lambda: plain(BENCH),
    "unfused_tails": lambda: plain(BENCH, env={"GPTST_FUSED_TAILS": "0"}),
    "deterministic": lambda: plain(BENCH, deterministic=True),
    "safe_mode": lambda: plain(BENCH, safe=True),
    "c128": lambda: plain(C128),
    "shard_one_rank": shard_one_rank,
    "shard_two_thread_ranks": shard_threads,
    "graphed_module_no_kl": lambda: graphed(False),
    "graphed_module_kl": lambda: graphed(True),
    "autograd_node": autograd_node,
}
for _k in ("FUSE_HT_BWD", "FUSE_CROSS", "CAP_LIN", "CHAIN_FWD", "PAIR_BWD", "GUIDEIN", "CARRY_RED", "CARRY_KL"):      # branches behind the engine's switches
    CONFIGS["no_" + _k.lower()] = lambda k=_k: plain(BENCH, attrs={k: False})
CONFIGS["c128_no_chain128"] = lambda: plain(C128, attrs={"CHAIN128": False})

if __name__ == "__main__":
    for name in sys.argv[1:] or list(CONFIGS):
        print("==== %s" % name, flush=True)
        CONFIGS[name]()
        sys.stdout.flush()
