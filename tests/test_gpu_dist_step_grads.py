"""GPU: every parameter gradient of ONE step of the two scaled forms of the pretraining step — node shards (shard.py ShardedPretrainStep) and
data parallelism (PretrainStep(dp=...)) — against the fp64 oracle's autograd on the GLOBAL problem (all N nodes; the concatenated batch).
tests/test_gpu_shard*.py compare weights after three Adam steps, and Adam's m / (sqrt(v) + eps) does not move when a tensor's gradient is scaled
by a constant: a gradient W times too large, or the sum of W - 1 of W ranks, passes there.  Here the ranks (threads on this GPU,
step_grad_util.sharded_one_step / dp_one_step) leave their gradient views, and what the steppers add to PretrainStep's body is held per tensor:
the 1/W on the replicated-compute gradients, the save / restore of the node-local slots around the all-reduce, the zero capacity padding of
ragged shards, the clip-norm correction, the kept count in the buffer's tail, cap's cluster aggregations across ranks (C = 64 and 128), the
unfused sharded form, the KL backward as gptst_tail_kl, and under DP the statistics fold before the all-reduce, the label gather, rank_weight
and the three-slice all-reduce of GPTST_DP_OVERLAP inside one graph.  The assembling and checking code is proven on the CPU by
tests/test_dist_step_grad_compare_cpu.py.

Bound per tensor: max|a - b| / max|b| < 1e-4 against fp64 (step_grad_util.GRAD_TOL), path A divided by the global kept count.  ALLOWANCE may
hold only tensors whose fp32-ORACLE gradient alone reaches 1e-4 / 1.5 at that case; the fp32 oracle's worst tensor over this table is 4.4e-5
(time_feature1_.ln2.weight, N = 40 adaptive), 3.0e-5 at the C = 128 shape, so ALLOWANCE is empty and every tensor is held to 1e-4 outright.

Masks: the sharded step takes no forced mask, so every adaptive case must be compared on its free-running mask; the seeds of the table are
chosen on the CPU so that the fp64 classifier's smallest top-2 margin is far beyond MARGIN (asserted before anything runs on the GPU).

Measured on an MI355X (profiles/parity_dist_step_grads.json): worst tensor of the whole table 1.5e-5 (decoder time_feature1_.ln2.bias at
dp2_local_mask-ada), clip norm within 7.5e-8 of the oracle's and 7.1e-8 of the gradient held, kept counts and masks exact, padding zero.
What the file found: at the ragged three-rank shape (w3_n40, w3_n40_unfused) the shared weights after ONE step were one ulp apart on the
ranks (49 to 61 tensors, max |dw| 3.0e-8 .. 6.0e-8) although the shared gradients were bit-identical — every rank had rounded its clip norm
with its own node-local part mixed in.  shard.py::_after_backward now forms the total alike on every rank and hands it to the optimiser."""
import time

import pytest
import torch

import step_grad_util as U
from gptst_amd import synth
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu

ALLOWANCE = {}                                  # (module docstring) none
MARGIN = 1e-4

# NODE_SUM: the launch in front of engine.CTX.NODE_REDUCE.  Every shape of this table, C = 64 and C = 128, takes the streaming cap
# (ops.capflow_ok), whose gptst_capflow_post folds the node-chunk partials before the ranks' sum; gptst_capbig_type1, the first-generation
# kernel in front of NODE_REDUCE (ops.CAP_FLOW = False, or a shape capflow.hip does not support), is launched at none of them and stays
# unchecked per tensor.  The name alone proves little — the unsharded streaming cap launches it too: that the sum over the ranks
# is taken, forward and backward, is what the per-tensor comparison with the GLOBAL oracle shows.
TAIL_KL, GUEST, NODE_SUM = "gptst_tail_kl", "gptst_hypertem_chain_fwd_kl", "gptst_capflow_post"
# the unfused sharded form runs the loss kernels of their own: its KL head is gptst_kl, and neither fused tail is launched
UNFUSED = dict(present=("gptst_mae_fwd", "gptst_mae_bwd", "gptst_kl"), absent=("gptst_tail_mae", TAIL_KL))

_S = U.SMALL_DIST
# fp64 top-2 label margins (CPU, seeds (sd_seed, source seed)): with the default (3, 11) N = 40, B = 2 has 3.9e-5 — too close to an fp32 flip;
# of sd seeds 3..7 x source seeds 11..16 the pair (6, 11) is the widest there.  Every other shape keeps the defaults.
SHARD_CASES = {
    "w2_n40": dict(W=2, B=2, over=dict(num_nodes=40, **_S), seeds=(6, 11)),                        # margin 0.055; shards 20 / 20
    "w3_n40": dict(W=3, B=2, over=dict(num_nodes=40, **_S), seeds=(6, 11)),                        # 14 / 13 / 13: padding, label_pad
    "w3_n40_unfused": dict(W=3, B=2, over=dict(num_nodes=40, **_S), seeds=(6, 11), env=dict(GPTST_SHARD_FUSED="0"), paths=UNFUSED),
    "w8_n170": dict(W=8, B=2, over=dict(num_nodes=170, **_S), seeds=(3, 11)),                      # margin 0.66; 22, 22, 21, ...
    "w2_n256_c128": dict(W=2, B=1, over=dict(num_nodes=256, hidden_dim=128, embed_dim=8), seeds=(3, 11)),      # margin 0.048; C = 128 aggregation
    "w2_base2": dict(W=2, B=2, ds="NYC_TAXI", over=dict(num_nodes=30, **_S), seeds=(3, 11)),       # margin 0.27; two values per cell
    "w1_graph": dict(W=1, B=2, over=dict(num_nodes=40, **_S), seeds=(6, 11), group="world1_graph"),
}
_N20 = dict(num_nodes=20, **_S)                                                                     # margin 0.085 at B = 2, 3 and 4 with (3, 11)
DP_CASES = {
    "dp2": dict(W=2, Bl=2, over=_N20, epochs=(1, 20)),
    "dp3": dict(W=3, Bl=1, over=_N20, epochs=(1, 20)),
    "dp2_local_mask": dict(W=2, Bl=2, over=_N20, epochs=(1, 20), global_mask=False),
    "dp2_tail": dict(W=2, Bl=2, over=_N20, epochs=(1, 20), global_mask=False, rank_weights=(1.0, 0.0), deterministic=True),
    "dp2_bench": dict(W=2, Bl=2, over={}, epochs=(20,)),                                            # PEMS08's own dims (N = 170, C = 64): margin 0.24
}


def _oracles(args, sd, src, epoch, inj, parity):
    t0 = time.time()
    g64, l64, m64, kept64 = U.oracle_grads(args, sd, src, epoch, inj, torch.float64)
    parity("oracle64_seconds", time.time() - t0)
    g32, l32, m32, _ = U.oracle_grads(args, sd, src, epoch, inj, torch.float32)
    if "forced_mask" not in inj:
        assert torch.equal(m32, m64), "the fp32 oracle's mask differs from the fp64 one: choose other seeds"
    return g64, l64, m64, kept64, g32, l32


def _margin(name, args, sd, src, epoch, parity):
    """adaptive cases: a condition on the INPUTS, asserted before the GPU runs"""
    if epoch > args.change_epoch:
        m = U.label_margin(args, sd, src)
        parity("fp64_label_margin", m)
        assert m > MARGIN, (name, m)


def _finish(name, per_rank, allowed, worst, l64, l32, parity):
    top = sorted(((v, k) for k, v in worst.items() if k.startswith("grad:")), reverse=True)[:3]
    print(name, "worst gradients:", ", ".join("%s %.2e" % (k[5:], v) for v, k in top))
    parity("grad_worst", top[0][0])
    for k, (e, e_orc) in allowed.items():
        print(name, "allowance used:", k, "e_hip %.3e e_orc %.3e" % (e, e_orc))
    assert set(allowed) <= set(ALLOWANCE.get(name, ())), (name, allowed)
    # the losses: within 3x the fp32 oracle's own deviation from fp64 (+ 2e-6), on every rank
    for r, p in enumerate(per_rank):
        assert float(p["stats"][5]) == 0.0, (name, r, "an in-launch hand-off expired")
        lh = U.losses_of(p["stats"], p["kl"])
        for i, what in ((1, "mae"), (2, "kl")):
            if l64[i] == 0.0:
                assert lh[i] == 0.0, (name, r, what, lh[i])
                continue
            e32, eh = abs(l32[i] - l64[i]) / abs(l64[i]), abs(lh[i] - l64[i]) / abs(l64[i])
            parity("loss_" + what, eh)
            parity("loss_" + what + "_oracle32", e32)
            assert eh <= 3.0 * e32 + 2e-6, (name, r, what, eh, e32)


def _recorder(parity):
    worst = {}

    def rec(k, v):
        parity(k, v)
        worst[k] = max(v, worst.get(k, 0.0))
    return rec, worst


@pytest.mark.parametrize("epoch", [1, 20], ids=["rand", "ada"])
@pytest.mark.parametrize("name", list(SHARD_CASES))
def test_sharded_step_gradients_vs_fp64_oracle(name, epoch, parity):
    c = SHARD_CASES[name]
    W, B = c["W"], c["B"]
    args = U.dist_args(c.get("ds", "PEMS08"), **c["over"])
    sd_seed, src_seed = c["seeds"]
    adaptive = epoch > args.change_epoch
    sd = O.init_state_dict(args, sd_seed)
    src = U.make_src(args, B, seed=src_seed)
    inj = U.noise_inject(args, B, epoch)
    _margin(name, args, sd, src, epoch, parity)
    g64, l64, m64, kept64, g32, l32 = _oracles(args, sd, src, epoch, inj, parity)
    assert U.grad_norm(g64) > args.max_grad_norm              # the clip acts

    t0 = time.time()
    per_rank, ranges, names = U.sharded_one_step(args, W, B, epoch, sd_seed=sd_seed, inject=inj, src=src, env=c.get("env"),
                                                 group=c.get("group", "thread"))
    parity("step_seconds", time.time() - t0)
    for r, p in enumerate(per_rank):                          # every rank's global mask: the fp64 oracle's, bit for bit
        assert torch.equal(p["mask"].reshape(-1), m64.reshape(-1)), (name, "global mask differs from the fp64 oracle's on rank %d" % r)
    kept = U.kept_count(args, src, m64)
    assert kept == kept64, (name, kept, kept64)
    rec, worst = _recorder(parity)
    allowed = U.check_sharded(per_rank, ranges, args, g64, lambda: g32, kept, rec)
    _finish(name, per_rank, allowed, worst, l64, l32, parity)

    # the routes
    if c.get("group") == "world1_graph":
        assert names == [], names                             # a graph replay enqueues nothing through ops
        return
    print(name, "launches:", names)
    if adaptive:
        if "paths" not in c:
            assert TAIL_KL in names, (name, "missing", TAIL_KL)
        assert GUEST not in names, (name, "unexpected", GUEST)
    if W > 1:
        assert NODE_SUM in names, (name, "missing", NODE_SUM)
    want = c.get("paths", {})
    for w in want.get("present", ()):
        if w == "gptst_kl" and not adaptive:
            continue
        assert w in names, (name, "missing", w)
    for w in want.get("absent", ()):
        assert w not in names, (name, "unexpected", w)


@pytest.mark.parametrize("name,epoch", [(n, e) for n, c in DP_CASES.items() for e in c["epochs"]],
                         ids=["%s-%s" % (n, "rand" if e == 1 else "ada") for n, c in DP_CASES.items() for e in c["epochs"]])
def test_data_parallel_step_gradients_vs_fp64_oracle(name, epoch, parity):
    c = DP_CASES[name]
    W, Bl = c["W"], c["Bl"]
    args = U.dist_args("PEMS08", **c["over"])
    adaptive = epoch > args.change_epoch
    gmask, weights = c.get("global_mask", True), c.get("rank_weights")
    sd = O.init_state_dict(args, U.SD_SEED)
    src_g = U.make_src(args, W * Bl)                           # rank r: rows [r * Bl, (r + 1) * Bl)
    inj_g = U.noise_inject(args, W * Bl, epoch)
    base, M = args.input_base_dim, Bl * args.lag * args.num_nodes
    _margin(name, args, sd, src_g, epoch, parity)
    if weights is not None:                                    # the tail round: the job's batch is rank 0's; rank 1 steps on padding (other rows)
        src_o, inj_o = src_g[:Bl].contiguous(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in U.rank_rows(inj_g, 0, W).items()}
    else:
        src_o, inj_o = src_g, inj_g
    if gmask or weights is not None:
        g64, l64, m64, kept64, g32, l32 = _oracles(args, sd, src_o, epoch, inj_o, parity)

    t0 = time.time()
    per_rank, names = U.dp_one_step(args, W, Bl, epoch, sd_seed=U.SD_SEED, inject=inj_g, src_global=src_g, global_mask=gmask,
                                    rank_weights=weights, deterministic=c.get("deterministic"))
    parity("step_seconds", time.time() - t0)
    if gmask:
        for r, p in enumerate(per_rank):
            assert torch.equal(p["mask"].reshape(-1), m64.reshape(-1)), (name, "global mask differs from the fp64 oracle's on rank %d" % r)
    else:
        for r, p in enumerate(per_rank):                       # per-rank masks: each the budget of its own cells
            assert int((p["mask"] == 0).sum()) == int(M * base * args.mask_ratio), (name, r, int((p["mask"] == 0).sum()))
        if weights is not None:
            assert torch.equal(per_rank[0]["mask"].reshape(-1), m64.reshape(-1)), (name, "rank 0's mask differs from the fp64 oracle's")
        else:                                                  # the oracle is teacher-forced with the concatenation of the ranks' masks
            forced = torch.cat([p["mask"].reshape(-1) for p in per_rank]).reshape(src_g.shape[:3] + (base,))
            g64, l64, m64, kept64, g32, l32 = _oracles(args, sd, src_g, epoch, dict(forced_mask=forced), parity)
            assert torch.equal(m64.reshape(-1), forced.reshape(-1))
    assert U.grad_norm(g64) > args.max_grad_norm               # the clip acts
    kept = U.kept_count(args, src_o, m64)
    assert kept == kept64, (name, kept, kept64)
    rec, worst = _recorder(parity)
    allowed = U.check_dp(per_rank, args, g64, lambda: g32, kept, rec)
    _finish(name, per_rank, allowed, worst, l64, l32, parity)
    print(name, "launches:", names)
    if adaptive:
        assert TAIL_KL in names, (name, "missing", TAIL_KL)
        assert GUEST not in names, (name, "unexpected", GUEST)


@pytest.mark.parametrize("epoch", [1, 20], ids=["rand", "ada"])
def test_dp1_overlap_graph_gradients_vs_fp64_oracle(epoch, parity):
    """W = 1 forced data parallelism on the native communicator with GPTST_DP_OVERLAP=1 and use_graph=True: the gradient leaves in three slices
    around dec_lo / dec_hi inside ONE hipGraph.  The communicator is set up as tests/test_gpu_multiproc.py::
    test_dp_step_in_one_graph_equals_the_plain_step sets it up (and required as there: no skip)."""
    import torch.distributed as dist
    from conftest import free_port
    from gptst_amd.dist import DataParallel
    from gptst_amd.model import GPTST_Model
    from gptst_amd.step import PretrainStep
    name, B, dev = "dp1_overlap_graph", 2, "cuda:0"
    args = U.dist_args("PEMS08", **_N20)
    sd = O.init_state_dict(args, U.SD_SEED)
    src = U.make_src(args, B)
    inj = U.noise_inject(args, B, epoch)
    _margin(name, args, sd, src, epoch, parity)
    g64, l64, m64, kept64, g32, l32 = _oracles(args, sd, src, epoch, inj, parity)
    env = dict(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), GPTST_FORCE_DP="1",
               GPTST_DP_OVERLAP="1")
    with U._Env(env), U._Names() as names:
        dp = DataParallel("nccl", native=True)
        try:
            assert dp.capturable and dp.rccl_ranks() == 1
            model = GPTST_Model(args); model.load_state_dict(sd); model = model.to(dev)
            st = PretrainStep(model, args, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B, use_graph=True, dp=dp)
            assert st.dp_overlap and 0 < st.dec_lo < st.dec_hi == model.nA
            injd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inj.items()}
            srcd = src.to(dev)
            U._two_steps(st, model, sd, lambda: st.step(srcd, epoch, **injd), names)
            assert all(g2 is None for _, g2 in st.graphs.values()) and not st._graph_comm_failed, "one graph per phase, collectives inside"
            per_rank = [U._rank_result(st, model, st.last_mask)]
        finally:
            dp.native.close()
            dist.destroy_process_group()
    assert torch.equal(per_rank[0]["mask"].reshape(-1), m64.reshape(-1)), (name, "mask differs from the fp64 oracle's")
    kept = U.kept_count(args, src, m64)
    assert kept == kept64, (name, kept, kept64)
    rec, worst = _recorder(parity)
    allowed = U.check_dp(per_rank, args, g64, lambda: g32, kept, rec)
    _finish(name, per_rank, allowed, worst, l64, l32, parity)
    assert names.names == set(), names.names                   # a graph replay enqueues nothing through ops
