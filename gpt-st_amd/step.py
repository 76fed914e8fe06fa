"""One fused pretraining step = the body of reference BasicTrainer.train_epoch (model/BasicTrainer.py:72-103):
zero_grad -> forward (mask generation included) -> masked-MAE (+0.1 KL) -> backward -> clip_grad_norm_(5) -> Adam,
entirely as HIP kernels enqueued on one stream and captured in a hipGraph (two graphs: random-mask phase and
adaptive-mask + KL phase).  Nothing in the step synchronises with the host: loss scalars are read from a device
statistics block whenever the caller asks.  Data-parallel: one process per GPU, one RCCL all-reduce (sum) of
[flat gradient | loss statistics] between backward and the optimiser (dist.py).
"""
import contextlib
import dataclasses
import itertools
import os
import random
from typing import Any, NamedTuple

import torch

from . import engine, ops

# mask generation on the 24-bit noise lattice (gptst_mask_*_u24, r04): the step's Philox noise and torch.rand fixtures are k * 2^-24, so the radix
# select takes two 12-bit digits on the integers instead of three float-bit digits: 6 launches instead of 8 in the adaptive phase.  (The whole
# generation as ONE single-workgroup launch was measured too: ~120 us against ~45 us at 65 280 cells — one CU's bandwidth; it serves <= 8192 cells.)
DEFER_GEN = os.environ.get("GPTST_DEFER_GEN", "1") == "1"      # the STHCNs' parameter generation inside the cooperative mask launch (r05)
U24 = os.environ.get("GPTST_MASK_U24", "1") == "1"


class Part1(NamedTuple):
    """what part 1 of a step hands to part 2"""
    tidx: Any
    gen: Any        # engine.GenAll
    red: Any        # engine.Reductions
    prob: Any       # the guide's probabilities and engine.GuideSaved (None: no guide in this phase)
    sv_g: Any


@dataclasses.dataclass(eq=False)
class Enqueued:
    """One enqueued optimisation step, as the stepper's ledger keeps it until the host has read its statistics"""
    phase: int
    epoch: int
    list_c: Any     # the class order the step ran with (None in the random-mask phase)
    weight: float   # rank_weight of the step
    src: Any        # device tensor that still holds the step's batch; None: the step cannot be repeated (injected noise, forced mask, buffer reused)
    stats: Any      # device snapshot of the step's statistics; None: written over by a later step
    replay: int     # shared by the steps of one graph replay
    group: int      # shared by the steps of one step() / step_group() call
    slot: Any       # j: sub-step j of a group (src, stats are the group's j-th buffers); None: a plain step (self.src, self.stats_out)
    row: Any = None  # the statistics on the host, once read


class PretrainStep:
    RING = 8                                  # pinned host slots in flight (ops.PinnedRing)
    DETERMINISTIC_MODE = True                 # the stepper sets the library's launch mode from self.deterministic (False: never touches it)
    FORCED_MASK = True                        # step(forced_mask=) is served

    def __init__(self, model, args, scaler_mean, scaler_std, batch_size, use_graph=True, dp=None, seed=0, global_mask=True,
                 deterministic=None):
        """``seed`` drives the class-order shuffle and (data parallel, global masks) the mask noise: it must be the SAME on every
        rank, because every rank regenerates the selection over the global batch and keeps its rows (dist.py)."""
        self.model, self.args = model, args
        self.mean, self.std = float(scaler_mean), float(scaler_std)
        self.B, self.T, self.N = batch_size, args.lag, args.num_nodes
        self.C, self.base, self.HS = args.hidden_dim, args.input_base_dim, args.HS
        self.dims = (self.B, self.T, self.N, self.C)
        self.dev = model.flat.device
        assert self.dev.type == "cuda", "PretrainStep needs the model on an MI355X (no CPU fallback)"
        self.use_graph, self.dp = use_graph, dp
        # bit-reproducible steps (GPTST_DETERMINISTIC=1): single-owner, fixed-order variants of the two reductions that end in float
        # atomics by default (ops.set_deterministic); with injected mask noise two runs of a step sequence are then bit-identical
        self.deterministic = self.DETERMINISTIC_MODE and ((os.environ.get("GPTST_DETERMINISTIC", "0") == "1") if deterministic is None else bool(deterministic))
        n = model.flat.numel()
        self.gbuf = torch.zeros(n + 8, device=self.dev)             # [flat gradient | stats] -> one collective
        self.gflat, self.stats = self.gbuf[:n], self.gbuf[n:]
        self.g = model.views_of(self.gflat)
        self.m, self.v = torch.zeros(n, device=self.dev), torch.zeros(n, device=self.dev)
        M = self.B * self.T * self.N
        self.src = torch.zeros(self.B, self.T, self.N, self.base + 2, device=self.dev)
        self.noise = torch.zeros(M * self.base, device=self.dev)
        self.noise_ar = torch.zeros(2 * M, device=self.dev)          # adaptive phase: [noise_a | noise_r], drawn by ONE launch
        self.noise_a, self.noise_r = self.noise_ar[:M], self.noise_ar[M:]
        # per-step host scalars in ONE device buffer / ONE H2D copy: [hyper (16 fp32) | list_c (HS int32) | adaptive_num, random_num | rng seed, step]
        self.hc = torch.zeros(16 + self.HS + 4, dtype=torch.int32, device=self.dev)
        self.hyper = self.hc[:16].view(torch.float32)
        self.ctrl = self.hc[16:16 + self.HS + 2]
        self.rng_words = self.hc[16 + self.HS + 2:]                  # Philox key of the step's mask noise (step_begin)
        self.noise_seed = 1234567 + seed
        self._ring = ops.PinnedRing(self.hc.numel(), slots=self.RING)        # (hundreds of steps are queued back to back by bench.py)
        self.phase_kl = False                                        # phase of the last enqueued step (losses())
        self._gK, self._group_failed = 0, False                      # step_group(): group size set up, capture refused
        self.stats_out = torch.zeros(8, device=self.dev)            # snapshot of stats after the step (graph output)
        self.mask_buf = torch.ones(M * self.base, device=self.dev)   # teacher-forced mask (parity runs)
        self.last_mask = None
        self.force_mask = False
        self.tA = self.tB = 0
        self.lr = args.lr_init
        self.rng = random.Random(seed)
        self.graphs = {}
        self._g_graphs = {}                  # step_group(): phase -> graph of K steps
        self._graph_comm_failed = False      # capturing the collectives failed once: they run between graph replays
        self._ctx_keep = []                  # part 1's tensors of every two-graph capture (inputs of its second graph)
        self._sws = None                     # fused loss statistics awaiting the optimiser's launch (_fold_stats)
        self.inject_noise = False
        self.global_count_scale = False      # set by subclasses that all-reduce [gradient | statistics] themselves (shard.py)
        self.node_reduce = None              # node shards: completes a sum over nodes across the ranks (engine.CTX.NODE_REDUCE while a step is enqueued)
        self.join_enc_dec = True             # the decoder's first hyperTem layer rides on the encoder's last chain launch (engine.autoencoder_fwd(join=))
        # r05, lost in-launch hand-offs (a bounded wait of the pair / role launches expired: the GPU was time-sliced away from the producer for
        # seconds): the optimiser skips the update of such a step (gptst_clip_adam's guard; stats_out[5] > 0), losses() / losses_group() notice,
        # switch this stepper to the launches WITHOUT hand-offs (safe_mode: graphs re-captured) and re-run the skipped steps from the untouched weights
        self.safe_mode = False
        self.lost_steps = 0                  # steps re-run so far
        self.lost_batches = 0                # ... and steps that were skipped with a later one and could not be repeated (their batches were gone)
        self._ledger = []                    # Enqueued records: the last call's steps, then every step enqueued since the host last read the statistics
        self._holder = {}                    # slot -> the record that last wrote that slot's buffers (_note)
        self._ids = itertools.count()
        self.arena = engine.ZeroArena(self.dev)
        self.fused_tails = os.environ.get("GPTST_FUSED_TAILS", "1") == "1" and engine.fused_tails_ok(model.param_views(), self.C, self.base, self.HS)
        # ---- data parallel: masks over the GLOBAL batch (dist.py) ----
        self.W = dp.world if dp is not None else 1
        self.gmask = bool(global_mask) and dp is not None and self.W > 1
        if self.gmask:
            Mg = M * self.W
            self.noise_g = torch.zeros(Mg * self.base, device=self.dev)
            self.noise_ar_g = torch.zeros(2 * Mg, device=self.dev)
            self.noise_a_g, self.noise_r_g = self.noise_ar_g[:Mg], self.noise_ar_g[Mg:]
            self.label_l = torch.zeros(M, dtype=torch.int32, device=self.dev)
            self.label_g = torch.zeros(Mg, dtype=torch.int32, device=self.dev)
        # r04, data parallel on the capturable communicator: the gradient leaves in BUCKETS — the decoder's parameters are complete when the decoder's
        # backward ends, so their reductions + all-reduce run on a forked branch UNDER the encoder's backward; only the encoder / KL bucket
        # is exchanged behind the chain (one 4.15 MB all-reduce behind everything before).  GPTST_DP_OVERLAP=0: the single all-reduce.
        # (the bucket's reductions stay on the chain's stream, only its all-reduce is forked: forking the reductions too cost 5 % at one rank)
        self.always_guide = os.environ.get("GPTST_ALWAYS_GUIDE", "0") == "1"      # run the guide classifier in the random-mask phase too (as the reference does)
        # r06: OFF by default.  Measured with one forced-DP rank (profiles/r06_dp_world1.txt): 854.9 steps/s with the overlap, 885.6 without, 891.1 without
        # data parallelism — the early bucket needs its own reduction flush in the middle of the backward (gram_bwd + job table + time-feature launch:
        # ~50 us) and keeps the reductions out of the routing backward's idle slots, i.e. it costs ~41 us per step on EVERY rank to hide part of a
        # 4.15 MB all-reduce that takes about that long un-hidden on eight xGMI-connected GPUs.  GPTST_DP_OVERLAP=1 turns it on.
        self.dp_overlap = (os.environ.get("GPTST_DP_OVERLAP", "0") != "0" and dp is not None and getattr(dp, "capturable", False)
                           and (self.W > 1 or os.environ.get("GPTST_FORCE_DP", "0") == "1"))
        self.dec_lo, self.dec_hi = self._decoder_bucket(model)
        self.rank_weight = 1.0                          # 0.0: this rank steps on padding (eager tail round of a data-parallel epoch, see _allreduce)
        self.fork_side = torch.cuda.Stream() if self.dp_overlap else None

    # ---- the enqueued work ---------------------------------------------------------------------------------------
    # A step is enqueued in two parts: part 1 ends with the guide classifier (the cluster labels of the local rows), part 2 starts
    # with the mask.  Under data parallelism with global masks the adaptive phase exchanges the labels BETWEEN the two parts (one
    # all-gather; the class histogram is taken from the gathered labels) — as two hipGraphs sharing one memory pool, so that the
    # guide forward is computed once and no collective sits inside a graph.  Everything else runs the two parts back to back.
    def _needs_exchange(self, phase):
        return self.gmask and phase == 1 and not self.force_mask

    @staticmethod
    def _decoder_bucket(model):
        """[lo, hi) of the decoder's trained parameters in the flat buffer (they are contiguous: segment A is in registration order,
        encoder first; the decoder's never-trained time features live in the last segment)."""
        offs = [(o, model.state_dict()[k].numel()) for k, o in model._offs.items() if k.startswith("decoder.") and o < model.nA]
        lo = min(o for o, _ in offs)
        hi = max(o + (n + 3) // 4 * 4 for o, n in offs)
        assert hi == model.nA and all(o >= lo for o, _ in offs), (lo, hi, model.nA)
        assert not any(lo <= o < hi for k, o in model._offs.items() if not k.startswith("decoder.")), "decoder bucket is not contiguous"
        return lo, hi

    def _allreduce(self, sl):
        """All-reduce of a slice of the packed [gradient | statistics] buffer.  rank_weight = 0 (an eager tail step of a data-parallel epoch:
        this rank has no batch of its own in the last, incomplete round and steps on padding) zeroes the rank's contribution first — gradient
        AND statistics, so the global kept-cell count the optimiser divides by does not see the padding either."""
        if self.rank_weight != 1.0:
            assert not self.use_graph, "a rank weight is baked into a captured graph: tail rounds use eager steppers"
            lost = self.stats[5:6].clone()              # the hand-off expiry count rides in the statistics block: a padding rank's expiry must reach its
            sl.mul_(self.rank_weight)                   # peers unscaled, or it alone skips the update and re-runs a step of collectives nobody joins
            self.stats[5:6].copy_(lost)
        self.dp.allreduce_(sl)

    def _bucket_ready(self, k):
        """engine.Reductions callback (inside the side-stream fork): bucket 0 = the decoder's gradient is final -> its all-reduce starts now"""
        if k == 0:
            self._allreduce(self.gbuf[self.dec_lo:self.dec_hi])
            self._dec_reduced = True

    def _dp_in_graph(self):
        """Data parallel on a capturable communicator (dist.DataParallel(native=True)): label gather, gradient all-reduce and optimiser are
        enqueued as part of the step body — one hipGraph per phase holds everything, as in the single-GPU case."""
        return self.dp is not None and getattr(self.dp, "capturable", False) and not self._graph_comm_failed

    def _part1(self, phase):
        p, dims, base = self.model.param_views(), self.dims, self.base
        engine.CTX.ARENA, engine.CTX.NODE_REDUCE = self.arena, self.node_reduce
        src = self.src
        # zero_grad + the step's zero scratch + the time index of node 0: one launch
        # (the step's mask noise is drawn by the same launch, unless injected / forced)
        noise = None if self.inject_noise or self.force_mask else self._noise_buffer(phase)
        tidx = ops.step_begin(self.gbuf, self.arena.begin(zero=False), src, base, noise=noise, rng=self.rng_words)
        need_guide = self._need_guide(phase)
        # time embeddings + every generated parameter: 3 launches; r05: the STHCNs' forward jobs wait for the mask's launch (_part2_impl)
        gen = engine.gen_all(p, tidx, dims, guide=need_guide, defer=DEFER_GEN)
        red = engine.Reductions()
        red.no_carry = self.deterministic
        red.want_tail = True                                         # (engine.tail_roles_ok decides per step)
        self._dec_reduced = False
        if self.dp_overlap and self._dp_in_graph():
            red.on_bucket = self._bucket_ready
            red.bucket_inline, red.fork_side = True, self.fork_side
        lowrank = self.fused_tails and engine.chain_ok(dims)      # the guide's backward (KL path) is the dPre chain: its first layers may run low-rank
        prob, sv_g = engine.guide_fwd(p, src, tidx, dims, base, gen=gen.guide, lowrank_in=lowrank) if need_guide else (None, None)
        if self._needs_exchange(phase):
            self.label_l.copy_(sv_g.label)                           # this rank's cluster labels -> all-gather (_exchange_labels)
        return Part1(tidx, gen, red, prob, sv_g)

    def _part2(self, phase, ctx):
        if not self.safe_mode:
            return self._part2_impl(phase, ctx)
        with engine.no_handoffs():              # hyperTem backward per layer, cross-time backward as a prologue: no in-launch waits
            return self._part2_impl(phase, ctx)

    def _part2_impl(self, phase, ctx):
        mdl, p, g, dims, base = self.model, self.model.param_views(), self.g, self.dims, self.base
        a = self.args
        src, tidx, gen, red, prob, sv_g = self.src, ctx.tidx, ctx.gen, ctx.red, ctx.prob, ctx.sv_g
        engine.CTX.ARENA, engine.CTX.NODE_REDUCE = self.arena, self.node_reduce
        pend = gen.pending       # the STHCNs' generated-parameter jobs: inside the mask's launch where that is the cooperative one
        mask = self._make_mask(phase, prob, sv_g.label if sv_g is not None else None, pend)
        if pend is not None:
            pend.launch()                      # (forced mask: nothing carried them; a no-op after a mask call)
        self.last_mask = mask
        fused = self.fused_tails
        kl, sws = None, None
        if phase == 1 and self._carry_kl(sv_g):   # the KL path's backward rides on the forward's chain launches (engine.KlCarry)
            sws = self._tail_sws()
            kl = engine.KlCarry(p, sv_g, prob, src, dims, 0.1, sws)
        # lowrank_in: the fused backward is the dPre chain, so the low-rank first layer may run; head: the fused loss tail goes through it itself
        fw = engine.autoencoder_fwd(p, src, mask, dims, base, mdl.num_route, mdl.scaler_zeros, gen=gen, tidx=tidx,
                                    lowrank_in=fused and engine.chain_ok(dims), kl=kl, head=not fused, join=self.join_enc_dec)
        if fused and sws is None:
            sws = self._tail_sws()
        engine.step_bwd(p, g, src, mask, tidx, fw, prob, sv_g, dims, base, mdl.scaler_zeros, red, (self.std, self.mean, a.mape_thresh),
                        self.stats, sws=sws, with_kl=phase == 1, kl=kl)
        self._fold_stats(sws)
        red.flush(tidx)                                           # all parameter-gradient reductions: 3 launches
        engine.CTX.ARENA = engine.CTX.NODE_REDUCE = None
        self._after_backward(phase)

    # ---- what a subclass with another partition of the work replaces (shard.py) ----------------------------------------
    def _noise_buffer(self, phase):
        """Hook: the buffer step_begin fills with the step's mask noise"""
        if self.gmask:
            return self.noise_g if phase == 0 else self.noise_ar_g
        return self.noise if phase == 0 else self.noise_ar

    def _need_guide(self, phase):
        """Hook.  The guide classifier (GPTST.py:325-332) feeds the adaptive mask and the KL term only: the random-mask phase neither generates
        its parameters nor runs it (the reference computes and discards the logits there; GPTST_Model.forward still returns them)"""
        return phase == 1 or self.always_guide

    def _make_mask(self, phase, prob, label, pend):
        """The visibility mask of this rank's cells.  label: the guide's argmax labels (rowdot's by-product, None without the guide);
        pend: the deferred generation jobs, which the mask's launch carries.  The selection covers the cells of _noise_buffer(phase)."""
        a = self.args
        if self.force_mask:
            return self.mask_buf
        noise = self._noise_buffer(phase)                   # Philox / torch.rand noise: k * 2^-24
        if phase == 0:
            mask = ops.mask_random(noise, int(noise.numel() * a.mask_ratio), ws=self._mask_ws(), u24=U24, jobs=pend)
        else:                                               # (class histogram: taken inside)
            noise_a, noise_r = noise.chunk(2)
            mask = ops.mask_adaptive(self._mask_labels(label), None, self.ctrl[:self.HS], self.ctrl[self.HS:], noise_a, noise_r,
                                     a.ada_type == "all", self.base, ws=self._mask_ws(), u24=U24, jobs=pend)[2]
        return self._mask_cut(mask)

    def _mask_labels(self, label):
        """Hook: the labels of the selection's cells (global masks: label_g was gathered by _exchange_labels())"""
        return self.label_g if self.gmask else label

    def _mask_cut(self, mask):
        """Hook: the selection -> this rank's cells (global masks: its rows of the selection over the global batch, identical on every rank)"""
        if not self.gmask:
            return mask
        self.last_mask_global = mask
        return self.dp.rows_of(mask, self.B * self.T * self.N * self.base)

    def _fold_stats(self, sws):
        """Hook: the fused heads' per-workgroup loss statistics -> stats[0..2] (sws None: the unfused loss kernels summed into stats themselves)"""
        if sws is None:
            return
        if self.dp is None:
            self._sws = sws                                                # folded by the optimiser's first launch (one launch less)
        else:
            ops.stats_fold(sws, self.stats)                                # ordered sum: the all-reduce must see them

    def _after_backward(self, phase):
        """Hook: from the finished gradient to the optimiser"""
        if self.dp is None:
            self._optim()
        elif self._dp_in_graph():           # gradient all-reduce + optimiser as the last nodes of the step's graph (no host gap behind the replay)
            if self._dec_reduced:           # the decoder bucket went out under the encoder's backward: what is left is [encoder] and [KL path | never | statistics]
                self._allreduce(self.gbuf[:self.dec_lo])
                self._allreduce(self.gbuf[self.dec_hi:])
            else:
                self._allreduce(self.gbuf)
            self._optim()

    def _tail_sws(self):
        """per-workgroup loss statistics of the two fused heads, zeroed by the step's first launch"""
        return self.arena.zeros(ops.tail_parts(self.B * self.T * self.N), 4)

    def _carry_kl(self, sv_g):
        """the KL path as guests of the forward's chain launches (engine.KlCarry): the plain fused stepper only — not under data parallelism, node
        shards, GPTST_ALWAYS_GUIDE, deterministic or safe mode (GPTST_CARRY_KL=0: never)"""
        return (self.fused_tails and self.dp is None and not self.global_count_scale and not self.deterministic and not self.safe_mode
                and not self.always_guide and engine.CTX.NODE_REDUCE is None and engine.kl_carry_ok(self.dims, self.HS, sv_g))

    def _mask_ws(self):
        """The selections' histogram scratch comes zeroed out of the step's arena (cleared by the step's first launch): no zeroing launch."""
        return self.arena.zeros(ops.mask_ws_floats())

    def _exchange_labels(self):
        """Adaptive phase under DP: ONE all-gather of the int32 cluster labels (261 KB per 32-sample rank), between the two parts."""
        self.dp.gather_labels(self.label_l, out=self.label_g)

    def _optim(self):
        sws, self._sws = self._sws, None
        ops.clip_adam(self.model.flat, self.gflat, self.m, self.v, self.model.nA, self.model.nB, self.hyper, self.stats,
                      stats_out=self.stats_out, sws=sws)

    @contextlib.contextmanager
    def _launch_mode(self):
        """while a step is enqueued or captured: the library's thread-local launch mode (captured into the graph)"""
        if self.DETERMINISTIC_MODE:
            ops.set_deterministic(self.deterministic)
        try:
            yield
        finally:
            if self.DETERMINISTIC_MODE:
                ops.set_deterministic(False)
            engine.CTX.ARENA = engine.CTX.NODE_REDUCE = None

    def _enqueue(self, phase):
        """part 1 [-> label exchange] -> part 2 (+ optimiser when there is no gradient all-reduce in between)"""
        ctx = self._part1(phase)
        if self._needs_exchange(phase):
            self._exchange_labels()
        self._part2(phase, ctx)

    def _body(self, phase):
        with self._launch_mode():
            self._enqueue(phase)

    # ---- host side of one step -------------------------------------------------------------------------------------
    def _phase(self, epoch):
        return 0 if epoch <= self.args.change_epoch else 1

    def _fill(self, row, phase, epoch, list_c):
        """Advance the optimiser counters by one step and write that step's host scalars into `row` (numpy, one pinned record of ops.PinnedRing).
        -> the class order the step runs with (None in the random-mask phase)"""
        a, HS = self.args, self.HS
        self.tA += 1
        if phase == 1:
            self.tB += 1
        self.phase_kl = phase == 1
        tA = self.tA
        # (sum loss: the backward carries the gradient of the SUM loss, the optimiser divides path A by the (global) kept count)
        row[:13].view("float32")[:] = ops.adam_scalars(self.lr, tA, self.tB, 0.9, 0.999, 1e-8, float(a.max_grad_norm) if a.grad_norm else 0.0,
                                                       kl=phase == 1, sum_loss=True)
        row[16 + HS + 2:16 + HS + 4] = (self.noise_seed & 0x7FFFFFFF, tA & 0x7FFFFFFF)          # same key on every rank: same global noise
        if phase == 0:
            return None
        if list_c is None:
            list_c = list(range(HS))
            self.rng.shuffle(list_c)                                   # GPTST.py:357-358
        list_c = [int(v) for v in list_c]
        ada, rnd = self.model.adaptive_counts(self.B * self.T * self.N * (self.W if self.gmask else 1), epoch)
        ada, rnd = self._budgets(ada, rnd, epoch)
        row[16:16 + HS + 2] = list_c + [int(ada), int(rnd)]
        return list_c

    def _budgets(self, ada, rnd, epoch):
        """Hook: subclasses whose masks cover more cells than this rank's batch (node sharding) replace the budgets."""
        return ada, rnd

    def _graphed(self):
        """Hook: does step() replay a captured graph?"""
        return self.use_graph

    def step(self, source, epoch, noise=None, noise_a=None, noise_r=None, list_c=None, forced_mask=None, _sub=None):
        """Enqueue one optimisation step on ``source`` (B,T,N,base+2).  Never synchronises.  Injected noise (tests) covers the cells of the
        selection: the GLOBAL batch with global masks, the GLOBAL nodes of a node shard.
        ``forced_mask`` (fp32, 1 = visible) teacher-forces the mask: used by loss-curve parity runs in the adaptive phase,
        where an fp32-level argmax flip of the cluster classifier would otherwise change which cells are masked.
        ``_sub`` = (group id, j): step_group() running its sub-step j as a single step — ``source`` is the group's j-th buffer."""
        phase = self._phase(epoch)
        forced = forced_mask is not None
        if forced and not self.FORCED_MASK:
            raise ValueError("%s does not teacher-force masks" % type(self).__name__)
        if source is not self.src:
            self.src.copy_(source, non_blocking=True)
        inject = noise is not None or noise_a is not None
        if inject:
            buf = self._noise_buffer(phase)
            if phase == 0:
                buf.copy_(noise.reshape(-1), non_blocking=True)
            else:
                na, nr = buf.chunk(2)
                na.copy_(noise_a.reshape(-1), non_blocking=True)
                nr.copy_(noise_r.reshape(-1), non_blocking=True)
        if forced:
            self.mask_buf.copy_(forced_mask.reshape(-1), non_blocking=True)
        list_c = self._fill(self._ring.next(), phase, epoch, list_c)
        self._ring.send(self.hc)
        key = (phase, inject, forced)
        if not self._graphed():
            self.inject_noise, self.force_mask = inject, forced
            self._body(phase)
        else:
            if key not in self.graphs:
                self._capture(key)
            g1, g2 = self.graphs[key]
            g1.replay()
            if g2 is not None:                          # global masks, adaptive phase: labels are exchanged between the two graphs
                self._exchange_labels()
                g2.replay()
        if self.dp is not None and not self._dp_in_graph():
            self._allreduce(self.gbuf)
            self._optim()
        group, j = _sub if _sub is not None else (next(self._ids), None)
        rec = Enqueued(phase, epoch, list_c, self.rank_weight, self.src, self.stats_out, next(self._ids), group, j)
        if inject or forced:
            rec.src = None
        elif j is not None:                             # the group's own buffers: later plain steps do not write over them
            rec.src, rec.stats = source, self._g_rows[j]
            rec.stats.copy_(self.stats_out)
        self._note(rec, *{None, j})

    def _note(self, rec, *slots):
        """Append to the ledger.  slots: whose buffers this enqueue wrote over (None: self.src / self.stats_out, j: the group's j-th) — the
        records that pointed at them can no longer be read or repeated."""
        for s in slots:
            old = self._holder.get(s)
            if old is not None and old.slot == s:
                old.src = old.stats = None
            self._holder[s] = rec
        self._ledger.append(rec)
        if len(self._ledger) > 4096:                    # (nobody looks: a lost hand-off is then undone for the steps still on record)
            del self._ledger[:2048]

    @property
    def last_replay_steps(self):
        """number of steps the most recent graph replay (eager: enqueue) ran"""
        return sum(1 for r in self._ledger if r.replay == self._ledger[-1].replay)

    def _capture(self, key):
        """Capture the step of `key` = (phase, injected noise, forced mask).  If capturing the collectives of a data-parallel step fails
        (a runtime that cannot record RCCL kernels into a hipGraph raises at capture time, identically on every rank), the step falls back
        to collectives BETWEEN graph replays — the pre-round-3 form — instead of aborting the run."""
        try:
            return self._capture_impl(key)
        except Exception as e:                                    # noqa: BLE001
            if not self._dp_in_graph():
                raise
            import sys
            print("gpt-st_amd: capturing the step with its collectives failed (%s: %s) -> collectives between graph replays"
                  % (type(e).__name__, str(e).splitlines()[0][:200]), file=sys.stderr)
            self._graph_comm_failed = True
            self.graphs.clear()                         # graphs captured earlier hold the in-graph all-reduce + optimiser: replaying them next to
            self._g_graphs.clear()                      # the eager collectives would reduce and step twice
            torch.cuda.synchronize()
            return self._capture_impl(key)

    def _capture_impl(self, key):
        phase, inject, forced = key
        self.inject_noise, self.force_mask = inject, forced
        keep = (self.model.flat.clone(), self.m.clone(), self.v.clone())
        engine.warm_up(lambda: self._body(phase))
        try:
            with self._launch_mode(), engine.quiet_gc():
                g1 = torch.cuda.CUDAGraph()
                if self._needs_exchange(phase) and not self._dp_in_graph():
                    with torch.cuda.graph(g1, capture_error_mode="thread_local"):      # other threads (RCCL watchdog) may call the runtime meanwhile
                        ctx = self._part1(phase)
                    g2 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g2, pool=g1.pool(), capture_error_mode="thread_local"):
                        self._part2(phase, ctx)
                    self._ctx_keep.append(ctx)                                         # part 1's tensors are inputs of graph 2
                else:
                    g2 = None
                    with torch.cuda.graph(g1, capture_error_mode="thread_local"):      # (capturable communicator: the label gather is a graph node)
                        self._enqueue(phase)
        finally:
            self.model.flat.copy_(keep[0]); self.m.copy_(keep[1]); self.v.copy_(keep[2])   # undo the warm-up updates (also when the capture failed)
            torch.cuda.synchronize()
        self.graphs[key] = (g1, g2)

    # ---- several steps per graph replay -----------------------------------------------------------------------------
    # Between two replays of the step graph the device idles for ~19 us (tools/timeline.py on profiles/r03z: 8.8 us from the optimiser's last
    # kernel to the H2D copy of the next step's host scalars, 4.1 us for that copy, 5.8 us until the graph's first kernel) — 1.3 % of a
    # 1.42 ms step.  step_group() enqueues K consecutive optimisation steps (K batches, K optimiser updates, each with its own host
    # scalars, source buffer and statistics snapshot) as ONE graph replay behind ONE H2D copy: the reference's batch loop
    # (BasicTrainer.py:72-103) unrolled K times.  Results are those of K step() calls (tests/test_gpu_step.py).
    def group_ok(self, epoch):
        """A group runs as one graph when the whole step is one graph (no host-side collective inside the step)."""
        phase = self._phase(epoch)
        if self._group_failed:
            return False
        return self.use_graph and (self.dp is None or self._dp_in_graph()) and not (self._needs_exchange(phase) and not self._dp_in_graph())

    def _group_init(self, K):
        if self._gK == K:
            return
        W = self.hc.numel()
        self._gK = K
        self._g_hc = torch.zeros(K, W, dtype=torch.int32, device=self.dev)
        self._g_src = [torch.zeros_like(self.src) for _ in range(K)]
        self._g_stats = torch.zeros(K, 8, device=self.dev)
        self._g_rows = list(self._g_stats.unbind(0))
        self._g_ring = ops.PinnedRing(W, rows=K, slots=self.RING)
        self._g_graphs = {}

    def group_sources(self, K):
        """The K device input buffers (B,T,N,base+2) of a group: fill them (or pass other tensors to step_group, which copies)."""
        self._group_init(K)
        return self._g_src

    def _sub(self, j):
        """Point the per-step buffers of the body at sub-step j of the group (host scalars, source, statistics snapshot)."""
        HS = self.HS
        r = self._g_hc[j]
        self.src, self.stats_out = self._g_src[j], self._g_rows[j]
        self.hyper, self.ctrl, self.rng_words = r[:16].view(torch.float32), r[16:16 + HS + 2], r[16 + HS + 2:]

    def step_group(self, sources, epoch, list_cs=None):
        """Enqueue len(sources) consecutive optimisation steps of the same epoch.  Never synchronises.  Falls back to a loop over step()
        where a step is not one graph (eager mode, host-side collectives).  losses_group() returns the K loss triples.  Either way the
        batches are kept in the group's own buffers (group_sources) until a later group reuses them: the caller's tensors are free at once."""
        K, phase, group = len(sources), self._phase(epoch), next(self._ids)
        list_cs = [None] * K if list_cs is None else list_cs
        grouped = K > 1 and self.group_ok(epoch)
        if grouped or K > self._gK:
            self._group_init(K)
        for j, src in enumerate(sources):
            if src is not self._g_src[j]:
                self._g_src[j].copy_(src, non_blocking=True)
        if not grouped:
            for j in range(K):                          # one replay per step, the same kind of record
                self.step(self._g_src[j], epoch, list_c=list_cs[j], _sub=(group, j))
            return
        if phase not in self._g_graphs:
            # capture BEFORE any per-step state is advanced: if the runtime cannot record this group (e.g. collectives of K steps in one
            # graph), every rank fails alike, the group falls back to K single steps and later groups do not try again
            keep = (self.src, self.stats_out, self.hyper, self.ctrl, self.rng_words)
            try:
                self._capture_group(phase, K, epoch)
            except Exception as e:                                    # noqa: BLE001
                import sys
                print("gpt-st_amd: capturing %d steps in one graph failed (%s: %s) -> one replay per step"
                      % (K, type(e).__name__, str(e).splitlines()[0][:200] if str(e) else ""), file=sys.stderr)
                self._group_failed = True
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
            finally:
                self.src, self.stats_out, self.hyper, self.ctrl, self.rng_words = keep
            if self.dp is not None and getattr(self.dp, "world", 1) > 1 and hasattr(self.dp, "max_over_ranks"):
                # ... and so is the outcome of the capture itself: one rank that could not record the group takes every rank to single steps
                if self.dp.max_over_ranks(1.0 if self._group_failed else 0.0) > 0 and not self._group_failed:
                    self._group_failed = True
                    self._g_graphs.pop(phase, None)
            if self._group_failed:
                return self.step_group(sources, epoch, list_cs)
        rows, replay = self._g_ring.next(), next(self._ids)
        for j in range(K):
            self._note(Enqueued(phase, epoch, self._fill(rows[j], phase, epoch, list_cs[j]), self.rank_weight, self._g_src[j], self._g_rows[j],
                                replay, group, j), j)
        self._g_ring.send(self._g_hc)
        self._g_graphs[phase].replay()

    def _capture_group(self, phase, K, epoch):
        self.inject_noise, self.force_mask = False, False
        keep = (self.model.flat.clone(), self.m.clone(), self.v.clone())
        # the warm-up runs need plausible host scalars in the device table: fill it as the first group would, then put the counters back
        st = (self.tA, self.tB, self.phase_kl, self.rng.getstate())
        rows = self._g_ring.next()
        for j in range(K):
            self._fill(rows[j], phase, epoch, None)
        self._g_ring.send(self._g_hc)
        torch.cuda.synchronize()
        self.tA, self.tB, self.phase_kl = st[:3]
        self.rng.setstate(st[3])
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        subs = iter(range(K))
        engine.warm_up(lambda: (self._sub(next(subs)), self._body(phase)))      # sub-steps 0 and 1 (a group has K >= 2)
        # Activations of the K sub-steps are NOT shared inside one capture (the graph-private pool grew K-fold at N = 4096, C = 128:
        # 4 x 56 GB): groups are for the shapes where the idle time between replays matters, i.e. small steps
        # (decided from the device's TOTAL memory, not from what happens to be free: every rank of a data-parallel job must take the same
        # branch, or their collective sequences diverge)
        per_step = torch.cuda.max_memory_allocated() - base
        total = torch.cuda.get_device_properties(self.dev).total_memory
        if self.dp is not None and getattr(self.dp, "world", 1) > 1 and hasattr(self.dp, "max_over_ranks"):
            # the group / no-group decision is COLLECTIVE: the largest per-step peak any rank measured and the smallest device decide
            # for all of them — ranks whose allocators differ must not take different branches (their collective sequences would diverge)
            per_step = int(self.dp.max_over_ranks(per_step))
            total = -int(self.dp.max_over_ranks(-total))
        if per_step * K > 0.25 * total:
            self.model.flat.copy_(keep[0]); self.m.copy_(keep[1]); self.v.copy_(keep[2])
            torch.cuda.synchronize()
            raise RuntimeError("a group of %d steps would need ~%.0f GB of activations (device: %.0f GB)" % (K, per_step * K / 2**30, total / 2**30))
        try:
            with self._launch_mode(), engine.quiet_gc():
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    for j in range(K):
                        self._sub(j)
                        self._enqueue(phase)
        finally:
            self.model.flat.copy_(keep[0]); self.m.copy_(keep[1]); self.v.copy_(keep[2])   # undo the warm-up updates
            torch.cuda.synchronize()
        self._g_graphs[phase] = g

    def losses_group(self):
        """[(loss, loss_flow, loss_s)] of the steps of the last step_group() (of the last step(): one triple) — synchronises."""
        self._look()
        if not self._ledger:                            # nothing enqueued since the stepper was built / loaded
            return [self._stats_row(self.stats_out.cpu(), bool(self.tB and self.phase_kl))]
        return [self._stats_row(r.row, r.phase == 1) for r in self._ledger]

    def _read(self, recs):
        """statistics of these records -> host: one copy per buffer (a group's table travels whole)"""
        host = {}
        for r in recs:
            if r.stats is not None:
                buf = r.stats if r.slot is None else r.stats._base
                if id(buf) not in host:
                    host[id(buf)] = buf.cpu()
                r.row = host[id(buf)] if r.slot is None else host[id(buf)][r.slot]

    def _look(self):
        """Read the statistics of every step enqueued since the last look, undo a lost hand-off (the one rule of DESIGN.md §15:
        however the steps were enqueued) and keep the last call's records for losses() / losses_group()."""
        led = self._ledger
        new = [r for r in led if r.row is None]         # (they trail the records read before)
        if not new:
            return
        self._read(new)
        first = next((i for i, r in enumerate(new) if r.row is not None and float(r.row[5]) > 0), None)
        if first is not None:
            # A hand-off expired in that step: the guard skipped its update and EVERY later one while the record was up.  The device counts them
            # (row[6]) — steps whose statistics were written over since (bench loops) included, as far as the ledger still knows them.
            n = min(max(len(new) - first, int(new[-1].row[6])), len(new))
            if new[-1].src is None:
                raise RuntimeError("an in-launch hand-off expired in a step with injected mask inputs: call _enter_safe_mode() and repeat the step")
            skipped = new[-n:]
            del led[-n:]
            self._enter_safe_mode(n, sum(r.phase for r in skipped))
            again = [r for r in skipped if r.src is not None]
            if len(again) < n:
                import sys
                self.lost_batches += n - len(again)
                print("gpt-st_amd: %d step(s) enqueued before the last one were skipped with it and cannot be repeated (their batches are gone): "
                      "the optimiser counters were taken back, the batches were not trained on" % (n - len(again)), file=sys.stderr)
            # (a plain step's batch lies in self.src, which every re-run writes: kept aside when it is not the only one)
            srcs = [r.src.clone() if r.src is self.src and len(again) > 1 else r.src for r in again]
            keep_w = self.rank_weight
            try:
                for r, src in zip(again, srcs):         # each the same weighted step (a padding rank of a tail round re-runs as padding)
                    self.rank_weight = r.weight
                    self.step(src, r.epoch, list_c=r.list_c, _sub=None if r.slot is None else (r.group, r.slot))
            finally:
                self.rank_weight = keep_w
            self._read(led[-len(again):])
        led[:] = [r for r in led if r.group == led[-1].group]

    @staticmethod
    def _stats_row(st, kl):
        lf = float(st[0] / max(float(st[1]), 1.0))
        ls = float(st[2]) * 0.1 if kl else 0.0
        return (lf + ls, lf, ls)

    def _enter_safe_mode(self, nsteps, nkl):
        """A hand-off expiry is on record: the last `nsteps` optimiser updates (nkl of them with the KL path) were skipped on the device.  Rewind the
        host's step counters, drop every captured graph (they hold the hand-off launches), clear the record, and from now on enqueue the step
        without in-launch hand-offs.  Collective under data parallelism by construction: the count travels in the all-reduced statistics."""
        import sys
        from . import _C
        torch.cuda.synchronize()
        print("gpt-st_amd: an in-launch hand-off expired (the GPU was shared?) — %d skipped step(s) are re-run without hand-off launches; "
              "this stepper stays in that mode" % nsteps, file=sys.stderr)
        self.tA -= nsteps
        self.tB -= nkl
        self.lost_steps += nsteps
        self.safe_mode = True
        self.graphs.clear()
        self._g_graphs.clear()
        _C.lib().call("gptst_handoff_reset")

    # ---- results ---------------------------------------------------------------------------------------------------
    def losses(self):
        """(loss, loss_flow, loss_s) of the last step — synchronises (reference BasicTrainer.py:98-103 does so every step)."""
        return self.losses_group()[-1]

    # ---- the run's state (checkpoint.py) -------------------------------------------------------------------------------------------
    # What a step sequence depends on besides its batches: weights, Adam moments, the two step counts (bias corrections AND, with noise_seed, the
    # Philox key of the mask noise), the learning rate and the class-order stream.  Moments are stored by parameter name with their true shape,
    # never as the flat buffer: the file does not know about segment order, alignment, node_capacity or ranks.
    def _to_global(self, named):
        """Hook: {key: this rank's device tensor} -> {key: GLOBAL tensor on the CPU} (node shards gather over their group)"""
        return {k: v.detach().cpu().clone() for k, v in named.items()}

    def _to_local(self, named):
        """Hook: {key: global tensor} -> this rank's part"""
        return named

    def state_dict(self):
        """The `model`, `optimizer` and `rng` sections of a checkpoint (checkpoint.py) — synchronises.  Collective where the stepper is."""
        self._look()
        mdl = self.model
        order = {k: i for i, k in enumerate(mdl.param_keys)}
        m, v = ({k: t for k, t in sorted(mdl.views_of(buf).items(), key=lambda kv: order[kv[0]])} for buf in (self.m, self.v))
        return dict(model=self._to_global(mdl.state_dict()),
                    optimizer=dict(exp_avg=self._to_global(m), exp_avg_sq=self._to_global(v), step=self.tA, step_kl=self.tB, lr=float(self.lr)),
                    rng=dict(noise_seed=int(self.noise_seed), class_order=self.rng.getstate()))

    def _stage_flat(self, named, what):
        """{key: this rank's tensor} -> a CPU image of a flat buffer in this model's layout; what no parameter owns (alignment, capacity padding) is zero"""
        mdl = self.model
        img = torch.zeros(mdl.flat.numel(), dtype=torch.float32)
        for k, view in mdl.views_of(img).items():
            if k not in named:
                raise KeyError("the checkpoint's %s lack %r" % (what, k))
            if tuple(named[k].shape) != tuple(view.shape):
                raise ValueError("%s of %s: the checkpoint holds shape %s, this model %s" % (what, k, tuple(named[k].shape), tuple(view.shape)))
            view.copy_(named[k])
        return img

    def load_state_dict(self, sd):
        """Continue from the `model`, `optimizer` and `rng` sections of a checkpoint.  Weights and moments are copied INTO the existing buffers: graphs
        captured before stay valid, steppers that alias m / v (the trainer's ragged-batch steppers) keep sharing them."""
        from .checkpoint import rng_state
        mdl, opt = self.model, sd["optimizer"]
        images = [self._stage_flat(self._to_local(named), what)
                  for named, what in ((sd["model"], "weights"), (opt["exp_avg"], "exp_avg"), (opt["exp_avg_sq"], "exp_avg_sq"))]
        self._look()                                   # nothing of this stepper's is in flight when its buffers change
        for dst, img in zip((mdl.flat, self.m, self.v), images):
            dst.copy_(img)
        for k, b in mdl.named_buffers():
            b.copy_(sd["model"][k])
        self.tA, self.tB, self.lr = int(opt["step"]), int(opt["step_kl"]), float(opt["lr"])
        self.noise_seed = int(sd["rng"]["noise_seed"])
        self.rng.setstate(rng_state(sd["rng"]["class_order"]))
        del self._ledger[:]
        self.lost_steps = self.lost_batches = 0
