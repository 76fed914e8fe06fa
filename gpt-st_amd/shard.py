"""Node-sharded pretraining step (BASELINE config 5: N = 4096 split 512 nodes per GPU).

Every rank owns a contiguous range of nodes [n0, n1): its slice of the input, of the node-indexed parameters
(``*.node_embeddings``, ``*.node_embeddings_spg``, ``encoder.neb4mask``, ``*.cap{1,2}.adj``) and of every activation.
hyperTem, MLP_RL, the in/out projections and the per-node parts of ``cap`` are node-local.  The only sums over nodes are the
cluster aggregations ``S = c . P`` of ``cap`` (R+2 = 4 per forward, 1 per backward: ``dv = sum_n c drec``); each is ONE kernel
(ops._capbig_type1) followed by ONE all-reduce of (B*T, HS, C) floats.  The cross-time hyperedge block of ``cap`` runs replicated
on the all-reduced ``s``, so the gradients it produces (``t_adj``, ``time_feature2``) are identical on every rank and are scaled
by 1/world before the gradient all-reduce.  Gradients of shared parameters: one all-reduce of the flat buffer (node-local slices
are zeroed before and put back afterwards — they belong to this rank alone); the global gradient norm is the reduced buffer's plus
every rank's node-local squared norm (one scalar all-reduce), formed alike on every rank and handed to the optimiser as the total.
Masks: the selection runs replicated over the GLOBAL (B,T,N) cells from identical noise and each
rank keeps its node columns; the adaptive phase all-gathers the per-cell cluster labels and sums the class counts.
Shards come from node_ranges() and may differ in width by one node: the label gather pads to the widest shard, and the models are built
with node_capacity = that width (model.py), so that the flat gradient buffer has the same layout on every rank.
Loss statistics (sum |e|, kept count, KL sum) travel in the tail of the gradient buffer, as in dist.py.

The collectives go through a small group object: ``DistNodeGroup`` (torch.distributed, RCCL on GPUs), ``NativeNodeGroup`` (the C-ABI
communicator of csrc/comm.hip: plain enqueues on the launch stream) or ``ThreadNodeGroup`` (ranks emulated by threads on ONE GPU —
how the tests check the protocol against the unsharded step).  A group whose collectives are stream-ordered device work
(``capturable``: world = 1, or NativeNodeGroup) lets the whole step — kernels AND collectives — be captured in ONE hipGraph per phase
(``use_graph``); otherwise the step is enqueued eagerly, the collectives sitting between the kernels.
"""
import os
import threading

import torch

from . import engine, ops
from .step import PretrainStep


def is_node_local(key):
    return (key.endswith("node_embeddings") or key.endswith("node_embeddings_spg") or key == "encoder.neb4mask"
            or (key.endswith(".adj") and ".cap" in key))


def is_replicated_compute(key):
    """Parameters whose gradient is computed identically on every rank (cross-time block on the all-reduced cluster capsules)."""
    return key.endswith(".t_adj") or ".time_feature2." in key


def node_ranges(N, world):
    """The node split of a sharded run: [(n0, n1)] per rank, contiguous and in rank order; the first N % world ranks own one node more
    (170 over 8: 22, 22, 21, 21, 21, 21, 21, 21).  Every bound of a node shard comes from here."""
    N, world = int(N), int(world)
    if world < 1:
        raise ValueError("node sharding needs at least one rank, got world = %d" % world)
    if world > N:
        raise ValueError("cannot split %d nodes over %d ranks: every rank needs at least one node" % (N, world))
    q, r = divmod(N, world)
    out, n0 = [], 0
    for k in range(world):
        n1 = n0 + q + (1 if k < r else 0)
        out.append((n0, n1))
        n0 = n1
    return out


def gather_node_columns(group, local, widths, pad=None):
    """(..., n_rank) of every rank -> (..., N): the last axis zero-padded to the widest shard for the group's all-gather, then trimmed and
    concatenated in rank (= node) order.  pad: a (..., max(widths)) buffer to reuse (its padding columns must be zero)."""
    n = local.shape[-1]
    if pad is None:
        pad = local.new_zeros(tuple(local.shape[:-1]) + (max(widths),))
    pad[..., :n].copy_(local)
    g = group.all_gather(pad)                                             # (W, ..., wmax)
    return torch.cat([g[r, ..., :w] for r, w in enumerate(widths)], dim=-1)


def _pad_nodes(key, t, width):
    """a node-local tensor zero-padded to `width` nodes along its node axis (the last one for cap*.adj, the first otherwise)"""
    adj = key.endswith(".adj")
    n = t.shape[-1] if adj else t.shape[0]
    if n == width:
        return t.contiguous()
    shape = list(t.shape)
    shape[-1 if adj else 0] = width
    out = t.new_zeros(shape)
    (out[..., :n] if adj else out[:n]).copy_(t)
    return out


def gather_state_dict(group, local_sd, ranges):
    """Collective: every rank's node-local tensors (padded to the widest shard, all-gathered, trimmed) assembled with the shared ones into the
    GLOBAL state dict — the keys, shapes and order of an unsharded model (the reference's checkpoint format).  Returned on every rank."""
    widths = [n1 - n0 for n0, n1 in ranges]
    wmax = max(widths)
    parts = [dict() for _ in ranges]
    for k, v in local_sd.items():
        if is_node_local(k):
            g = group.all_gather(_pad_nodes(k, v, wmax))                  # (W, ...)
            for r, w in enumerate(widths):
                parts[r][k] = g[r][..., :w] if k.endswith(".adj") else g[r][:w]
        else:
            for p_ in parts:
                p_[k] = v
    return unshard_state_dicts(parts)


def shard_state_dict(sd, n0, n1):
    """Global state dict -> this rank's (node-indexed tensors sliced to [n0, n1))."""
    out = {}
    for k, v in sd.items():
        if is_node_local(k):
            out[k] = (v[..., n0:n1] if k.endswith(".adj") else v[n0:n1]).clone()
        else:
            out[k] = v.clone()
    return out


def unshard_state_dicts(sds):
    """Inverse of shard_state_dict for a list of per-rank state dicts (rank order = node order)."""
    out = {}
    for k, v in sds[0].items():
        if is_node_local(k):
            out[k] = torch.cat([sd[k] for sd in sds], dim=-1 if k.endswith(".adj") else 0)
        else:
            out[k] = v.clone()
    return out


class DistNodeGroup:
    """Collectives of a node-sharded run over torch.distributed (nccl = RCCL over xGMI on the GPUs)."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world
        self.capturable = world == 1                     # one rank: the collectives are no-ops / device copies

    def all_reduce_(self, t):
        import torch.distributed as dist
        if self.world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t

    def all_gather(self, t):
        """-> (world, *t.shape)"""
        import torch.distributed as dist
        flat = t.contiguous().view(-1)
        out = torch.empty(self.world * flat.numel(), dtype=t.dtype, device=t.device)      # concatenation form (gloo and nccl)
        if self.world == 1:
            out.copy_(flat)
        else:
            dist.all_gather_into_tensor(out, flat)
        return out.view((self.world,) + tuple(t.shape))


class NativeNodeGroup:
    """The same collectives on the C-ABI communicator (dist.NativeComm: RCCL bound at run time, every call a plain enqueue on torch's
    current stream), so they can sit INSIDE a captured hipGraph.  The library reduces fp32 only: integer payloads (class counts, cluster
    labels) travel as exactly representable floats (< 2^24), and the all-gather is an all-reduce of a buffer in which every rank fills its
    own slot."""
    capturable = True

    def __init__(self, comm):
        self.comm, self.rank, self.world = comm, comm.rank, comm.world

    def all_reduce_(self, t):
        if t.dtype == torch.float32:
            if t.is_contiguous():
                self.comm.allreduce_(t)
            else:                                   # reduce a contiguous copy and write the sums back (an in-place reduce of the copy would be lost)
                f = t.contiguous()
                self.comm.allreduce_(f)
                t.copy_(f)
            return t
        if t.dtype == torch.float64:
            # (metric sums, once per run) each rank's values as hi + lo fp32 words in its own slot: every element of the reduced buffer has ONE
            # nonzero contributor, so the fp32 all-reduce is exact, and the sum over the ranks is taken in float64 afterwards (~48-bit values)
            flat = t.contiguous().view(-1)
            buf = torch.zeros(self.world, 2, flat.numel(), dtype=torch.float32, device=t.device)
            hi = flat.to(torch.float32)
            buf[self.rank, 0].copy_(hi)
            buf[self.rank, 1].copy_((flat - hi.to(torch.float64)).to(torch.float32))
            self.comm.allreduce_(buf)
            t.copy_(buf.to(torch.float64).sum(dim=(0, 1)).view(t.shape))
            return t
        f = t.to(torch.float32)
        self.comm.allreduce_(f)
        t.copy_(f.to(t.dtype))
        return t

    def all_gather(self, t):
        """-> (world, *t.shape)"""
        buf = torch.zeros((self.world,) + tuple(t.shape), dtype=torch.float32, device=t.device)
        buf[self.rank].copy_(t)
        self.comm.allreduce_(buf)
        return buf.to(t.dtype)


class ThreadNodeGroup:
    """The same collectives between `world` threads of one process sharing one GPU stream (tests).  Kernels of all threads land
    on the same stream in enqueue order, and a barrier separates 'everybody has enqueued its contribution' from the sum."""

    capturable = False

    class Shared:
        def __init__(self, world):
            self.world = world
            self.barrier = threading.Barrier(world)
            self.slots = [None] * world

    def __init__(self, rank, shared):
        self.rank, self.world, self.sh = rank, shared.world, shared

    def all_reduce_(self, t):
        sh = self.sh
        sh.slots[self.rank] = t
        sh.barrier.wait()
        total = sh.slots[0].clone()
        for r in range(1, self.world):
            total += sh.slots[r]
        sh.barrier.wait()                      # everybody has read every slot
        t.copy_(total)
        sh.barrier.wait()
        return t

    def all_gather(self, t):
        sh = self.sh
        sh.slots[self.rank] = t
        sh.barrier.wait()
        out = torch.stack([sh.slots[r] for r in range(self.world)])
        sh.barrier.wait()
        return out


class ShardedPretrainStep(PretrainStep):
    """One optimisation step of a rank that owns nodes [n0, n1) of N (node_ranges: shard widths may differ by one).  Unequal shards
    need models built with node_capacity = the widest shard, so that [flat gradient | statistics] has the same layout on every rank."""
    DETERMINISTIC_MODE = False      # the sharded step has never taken the bit-reproducible launch forms: GPTST_DETERMINISTIC is not read here
    FORCED_MASK = False             # ... nor teacher-forced masks

    def __init__(self, model_local, args_local, n_global, group, scaler_mean, scaler_std, batch_size, seed=0, use_graph=None):
        """use_graph: None = capture the step in a hipGraph when the group's collectives are capturable (see the module docstring)."""
        super().__init__(model_local, args_local, scaler_mean, scaler_std, batch_size, use_graph=False, dp=None, seed=seed)
        self.shard_graph = bool(getattr(group, "capturable", False)) if use_graph is None else bool(use_graph)
        assert not self.shard_graph or getattr(group, "capturable", False), "this group's collectives cannot be captured"
        # r05: the node-local part of the step is the fused step's — loss / KL heads with their backward in one pass each (their per-workgroup
        # statistics are folded into the gradient buffer's tail BEFORE the all-reduce), the dPre chain, hyperTem forward chains and backward
        # pairs, the low-rank first layers.  Only the cluster aggregations of cap keep their all-reduce form (engine.CTX.NODE_REDUCE).
        self.fused_tails = (os.environ.get("GPTST_FUSED_TAILS", "1") == "1" and os.environ.get("GPTST_SHARD_FUSED", "1") == "1"
                            and engine.fused_tails_ok(model_local.param_views(), self.C, self.base, self.HS))
        self.group, self.Ng = group, n_global
        self.Nl = args_local.num_nodes
        self.ranges = node_ranges(n_global, group.world)
        self.widths = [n1 - n0 for n0, n1 in self.ranges]
        if self.ranges[0][0] != 0 or self.ranges[-1][1] != n_global or any(a[1] != b[0] for a, b in zip(self.ranges, self.ranges[1:])):
            raise ValueError("node ranges %s do not cover the %d nodes" % (self.ranges, n_global))
        self.n0, self.n1 = self.ranges[group.rank]
        if self.n1 - self.n0 != self.Nl:
            raise ValueError("rank %d owns nodes [%d, %d) of %d over %d ranks, but its model was built with num_nodes = %d"
                             % (group.rank, self.n0, self.n1, n_global, group.world, self.Nl))
        # adaptive phase, unequal shards: this rank's labels travel padded to the widest shard (gather_node_columns)
        self.label_pad = (torch.zeros(self.B, self.T, max(self.widths), dtype=torch.int32, device=self.dev)
                          if group.world > 1 and min(self.widths) != max(self.widths) else None)
        self._eval_gen = None
        self._check_agreement()
        Mg = self.B * self.T * self.Ng
        torch.cuda.manual_seed(7654321 + seed)              # identical global mask noise on every rank
        self.noise_g = torch.zeros(Mg * self.base, device=self.dev)
        self.noise_ar_g = torch.zeros(2 * Mg, device=self.dev)      # adaptive phase: [noise_a | noise_r] over the GLOBAL cells, drawn by ONE launch
        self.noise_a_g, self.noise_r_g = self.noise_ar_g[:Mg], self.noise_ar_g[Mg:]
        self.tail = None                                    # single stream: collectives order against everything
        self.global_count_scale = True
        # ---- where this step differs from PretrainStep's body besides the hooks below ----
        self.node_reduce = group.all_reduce_                # cap's cluster aggregations sum over all ranks' nodes
        self.join_enc_dec = self.fused_tails                # the unfused sharded step runs encoder hyperTem4 / decoder hyperTem1 as launches of their own
        named = dict(model_local.named_parameters())
        self.local_keys = [k for k in named if is_node_local(k)]
        self.repl_keys = [k for k in named if is_replicated_compute(k)]
        self.segA = {k: model_local._offs[k] < model_local.nA for k in self.local_keys}
        # node-local gradients are kept out of the gradient all-reduce by a save / restore around it: ONE flat buffer, [reconstruction-path keys |
        # KL-path keys], moved by multi-tensor copies (r05: a clone, a copy and three norm launches PER KEY before — ~95 tiny launches per step).
        # Each key's WHOLE slot travels (node_capacity, model.py): the all-reduce adds the wider ranks' node-local gradients into a narrower
        # rank's padding, and the restore writes the padding's zeros back over them — the padding stays zero in gradients, moments and weights
        # and every rank's clip norm sees the same set of values.
        ordered = [k for k in self.local_keys if self.segA[k]] + [k for k in self.local_keys if not self.segA[k]]
        sizes = [model_local._slot_numel[k] for k in ordered]
        self.keep_flat = torch.zeros(sum(sizes), device=self.dev)
        self.keep_nA = sum(n for k, n in zip(ordered, sizes) if self.segA[k])
        offs = [sum(sizes[:i]) for i in range(len(sizes))]
        self.keep_views = [self.keep_flat[o:o + n] for o, n in zip(offs, sizes)]
        self.keep_grads = [self.gflat[model_local._offs[k]:model_local._offs[k] + n] for k, n in zip(ordered, sizes)]
        self.repl_grads = [self.g[k] for k in self.repl_keys]

    def _check_agreement(self):
        """The collectives of a step assume the same flat layout, the same loss-head form and the same launch form on every rank; a rank that
        disagrees would sum unrelated parameters or wait in a collective nobody else enters.  Checked once, collectively: every rank fills its
        row of a small table (the fingerprint in 12-bit digits, exact in fp32 on every group) and ONE all-reduce gives every rank all rows; the
        column-wise min and max then differ on every rank or on none."""
        W = self.group.world
        if W == 1:
            return
        mdl = self.model
        order = sorted(mdl._offs, key=mdl._offs.get)
        names = ["flat.numel()", "fused_tails", "shard_graph"]
        fp = [mdl.flat.numel(), int(self.fused_tails), int(self.shard_graph)]
        for i, k in enumerate(order):          # where the shared parameters resume after each node-local one (node_capacity)
            if is_node_local(k):
                nxt = next((q for q in order[i + 1:] if not is_node_local(q)), None)
                names.append("offset of %s (after %s)" % (nxt, k))
                fp.append(mdl._offs[nxt] if nxt is not None else -1)
        L = 32
        vals = ([v + 1 for v in fp] + [0] * L)[:L]
        digits = [(v >> s) & 4095 for v in vals for s in (0, 12, 24)]
        table = torch.zeros(W, 3 * L, device=self.dev)
        table[self.group.rank] = torch.tensor(digits, dtype=torch.float32, device=self.dev)
        self.group.all_reduce_(table)
        bad = (table.amax(0) != table.amin(0)).view(L, 3).any(1).cpu()
        if bool(bad.any()):
            t = table.view(W, L, 3).cpu().to(torch.int64)
            rows = t[..., 0] + (t[..., 1] << 12) + (t[..., 2] << 24) - 1
            what = ["%s: %s" % (names[i] if i < len(names) else "entry %d" % i, rows[:, i].tolist()) for i in range(L) if bad[i]]
            raise RuntimeError("node shards disagree on what their collectives depend on (values per rank) — %s.  Shards of unequal width "
                               "need models built with node_capacity = the widest shard." % "; ".join(what))

    def _gather_labels(self, label, B):
        """this rank's cluster labels of (B,T,Nl) cells -> the (B,T,N) labels of the global cells, flat, node order"""
        if self.group.world == 1:
            return label.reshape(-1)
        lab = label.view(B, self.T, self.Nl)
        if self.label_pad is None:                                                     # equal shards
            return self.group.all_gather(lab).permute(1, 2, 0, 3).contiguous().view(-1)   # (W,B,T,Nl) -> (B,T,N)
        pad = self.label_pad if B == self.B else None
        return gather_node_columns(self.group, lab, self.widths, pad=pad).reshape(-1)

    # global mask -> this rank's node columns
    def _cols(self, flat_global, per_cell, B=None):
        B = self.B if B is None else B
        return flat_global.view(B, self.T, self.Ng, per_cell)[:, :, self.n0:self.n1].contiguous().view(-1)

    def _noise_buffer(self, phase):
        """the GLOBAL mask noise (Philox keyed by [seed, step]: identical on every rank)"""
        return self.noise_g if phase == 0 else self.noise_ar_g

    def _need_guide(self, phase):
        """the fused form skips the classifier in the random-mask phase; the unfused form always runs it (GPTST_ALWAYS_GUIDE is not read here)"""
        return phase == 1 or not self.fused_tails

    def _mask_labels(self, label):
        """the guide's argmax labels of the local cells -> of the GLOBAL cells (the class histogram is taken from the gathered labels)"""
        return self._gather_labels(label, self.B)

    def _mask_cut(self, mask):
        """the selection over the GLOBAL cells, cut to this rank's node columns"""
        self.last_mask_global = mask
        return self._cols(mask, self.base)

    def _fold_stats(self, sws):
        """always into the gradient buffer's tail, which the all-reduce moves.  Unfused (sws None): a zero row — only the fold's other job, stats[5] <-
        this rank's hand-off expiries, so that every rank skips the update and re-runs the step together, as on the fused path"""
        ops.stats_fold(sws if sws is not None else self.arena.zeros(1, 4), self.stats)

    def _graphed(self):
        """one hipGraph per (phase, injected noise), kernels and collectives: the base class's capture"""
        return self.shard_graph

    def group_ok(self, epoch):
        """a sharded stepper never runs a group as one graph"""
        return False

    def _fill(self, row, phase, epoch, list_c):
        list_c = super()._fill(row, phase, epoch, list_c)
        row[13:14].view("float32")[0] = 1.0 if self.group.world > 1 else 0.0     # the optimiser clips by the norm _after_backward leaves in stats[3]
        return list_c

    def _after_backward(self, phase):
        # ---- gradients: replicated-compute parameters count once, node-local ones stay local, the rest is summed ----
        W = self.group.world
        if W > 1:
            if self.repl_grads:
                torch._foreach_mul_(self.repl_grads, 1.0 / W)
            torch._foreach_copy_(self.keep_views, self.keep_grads)
            torch._foreach_zero_(self.keep_grads)                  # (so that the reduced buffer is the shared gradient alone, the same bits on every rank)
        self.group.all_reduce_(self.gbuf)                          # [flat gradient | loss statistics]
        if W > 1:
            # global gradient norm = shared part + every rank's node-local part (reconstruction-path gradients are still unnormalised sums: scaled by
            # 1 / kept cells like the optimiser does).  Every rank adds the same words in the same order — the shared part from the reduced buffer
            # while the node-local slots are still zero, the node-local parts through one scalar all-reduce — and hands the optimiser the TOTAL
            # (hyper[13]): a rank that summed its own gradient buffer instead had its node-local part mixed in, rounded the total differently in
            # the last bit, clipped by another scale and left the replicas one ulp apart after a single step (ragged shards, W = 3).
            nA, nB = self.model.nA, self.model.nB
            # (dot products: one pass over each segment, no temporaries — 3 launches in the random phase, 5 with the KL path)
            sa2 = (1.0 / torch.clamp(self.stats[1], min=1.0)) ** 2
            gA, kA = self.gflat[:nA], self.keep_flat[:self.keep_nA]
            shared = (torch.dot(gA, gA) * sa2).view(1)
            own = (torch.dot(kA, kA) * sa2).view(1)
            if phase == 1:
                gB, kB = self.gflat[nA:nA + nB], self.keep_flat[self.keep_nA:]
                shared = shared + torch.dot(gB, gB)
                if kB.numel():
                    own = own + torch.dot(kB, kB)
            self.group.all_reduce_(own)
            self.stats[3] = (shared + own)[0]
            torch._foreach_copy_(self.keep_grads, self.keep_views)
        self._optim()

    def _budgets(self, ada, rnd, epoch):
        return self.model.adaptive_counts(self.B * self.T * self.Ng, epoch)      # mask budgets over the GLOBAL cell count

    def evaluate(self, source, epoch, noise=None, noise_a=None, noise_r=None, list_c=None):
        """Forward only (the end-of-training report of a node-sharded run): guide, global mask, encoder, decoder with its head — the first half of
        the step's body in the form GPTST_Model.forward takes.  No backward, no optimiser step, no counter moves.  source: this rank's (B',T,Nl,base+2)
        slice, any batch size.  Injected noise covers the GLOBAL cells; what is not injected is drawn from generators this evaluator owns, seeded
        from the run's seed and identical on every rank (not the process-wide ones: ranks emulated by threads share those).
        -> (out (B',T,Nl,base), visibility mask (B',T,Nl,base) fp32, 1 = visible) of this rank's cells."""
        import random
        mdl, a, base = self.model, self.args, self.base
        src = source.to(self.dev).contiguous().float()
        B, T = src.shape[0], src.shape[1]
        dims = (B, T, self.Nl, self.C)
        Mg = B * T * self.Ng
        if self._eval_gen is None:
            seed = int(getattr(a, "seed", 0))
            self._eval_gen = torch.Generator(device=self.dev)
            self._eval_gen.manual_seed(9876543 + seed)
            self._eval_rng = random.Random(seed)
        rand = lambda n: torch.rand(n, device=self.dev, generator=self._eval_gen)      # noqa: E731
        p = mdl.param_views()
        ctx = engine.CTX
        ctx.NODE_REDUCE = self.group.all_reduce_
        try:
            with torch.no_grad():
                tidx = mdl._tidx(src)
                gen = engine.gen_all(p, tidx, dims)
                prob, _ = engine.guide_fwd(p, src, tidx, dims, base, gen=gen.guide)
                if epoch <= a.change_epoch:
                    noise = rand(Mg * base) if noise is None else noise.to(self.dev).reshape(-1).contiguous()
                    mask_g = ops.mask_random(noise, int(Mg * base * a.mask_ratio))
                else:
                    label_g = self._gather_labels(ops.mask_labels(prob.reshape(B * T * self.Nl, -1))[0], B)
                    if list_c is None:
                        list_c = list(range(self.HS))
                        self._eval_rng.shuffle(list_c)
                    na = rand(Mg) if noise_a is None else noise_a.to(self.dev).reshape(-1).contiguous()
                    nr = rand(Mg) if noise_r is None else noise_r.to(self.dev).reshape(-1).contiguous()
                    lc = torch.tensor([int(v) for v in list_c], dtype=torch.int32, device=self.dev)
                    nums = torch.tensor(mdl.adaptive_counts(Mg, epoch), dtype=torch.int32, device=self.dev)
                    mask_g = ops.mask_adaptive(label_g, None, lc, nums, na, nr, a.ada_type == "all", base)[2]
                mask = self._cols(mask_g, base, B)
                out = engine.autoencoder_fwd(p, src, mask, dims, base, mdl.num_route, mdl.scaler_zeros, gen=gen, tidx=tidx, join=False).out
        finally:
            ctx.NODE_REDUCE = None
        return out.view(B, T, self.Nl, base), mask.view(B, T, self.Nl, base)

    # ---- the run's state: GLOBAL tensors in the file, this rank's node range in its buffers (both collective) -------------------------
    def _to_global(self, named):
        full = gather_state_dict(self.group, {k: v.detach() for k, v in named.items()}, self.ranges)
        return {k: v.cpu().clone() for k, v in full.items()}

    def _to_local(self, named):
        return shard_state_dict(named, self.n0, self.n1)

    def _padding(self):
        """mask of the flat buffer's elements no parameter owns (node_capacity padding, alignment)"""
        mdl = self.model
        pad = torch.ones(mdl.flat.numel(), dtype=torch.bool)
        for k, t in mdl.named_parameters():
            pad[mdl._offs[k]:mdl._offs[k] + t.numel()] = False
        return pad.to(self.dev)

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        pad = self._padding()
        if bool(pad.any()):
            worst = max(float(buf[pad].abs().max()) for buf in (self.model.flat, self.m, self.v))
            assert worst == 0.0, "node_capacity padding is not zero after the load (largest |value| %g)" % worst
