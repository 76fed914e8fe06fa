"""Hand-written forward / backward of the GPT-ST pretraining network on the HIP kernels (no torch autograd inside).

Every ``*_fwd`` returns ``(outputs..., saved)`` and every ``*_bwd`` ACCUMULATES parameter gradients into the tensors of a
gradient dict ``g`` (views into one flat buffer) and returns the input gradients.  ``p`` / ``g`` map the reference's
state_dict keys to tensors.  Citations: reference model/Pretrain_model/GPTST.py.
"""
import contextlib
import gc
import os
import threading
from typing import Any, NamedTuple

import torch

from . import _C, ops
from .ops import (EPI_ADD_DPRE, EPI_ADD_PREMUL, EPI_LRELU, EPI_PREMUL, EPI_PLAIN, EPI_RES_LRELU, MODE_NODE, MODE_SHARED, MODE_TIME, PRO_DPRE, PRO_NONE)

TF_NAMES = ("ln_day", "ln_week", "ln1", "ln2", "ln")


class ZeroArena:
    """All zero-initialised scratch of one step (bias-gradient accumulators, embedding gradients) comes from ONE buffer that
    is cleared with ONE memset per step instead of ~30 torch.zeros launches.  The first (sizing) pass falls back to torch.zeros."""

    def __init__(self, device):
        self.device, self.buf, self.off, self.need = device, None, 0, 0

    def begin(self, zero=True):
        """-> the buffer the caller has to zero itself when zero=False (None when there is none or it was just created zeroed)"""
        pending = None
        if self.buf is None or self.buf.numel() < self.need:
            self.buf = torch.zeros(max(self.need, 1), device=self.device) if self.need else None
        elif self.buf is not None:
            if zero:
                self.buf.zero_()
            else:
                pending = self.buf
        self.off, self.need = 0, 0
        return pending

    def zeros(self, *shape):
        n = 1
        for d in shape:
            n *= d
        n4 = (n + 3) // 4 * 4
        self.need += n4
        if self.buf is None or self.off + n4 > self.buf.numel():
            return torch.zeros(*shape, device=self.device)
        t = self.buf[self.off:self.off + n].view(*shape)
        self.off += n4
        return t


class _Context(threading.local):
    """Per-thread execution context of a step (thread-local so that several shard steppers can run side by side in one process:
    tests emulate the ranks of a node-sharded run with threads).
      ARENA        ZeroArena of the running step (None -> plain torch.zeros)
      NODE_REDUCE  node-sharded run: callable that completes a sum over nodes across the ranks, in place (None -> single shard)
      NO_HANDOFFS  the step is enqueued without launches in which one workgroup waits for another (no_handoffs(): a stepper in safe mode) — per
                   thread, so that one emulated rank in safe mode does not change the launches another thread is enqueuing"""
    ARENA = None
    NODE_REDUCE = None
    NO_HANDOFFS = False


CTX = _Context()


# (r05: the side-stream modes of rounds 1-3 — weight gradients, reductions, parameter generation and the KL backward on a second stream / graph
#  branch — were each measured slower than the single chain (DESIGN.md sections 7-8: 364 vs 403, 558-579 vs 597, 651 / 659 vs 675 steps/s) and left
#  the engine; the one fork that remains is the data-parallel gradient bucket's all-reduce, Reductions.flush_async.)


class Reductions:
    """Everything of a backward pass that only produces PARAMETER gradients from per-layer partial results — the sums of the
    generated weights' gradients into their pools and embeddings (GPTST.py:24-25,29-30,104,129,137-138,156,160-161 backward), the
    temporal-graph factor gradients and the seven time-feature MLPs — is collected here while the data-gradient chain runs and
    executed at the end of the backward as THREE launches (gram_bwd, one job table, one time-feature job table) instead of ~20
    small launches per STHCN.  Nothing on the critical chain waits for these results; only the optimiser does.  In the tail-role form
    (tail_roles_ok) the job table has no launch of its own: the encoder's first-layer backward, gram_bwd and the time-feature backward carry it."""

    def __init__(self):
        self.jobs = ops.PoolJobs()   # reductions whose inputs are complete when they are queued (their producer has been launched)
        self.late = ops.PoolJobs()   # reductions over dA, which gram_bwd writes in _run(): never carried by an earlier launch
        self.no_carry = False        # (deterministic steppers: one reduction launch, as the single-owner kind-2 launch groups by target)
        self.grams = []          # (A (L*N,Hm,T), dG (L*N,T,T), dA out)
        self.tf = []             # ops.TimefeatJob with grads and dout
        self.keep = []
        self.on_bucket = None    # callable(k): gradient bucket k is complete (k = 0: the decoder's) — called on the forked stream, right behind
        self.nbucket = 0         # the reductions that finish it, so a data-parallel step can enqueue that bucket's all-reduce under the rest of the backward
        self.bucket_inline = False   # flush_async() runs the bucket's reductions on the calling stream and forks only on_bucket, onto fork_side
        self.fork_side = None
        self.forked = False          # a fork is open: flush() joins it
        self._dG = self._dA = None   # graph / factor gradient buffers shared by the step's STHCNs (_grad_buffers)
        self.want_tail = False       # the caller's step may end its backward in the tail-role form (the fused steppers: step.py)
        self.tail = False            # ... and this step does (tail_roles_ok, decided by step_bwd): the last three launches carry the reductions

    def take_carry(self, mb):
        """Up to `mb` MB of the queued reductions for a backward launch that carries them as role workgroups (ops.cap_cross_route_lin_bwd jobs=): the
        decoder's reductions under the encoder's routing backward.  None: nothing to carry / not in this step (data-parallel bucket overlap: the bucket's
        reductions run where the bucket closes; node shards; deterministic mode)."""
        if not CARRY_RED or self.no_carry or self.on_bucket is not None or CTX.NODE_REDUCE is not None or not self.jobs.jobs:
            return None
        take, rest, nb = [], [], 0.0
        for j in self.jobs.jobs:
            b = 4.0 * j.R * j.cols * j.nsplit / 2 ** 20
            if j.kind in (ops.PoolJobs.BWD_POOL, ops.PoolJobs.BWD_EMB) and nb + b <= mb and len(take) < 100 and (j.cols | j.ldx) % 4 == 0:     # (float4-shaped jobs only)
                take.append(j); nb += b
            else:
                rest.append(j)
        if not take:
            return None
        self.jobs.jobs = rest
        c = ops.PoolJobs()
        c.jobs = take
        return c

    def take_all(self):
        """every queued reduction, for the launch that carries them at the end of the backward (tail roles: ops.encin_ht1_bwd jobs=)"""
        c = ops.PoolJobs()
        c.jobs, self.jobs.jobs = self.jobs.jobs, []
        return c

    def untake(self, carry):
        if carry is not None and carry.jobs:
            self.jobs.jobs = carry.jobs + self.jobs.jobs
            carry.jobs = []

    def gram(self, A, dG, dA, N, nsG):
        """A (L*N,Hm,T), dG (L, nsG, N, T, T) partial graph gradients, dA (L*N,Hm,T) output"""
        self.grams.append((A, dG, dA, N, nsG))

    def timefeat(self, p, g, pfx, tidx, dout, spg=False):
        self.tf.append(_tf_job(p, pfx, tidx, spg)._replace(grads=_tf_tensors(g, pfx), dout=dout))

    def flush_async(self, tidx):
        """A gradient bucket is complete (a data-parallel step, GPTST_DP_OVERLAP=1; no-op otherwise): its reductions run HERE, on the calling
        stream (as a side branch their ~1300 bandwidth-bound workgroups slowed the chain they ran under by more than they hid: 717 vs 752
        steps/s at one rank), and only the bucket's all-reduce — a few RCCL workgroups — is forked under the rest of the backward."""
        if self.bucket_inline and self.on_bucket is not None and self.nbucket == 0 and (self.jobs.jobs or self.late.jobs or self.grams or self.tf):
            self._run(tidx)
            self.fork_side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.fork_side):
                self.on_bucket(0)
            self.forked = True
            self.nbucket += 1

    def flush(self, tidx):
        self._run(tidx)
        if self.forked:
            torch.cuda.current_stream().wait_stream(self.fork_side)
            self.forked = False

    def _run(self, tidx):
        gr, self.grams = sorted(self.grams, key=lambda t: t[0].data_ptr()), []
        while gr:                                   # adjacent (A, dG, dA) triples (both STHCNs of a step) share one launch
            A, dG, dA, N, nsG = gr.pop(0)
            while gr and gr[0][0].data_ptr() == A.data_ptr() + 4 * A.numel() and gr[0][1].data_ptr() == dG.data_ptr() + 4 * dG.numel() \
                    and gr[0][2].data_ptr() == dA.data_ptr() + 4 * dA.numel() and gr[0][3:] == (N, nsG):
                A2, dG2, dA2 = gr.pop(0)[:3]
                A = torch.as_strided(A, (A.shape[0] + A2.shape[0],) + tuple(A.shape[1:]), A.stride())
                dG = torch.as_strided(dG, (dG.shape[0] + dG2.shape[0],) + tuple(dG.shape[1:]), dG.stride())
                dA = torch.as_strided(dA, (dA.shape[0] + dA2.shape[0],) + tuple(dA.shape[1:]), dA.stride())
            # tail roles, level 2: what was queued behind the encoder's first layer (its own reductions; the guide's, where the forward did not
            # carry the KL path) rides with the graph-factor gradients — every producer has been enqueued, and none of these jobs reads dA
            ops.gram_bwd(A, dG, out=dA, layers=A.shape[0] // N, nsplit=nsG, jobs=self.jobs if self.tail else None)
        tf, self.tf = self.tf, []
        if self.tail:                               # level 3: the reductions over dA ride with the time-feature MLPs' backward
            self.jobs.launch()                      # (nothing left, unless the step had no temporal graph)
            ops.timefeat_jobs_bwd(tf, tidx, jobs=self.late)
        else:
            self.jobs.jobs, self.late.jobs = self.jobs.jobs + self.late.jobs, []
            self.jobs.launch()
            ops.timefeat_jobs_bwd(tf, tidx)
        self.tail = False
        self.keep = []


def _zeros(ref, *shape):
    if CTX.ARENA is not None:
        return CTX.ARENA.zeros(*shape)
    return torch.zeros(*shape, device=ref.device)


def _tf_tensors(d, pfx):
    out = []
    for n in TF_NAMES:
        out += [d[pfx + n + ".weight"], d[pfx + n + ".bias"]]
    return out


# ---- time features (GPTST.py:187-219) -----------------------------------------------------------------------------
def _tf_job(p, pfx, tidx, spg=False):
    B, T = tidx.shape[0], tidx.shape[1]
    rows, K = (B, T) if spg else (B * T, 1)
    return ops.TimefeatJob(_tf_tensors(p, pfx), rows, K)


# ---- hyperTem (GPTST.py:154-163) -----------------------------------------------------------------------------------
# Parameter generation (A, G, W_bt, b_bt) and the gradient reductions into the pools / embeddings are batched per STHCN
# (sthcn_fwd / sthcn_bwd below): one launch for all four hyperTem layers instead of one per layer.
# C = 64: the forward may skip writing R = G (*) X and the fused backward rebuild it from X (12 L2-hit float4 per operand).  Measured r03 at the
# bench shape (scratch/mb_ht5.py): forward 22.2 -> 18.8 us, backward 29.4 -> 37.9 us (the weight-gradient workgroups become the long pole: 565 KB
# of L2 reads each) — a net loss of 5 us per layer although it removes 33 MB of HBM traffic, so R is kept.  GPTST_DROP_R=1 switches it on.
DROP_R = os.environ.get("GPTST_DROP_R", "0") == "1"


class HtSaved(NamedTuple):
    """saved state of a hyperTem layer: input x, R = G (*) x (None: not kept), output, temporal graph, generated weights"""
    x: Any
    R: Any
    out: Any
    G: Any
    Wbt: Any


class WgradParts(NamedTuple):
    """weight-gradient partials of a generated layer, what its reductions are queued from: dW (ns * groups, C*C) and db (ns * groups, C), possibly
    column windows of [dW | db] rows; ns row splits"""
    dW: Any
    ns: int
    db: Any


def _ht_fused_bwd(dims):
    """the one-launch hyperTem backward (hypertem_bwd_wgrad) serves this step"""
    return dims[3] == 64 and FUSE_HT_BWD


def hypertem_core_fwd(x, G, Wbt, bbt, dims):
    """x (BTN, C) rows -> out (BTN, C);  G (N,T,T), Wbt (BT,C,C), bbt (BT,C) precomputed."""
    B, T, N, C = dims
    if C == 64:
        keep = not (DROP_R and _ht_fused_bwd(dims) and ops.wgrad_nsplit(MODE_TIME, B * T, N, C) == 1)
        R, out = ops.hypertem_fwd(x.view(B, T, N, C), G, Wbt, bbt, want_R=keep)         # :157-158 + :162-163 fused
        R, out = (R.view(-1, C) if keep else None), out.view(-1, C)
    else:
        R = ops.tmix(x.view(B, T, N, C), G).view(-1, C)                                 # :157-158
        out = ops.apply(R, Wbt, MODE_TIME, B * T, N, bias=bbt, resid=x, epi=EPI_RES_LRELU)  # :162-163
    return out, HtSaved(x, R, out, G, Wbt)


FUSE_HT_BWD = True         # hyperTem backward + its weight gradient in one launch (False: two launches)


def graph_grad_splits(dims):
    """partial graph gradients per layer: the fused C = 64 backward writes one per sample, the unfused path one in total"""
    return dims[0] if dims[3] == 64 else 1


CHAIN128 = os.environ.get("GPTST_CHAIN128", "1") == "1"


def chain_ok(dims):
    """The "dPre chain" (include/gptst_hip.h, gptst_hypertem_bwd): every backward kernel of the layer chain hands its input gradient down
    already multiplied by lrelu'(its input), so that no kernel reads its own output only for the sign.  C = 64: the fused kernels; C = 128
    (r05): the unfused passes in their chain forms (apply128 / wgrad128 without the dPre prologue, gptst_tmix_bwd_chain, epilogue 4) — three
    activation-sized reads less per hyperTem layer, two per cap (BASELINE configs[4])."""
    return _ht_fused_bwd(dims) or (CHAIN128 and dims[3] == 128)


def _wb_parts(dWb, C, ns=1):
    """rows [dW | db] of a weight-gradient launch with ns row splits -> WgradParts of the two column windows"""
    return WgradParts(dWb[:, :C * C], ns, dWb[:, C * C:])


def _wgrad_parts(a, dout, out, mode, dims):
    """the weight-gradient launch of a generated layer on the input a; it also emits the bias gradient (column sums of dPre per group): rows
    [dW | db].  out None: dout already is dPre (chain); else dPre is made from the layer's output in the prologue."""
    B, T, N, C = dims
    dWb, ns = ops.wgrad(a, dout, mode, B * T, N, D2=out, pro=PRO_NONE if out is None else PRO_DPRE, colsum_d=True)
    return _wb_parts(dWb, C, ns)


def _genlin_bwd(dout, out, x, W, mode, dims, chain, premul=False):
    """Backward of a generated linear layer LReLU(x W + b) -> dx, WgradParts.  C = 64: data, weight and bias gradient in one pass; C = 128: the
    dPre chain (neither pass reads the layer's output) or the dPre prologue.  premul (chain only): dx is returned multiplied by lrelu'(x)."""
    B, T, N, C = dims
    BT = B * T
    if C == 64:
        dx, dW, db, ns = ops.apply_wgrad(dout, None if chain else out, x, W, mode, BT, N, premul=chain and premul)
        return dx, WgradParts(dW, ns, db)
    if chain:
        dx = (ops.apply(dout, W, mode, BT, N, transw=True, resid2=x, epi=EPI_PREMUL) if premul
              else ops.apply(dout, W, mode, BT, N, transw=True))
        return dx, _wgrad_parts(x, dout, None, mode, dims)
    dx = ops.apply(dout, W, mode, BT, N, A2=out, transw=True, pro=PRO_DPRE)
    return dx, _wgrad_parts(x, dout, out, mode, dims)


def hypertem_core_bwd(saved, dout, dG_out, dims, chain=False, premul=False):
    """-> dx, WgradParts (dWbt, nsplit, dbias partials); the graph-gradient partials are written into dG_out (nsG, N, T, T).
    chain: dout already is dPre (the layer's output is not read);  premul (chain only): dx is returned multiplied by lrelu'(x)."""
    B, T, N, C = dims
    x, R, out, G, Wbt = saved
    BT = B * T
    v = lambda a: a.view(B, T, N, C)      # noqa: E731
    assert not chain or chain_ok(dims)
    if _ht_fused_bwd(dims):
        # data / graph gradients and the weight + bias gradient side by side in one launch: rows [dW_bt | db_bt]
        dx, dWb, ns, _ = ops.hypertem_bwd_wgrad(v(dout), None if chain else v(out), v(x), G, Wbt, v(R) if R is not None else None, dG=dG_out,
                                                premul=chain and premul)
        return dx.view(-1, C), _wb_parts(dWb, C, ns)
    hp = _wgrad_parts(R, dout, None if chain else out, MODE_TIME, dims)
    if C == 64:
        dx, _, _ = ops.hypertem_bwd(v(dout), v(out), v(x), G, Wbt, dG=dG_out, want_dbias=False)
    elif chain:                                       # C = 128, dPre chain: no pass reads the layer's output
        dR = ops.apply(dout, Wbt, MODE_TIME, BT, N, transw=True)
        dx, _ = ops.tmix_bwd_chain(v(dR), v(x), G, v(dout), premul=premul, dG=dG_out[0])
    else:
        dR = ops.apply(dout, Wbt, MODE_TIME, BT, N, A2=out, transw=True, pro=PRO_DPRE)
        dx, _ = ops.tmix_bwd(v(dR), v(x), G, v(dout), v(out), dG=dG_out[0])
    return dx.view(-1, C), hp


CARRY_RED = os.environ.get("GPTST_CARRY_RED", "1") == "1"        # queued weight-gradient reductions as role workgroups of the routing backward (r05, late)
CARRY_MB = float(os.environ.get("GPTST_CARRY_MB", "25"))        # at most this much of them per launch
CARRY_KL = os.environ.get("GPTST_CARRY_KL", "1") == "1"        # the KL path's backward as guests of the forward's chain launches (KlCarry; 0: after model_bwd)
TAIL_ROLES = os.environ.get("GPTST_TAIL_ROLES", "1") == "1"        # the end of the backward in three launches that carry the reductions (tail_roles_ok; 0: four launches)
PAIR_UNDER_DP = os.environ.get("GPTST_PAIR_UNDER_DP", "1") == "1"    # the decoder-hyperTem1 / encoder-hyperTem4 pair also when the decoder's gradient bucket leaves early (r05)
PAIR_BWD = os.environ.get("GPTST_PAIR_BWD", "1") == "1"        # two adjacent hyperTem layers' backward in one launch (r04)


@contextlib.contextmanager
def no_handoffs():
    """Enqueue (or capture) the step without launches in which one workgroup waits for another (the hyperTem backward pairs, the cross-time role
    of the routing backward, the cooperative mask launch): what a stepper falls back to after a bounded wait expired (step.py::_enter_safe_mode).
    Everything it switches is per thread (CTX, the library's thread-local mask switch) and put back as it was found."""
    from . import _C
    keep = (CTX.NO_HANDOFFS, _C.lib().value("gptst_mask_cooperative_state"))
    CTX.NO_HANDOFFS = True
    _C.lib().call("gptst_mask_cooperative", 0)
    try:
        yield
    finally:
        CTX.NO_HANDOFFS = keep[0]
        _C.lib().call("gptst_mask_cooperative", keep[1])


def pair_bwd_on():
    return PAIR_BWD and not CTX.NO_HANDOFFS


def cross_role():
    return 0 if CTX.NO_HANDOFFS else CROSS_ROLE


TAIL_MAX_WG = 512      # most workgroups of a level's own grid (B*T + 4B, the routing role form's bound) for the tail-role form


def tail_roles_ok(red, dims, sv_e):
    """The end of the backward — the encoder's low-rank first layer, gram_bwd, the reduction launch, the time-feature MLPs: none of them on the
    data-gradient chain — runs as THREE launches, each carrying the reductions whose inputs exist by then as further workgroups (ops.encin_ht1_bwd /
    gram_bwd / timefeat_jobs_bwd jobs=).  Taken where the step is of the kind that carries reductions in its routing backward (cap_core_bwd): not in
    deterministic or safe mode, not under the data-parallel bucket overlap or node shards, C = 64, the low-rank EncIn first layer, and a batch whose
    B*T (b,t) workgroups leave the chip room (the grid bound of gptst_cap_route_roles_ok; its LDS bound is the routing kernel's own and does not
    matter here: N = 207 and N = 24 take this form); a caller asks for it with red.want_tail."""
    B, T, N, C = dims
    return bool(TAIL_ROLES and red.want_tail and CARRY_RED and not red.no_carry and red.on_bucket is None and CTX.NODE_REDUCE is None
                and cross_role() and FUSE_CROSS and CAP_LIN and C == 64 and T == 12 and sv_e is not None and isinstance(sv_e.h1, EncIn)
                and B * T + 4 * B <= TAIL_MAX_WG)


def _ht_pair_shape_ok(dims):
    """the launcher's own shape conditions (gptst_hypertem_bwd_pair, hypertem.hip): T = 12, and rounding a split's rows up to even must not
    change the split count — checked HERE so that a deferred hyperTem1 (PendingH1) is never handed to a launch that would refuse it"""
    B, T, N, C = dims
    if T != 12 or C != 64:
        return False
    ns = ops.wgrad_nsplit(MODE_TIME, B * T, N, C)
    rps = (-(-N // ns) + 1) & ~1
    return -(-N // rps) == ns


def ht_pair_ok(saved1, saved0, dims):
    return (pair_bwd_on() and dims[3] == 64 and not isinstance(saved1, EncIn) and saved1.R is not None and saved0.R is not None
            and _ht_fused_bwd(dims) and _ht_pair_shape_ok(dims))


class PendingH1:
    """the decoder's hyperTem1 backward, deferred into the pair launch with the encoder's hyperTem4 (GPTST.py:271 -> :454): its dPre, saved
    tensors and the output buffers the decoder's reduction jobs already point at"""

    def __init__(self, saved, dd, dG, dWb):
        self.saved, self.dd, self.dG, self.dWb = saved, dd, dG, dWb


def ht_pair_bwd(saved1, saved0, dout, dG1, dG0, dims, dWb1=None):
    """dPre-chain backward of hyperTem layers 1 (upper, dout = its dPre) and 0 in ONE launch -> dx0 (times lrelu'(x0)), hp1, hp0 (as
    hypertem_core_bwd's second result), or None (shape / no saved R)."""
    B, T, N, C = dims
    if not ht_pair_ok(saved1, saved0, dims):
        assert dWb1 is None
        return None
    s1, s0 = saved1, saved0
    v = lambda a: a.view(B, T, N, C)
    r = ops.hypertem_bwd_pair(v(dout), v(s1.x), s1.G, s1.Wbt, v(s1.R), v(s0.x), s0.G, s0.Wbt, v(s0.R), dG1, dG0, _zeros(dout, B), dWb1=dWb1)
    assert r is not None or dWb1 is None
    if r is None:
        return None
    dmid, dx0, dWb1, dWb0, ns = r
    return dx0.view(-1, C), _wb_parts(dWb1, C, ns), _wb_parts(dWb0, C, ns)


# ---- cap (GPTST.py:100-141) ----------------------------------------------------------------------------------------
FUSE_CROSS = os.environ.get("GPTST_FUSE_CROSS", "1") == "1"     # cross-time block folded into its (b,t)-grouped neighbours (r03)
CAP_LIN = os.environ.get("GPTST_CAP_LIN", "1") == "1"           # ... and the entry Linear's backward folded into the same launch (r05)
CROSS_ROLE = int(os.environ.get("GPTST_CROSS_ROLE", "1"))       # ... its backward as a ROLE of the routing backward's launch (r04; 0: replicated prologue —
                                                                # what a stepper falls back to after a lost hand-off.  The rec backward as a THIRD role
                                                                # measured 799 vs 814 steps/s, profiles/r04_roles3_stamps.txt, and left the library in r05)


class CapSaved(NamedTuple):
    """saved state of a cap: input, output, the node scatter's result rec, assignment c (BT,HS,N), cluster rows s, cross-time output v with its
    Ht / Rt, the generated dyn and W_n, and the routing's Y (None: rebuilt in the backward)"""
    x: Any
    out: Any
    rec: Any
    c: Any
    s: Any
    v: Any
    Ht: Any
    Rt: Any
    dyn: Any
    Wn: Any
    Y: Any


class CapParts(NamedTuple):
    """what cap_core_bwd leaves to the caller's batched reductions: the node layer's WgradParts, and the gradients of dyn and of the routing logits"""
    wn: WgradParts
    ddyn: Any
    dlogit: Any


def cap_head_fwd(p, pfx, x, dadj, dyn, dims, num_route, HS, HT):
    """cap up to the cluster -> node scatter (GPTST.py:102-135): x (BTN,C) -> rec (BTN,C), c (BT,HS,N), (s, v, Ht, Rt, Y)."""
    B, T, N, C = dims
    c, s, Y = ops.cap_route_fwd(x.view(B, T, N, C), p[pfx + "ln_p.weight"], p[pfx + "ln_p.bias"], dadj, HS, num_route,
                                reduce_nodes=CTX.NODE_REDUCE, want_Y=True)                                            # :102-123
    fused = ops.cap_cross_rec_fwd(s, dyn, p[pfx + "mask_template"], c, B, T, N, HS, HT) if (FUSE_CROSS and CTX.NODE_REDUCE is None) else None
    if fused is not None:                                                                                             # :125-135, one launch
        v, Ht, Rt, rec = fused
    else:
        v, Ht, Rt = ops.cap_cross_fwd(s, dyn, p[pfx + "mask_template"], B, T, HS, HT)                                 # :125-134
        rec = ops.cap_rec_fwd(c, v, N, C)                                                                             # :135
    return rec, c, (s, v, Ht, Rt, Y)


def cap_core_fwd(p, pfx, x, dadj, dyn, Wn, bn, dims, num_route, HS, HT):
    """x (BTN,C); dadj (BT,HS*N), dyn (B,HT,T*HS), Wn (N,C,C), bn (N,C) precomputed -> out, c (BT,HS,N), saved."""
    B, T, N, C = dims
    rec, c, (s, v, Ht, Rt, Y) = cap_head_fwd(p, pfx, x, dadj, dyn, dims, num_route, HS, HT)
    out = ops.apply(rec, Wn, MODE_NODE, B * T, N, bias=bn, resid=x, epi=EPI_RES_LRELU)                                # :139-141
    return out, c, CapSaved(x, out, rec, c, s, v, Ht, Rt, dyn, Wn, Y)


# Forward chains on the (sample, 16-node) slab (r04, gptst_hypertem_chain_fwd): consecutive hyperTem layers are node-local, so [hyperTem2, hyperTem3]
# and [hyperTem4, the next STHCN's hyperTem1] run as ONE launch each, and the chained layer has no load phase of its own.  GPTST_CHAIN_FWD=0: one
# launch per layer.  (The caps' node layers stay on the node-grouped apply64 — it shares W_n over the 384 (b,t) rows of a node: 12.6 us against
# ~18 us for the per-sample form inside the chain launch, measured in r04 and removed in r05.)
CHAIN_FWD = os.environ.get("GPTST_CHAIN_FWD", "1") == "1"


def chain_fwd_ok(dims):
    return CHAIN_FWD and dims[3] == 64 and not DROP_R      # (node shards too: the chained layers are node-local, r05)


def ht_chain_fwd(x, stages, dims, kl=None):
    """consecutive hyperTem layers in one launch -> [HtSaved per layer], last output.  stages: [(G, Wbt, bbt), ...]
    kl: the step's KlCarry — the launch carries its next KL-path stage as guest workgroups, if one is due"""
    B, T, N, C = dims
    res = ops.hypertem_chain_fwd(x.view(B, T, N, C), stages, guest=kl.guest() if kl is not None else None)
    saved, xin = [], x
    for (G, Wbt, _b), (R, o) in zip(stages, res):
        o = o.view(-1, C)
        saved.append(HtSaved(xin, R.view(-1, C), o, G, Wbt))
        xin = o
    return saved, xin


def cap_core_bwd(p, g, pfx, saved, dout, dims, HS, HT, red, chain=False):
    """-> dx and the pieces whose reductions are batched by the caller: CapParts.
    chain: dout already is dPre, and dx is returned multiplied by lrelu'(x) (x is a hyperTem output)."""
    B, T, N, C = dims
    x, out, rec, c, s, v, Ht, Rt, dyn, Wn, Y = saved
    BT, dev = B * T, x.device
    assert not chain or chain_ok(dims)
    drec, wn = _genlin_bwd(dout, out, rec, Wn, MODE_NODE, dims, chain)      # the node-conditioned layer
    dc1, dv = ops.cap_rec_bwd(drec, c, v, reduce_nodes=CTX.NODE_REDUCE)
    gw, gb = g[pfx + "ln_p.weight"], g[pfx + "ln_p.bias"]
    if FUSE_CROSS and CAP_LIN and C == 64 and CTX.NODE_REDUCE is None and Y is None:
        # r05: cross-time backward (role) + routing backward + the entry Linear's backward and the residual branch in ONE launch; dY never leaves LDS
        # r05: queued reductions of the layers already behind us ride in this launch — where it has the role form (idle slots: B*T + 4B <= 512 workgroups)
        carry = red.take_carry(CARRY_MB) if cross_role() and _C.lib().value("gptst_cap_route_roles_ok", B, T, N, C, HS, HT) == 1 else None
        lin = ops.cap_cross_route_lin_bwd(x.view(B, T, N, C), p[pfx + "ln_p.weight"], p[pfx + "ln_p.bias"], c, dc1, dv, s, Rt, Ht, dyn,
                                          p[pfx + "mask_template"], dout, None if chain else out, chain, B, T, HS, HT,
                                          flags=_zeros(x, 4 * B) if cross_role() else None, jobs=carry)
        red.untake(carry)                                              # (not launched: shape beyond the fused form)
        if lin is not None:
            dx, dWp, dbp, dlogit, ddyn = lin
            red.jobs.bwd_pool(_ones(dev, dWp.shape[0]), dWp, gw.view(1, C * C))      # B*T (+ the node halves' rows, r06) partials
            red.jobs.bwd_pool(_ones(dev, dbp.shape[0]), dbp, gb.view(1, C))
            return dx, CapParts(wn, ddyn, dlogit)
    fused = None
    if FUSE_CROSS and CTX.NODE_REDUCE is None and Y is None:
        fused = ops.cap_cross_route_bwd(x.view(B, T, N, C), p[pfx + "ln_p.weight"], p[pfx + "ln_p.bias"], c, dc1, dv, s, Rt, Ht, dyn,
                                        p[pfx + "mask_template"], B, T, HS, HT, flags=_zeros(x, 4 * B) if cross_role() else None)
    if fused is not None:
        dY, dlogit, ddyn = fused
    else:
        dS, ddyn = ops.cap_cross_bwd(dv, s, Rt, Ht, dyn, p[pfx + "mask_template"], B, T, HS, HT)
        dY, dlogit = ops.cap_route_bwd(x.view(B, T, N, C), p[pfx + "ln_p.weight"], p[pfx + "ln_p.bias"], c, dc1, dS, Y=Y)
    if C == 64:
        # dx = dY Wp + dout*lrelu'(out), the ln_p weight gradient and its bias gradient in one pass over dY
        dx, dWp, dbp, ns2 = ops.linear_bwd(dY, x, p[pfx + "ln_p.weight"], dout, None if chain else out, premul=chain)
        red.jobs.bwd_pool(_ones(dev, ns2), dWp, gw.view(1, C * C))
        red.jobs.bwd_pool(_ones(dev, ns2), dbp, gb.view(1, C))
    else:
        if chain:   # (dY Wp + dPre) * lrelu'(x): the sign comes from the layer's INPUT, which the weight gradient below reads anyway
            dx = ops.apply(dY, p[pfx + "ln_p.weight"], MODE_SHARED, BT, N, resid=dout, resid2=x, epi=EPI_ADD_PREMUL)
        else:
            dx = ops.apply(dY, p[pfx + "ln_p.weight"], MODE_SHARED, BT, N, resid=dout, resid2=out, epi=EPI_ADD_DPRE)
        dWp, ns2 = ops.wgrad(dY, x, MODE_SHARED, BT, N, colsum_a=True)                     # rows [dWp | colsum dY]
        wp = _wb_parts(dWp, C, ns2)
        red.jobs.bwd_pool(_ones(dev, ns2), wp.dW, gw.view(1, C * C))
        red.jobs.bwd_pool(_ones(dev, ns2), wp.db, gb.view(1, C))
    return dx, CapParts(wn, ddyn, dlogit)


_ONES = {}


def _ones(dev, n=1):
    """cached (n, 1) column of ones: the 'embedding' of a plain sum over n partial rows"""
    if (dev, n) not in _ONES:
        _ONES[(dev, n)] = torch.ones(n, 1, device=dev)
    return _ONES[(dev, n)]


# ---- LReLU(x W_g + b_g) with generated weights, no residual (MLP_RL, GPTST.py:24-32) --------------------------------
class CondLinSaved(NamedTuple):
    x: Any
    out: Any
    W: Any


def condlin_fwd(x, Wg, bg, mode, dims):
    B, T, N, C = dims
    out = ops.apply(x, Wg, mode, B * T, N, bias=bg, epi=EPI_LRELU)
    return out, CondLinSaved(x, out, Wg)


def condlin_bwd(saved, dout, emb, wpool, bpool, g_wpool, g_bpool, d_emb, mode, dims, red, chain=False, premul=False, carried=None):
    """chain: dout already is dPre;  premul (chain only): dx is returned multiplied by lrelu'(x).
    carried: (dx, WgradParts) of the fused C = 64 pass already run by an earlier launch (KlCarry): only the reductions are queued."""
    assert not chain or chain_ok(dims)
    dx, w = carried if carried is not None else _genlin_bwd(dout, saved.out, saved.x, saved.W, mode, dims, chain, premul)
    queue_generated(red.jobs, emb, w, wpool, bpool, g_wpool, g_bpool, d_emb)
    return dx


# ---- reductions of a generated layer's gradients into its pools and embeddings -----------------------------------------
def queue_generated(J, emb, parts, wpool, bpool, g_wpool, g_bpool, d_emb):
    """Queue on J (a PoolJobs) the four reductions of a generated layer's WgradParts: pool dW, pool db, then the embedding's gradient from dW
    and from db.  emb (R, K) generated the layer's weights from wpool (K, C, C) and bpool (K, C)."""
    K = emb.shape[1]
    cols = wpool.numel() // K
    dW = parts.dW if parts.dW.dim() == 2 else parts.dW.view(-1, cols)      # (ns*R, C*C), possibly a column window of [dW | db] rows
    J.bwd_pool(emb, dW, g_wpool.view(K, cols), nsplit=parts.ns)
    J.bwd_pool(emb, parts.db, g_bpool, nsplit=parts.ns)
    J.bwd_emb(dW, wpool.view(K, cols), d_emb, nsplit=parts.ns)
    J.bwd_emb(parts.db, bpool, d_emb, nsplit=parts.ns)


def queue_ht(J, p, g, h, hp, time_eb, d_te):
    """the reductions of hyperTem layer h (parameter-name prefix) from its WgradParts hp; d_te: gradient of the time embedding"""
    queue_generated(J, time_eb, hp, p[h + "weights_pool"], p[h + "bias_pool"], g[h + "weights_pool"], g[h + "bias_pool"], d_te)


def queue_cap(J, p, g, c, cp, node, spg, time):
    """the reductions of cap c (parameter-name prefix) from its CapParts cp.  node, spg, time: (embedding, its gradient) of the node layer
    (node_embeddings_spg), of dyn (time_feature2, one row per sample) and of the routing logits (time_feature1_, one row per (b,t))"""
    queue_generated(J, node[0], cp.wn, p[c + "weights_spa"], p[c + "bias_spa"], g[c + "weights_spa"], g[c + "bias_spa"], node[1])
    for (emb, d_emb), name, dy in ((spg, "t_adj", cp.ddyn), (time, "adj", cp.dlogit)):
        R, K = emb.shape
        dy = dy.view(R, -1)
        J.bwd_pool(emb, dy, g[c + name].view(K, -1))
        J.bwd_emb(dy, p[c + name].view(K, -1), d_emb)


# ---- STHCN (GPTST.py:253-273) --------------------------------------------------------------------------------------
ENC, DEC = "encoder.STHCN_encode.", "decoder.STHCN_decode."
GUIDE_TF = "encoder.teb4mask."


def _sthcn_names(pfx):
    return [pfx + "hyperTem%d." % i for i in (1, 2, 3, 4)], [pfx + "cap1.", pfx + "cap2."]


class SthcnGen(NamedTuple):
    """everything generated for one STHCN from the time index and the parameters, and the names / sizes its layers share"""
    emb: Any        # (time_eb, teb, tes): the three time embeddings
    A_all: Any      # (4, N, Hm*T) hyperTem factors, G_all (4, N, T, T) their temporal graphs
    G_all: Any
    Wb: Any         # [(Wbt, bbt)] per hyperTem layer
    Wn: Any         # [(Wn, bn)] per cap
    dadj: Any       # per cap
    dyn: Any        # per cap
    hts: Any        # parameter-name prefixes of the four hyperTem layers, cps: of the two caps
    cps: Any
    d: int
    Hm: int
    ds: int
    HS: int
    HT: int
    slot: Any       # (k, n): the k-th of the n STHCNs generated together (their graph-gradient buffers are adjacent); None: on its own

    def ht(self, i):
        """(G, Wbt, bbt) of hyperTem i+1"""
        return (self.G_all[i],) + self.Wb[i]


class SthcnSaved(NamedTuple):
    """saved state of an STHCN: HtSaved (h1: or EncIn) and CapSaved per layer, and what its backward needs of the SthcnGen"""
    h1: Any
    h2: Any
    h3: Any
    h4: Any
    c1: Any
    c2: Any
    emb: Any
    gen: SthcnGen
    slot: Any


class GenAll(NamedTuple):
    """what gen_all returns"""
    sthcn: Any      # {prefix: SthcnGen}
    guide: Any      # (t4m, Wspa, bspa, Wtem, btem); None: not generated
    pending: Any    # defer: the STHCNs' unlaunched ops.PoolJobs; else None


def _sthcn_gen_jobs(p, pfx, emb, jobs, A_all, dims, G_all, slot=None):
    """Queue the generated-parameter problems of one STHCN (20 jobs, and the 4 temporal graphs); -> SthcnGen (tensors are filled by jobs.launch())."""
    B, T, N, C = dims
    time_eb, teb, tes = emb
    ne, nes = p[pfx + "node_embeddings"], p[pfx + "node_embeddings_spg"]
    hts, cps = _sthcn_names(pfx)
    adj0 = p[hts[0] + "adj"]
    d, Hm = adj0.shape[0], adj0.shape[1]
    cadj, tadj = p[cps[0] + "adj"], p[cps[0] + "t_adj"]
    ds, HS, HT = cadj.shape[0], cadj.shape[1], tadj.shape[1]
    for i, h in enumerate(hts):
        jobs.fwd(ne, p[h + "adj"].view(d, Hm * T), out=A_all[i])                                          # :156
        jobs.gram(ne, p[h + "adj"].view(d, Hm * T), out=G_all[i], A=A_all[i])                             # :156-158 G_n = A_n^T A_n, same launch
    Wb = [(jobs.fwd(time_eb, p[h + "weights_pool"]), jobs.fwd(time_eb, p[h + "bias_pool"])) for h in hts]  # :160-161
    Wn = [(jobs.fwd(nes, p[c + "weights_spa"]), jobs.fwd(nes, p[c + "bias_spa"])) for c in cps]            # :137-138
    dadj = [jobs.fwd(teb, p[c + "adj"].view(ds, HS * N)) for c in cps]                                    # :104
    dyn = [jobs.fwd(tes, p[c + "t_adj"].view(ds, HT * T * HS)).view(B, HT, T * HS) for c in cps]          # :129
    return SthcnGen(emb, A_all, G_all, Wb, Wn, dadj, dyn, hts, cps, d, Hm, ds, HS, HT, slot)


def gen_all(p, tidx, dims, which=(ENC, DEC), guide=True, defer=False):
    """Everything of a step that depends only on the time index and the parameters — the seven time embeddings (:256-261, :337)
    and every generated parameter of both STHCNs and of the guide MLP — in THREE launches (one time-feature job table, one
    poolgen job table, one gram) instead of 23.  -> GenAll
    defer (r05): only the guide's parameters are generated here; the jobs of the STHCNs (parameters and temporal graphs) come back unlaunched as
    its pending (a PoolJobs) — the stepper hands them to the mask generation, whose cooperative launch runs them on the CUs it leaves idle
    (ops.mask_random / mask_adaptive jobs=); nothing before the mask reads their outputs."""
    B, T, N, C = dims
    tfj = []
    for pfx in which:
        tfj += [_tf_job(p, pfx + "time_feature1.", tidx), _tf_job(p, pfx + "time_feature1_.", tidx),
                _tf_job(p, pfx + "time_feature2.", tidx, spg=True)]
    if guide:
        tfj.append(_tf_job(p, GUIDE_TF, tidx))
    embs = ops.timefeat_jobs_fwd(tfj, tidx)
    jobs = ops.PoolJobs()
    now = ops.PoolJobs() if defer else jobs
    sthcn, gd = {}, None
    L = 4 * len(which)
    if guide:
        gj = now
        m = "encoder.MLP_RL."
        t4m = embs[-1]
        gd = (t4m, gj.fwd(p["encoder.neb4mask"], p[m + "weights_pool_spa"]), gj.fwd(p["encoder.neb4mask"], p[m + "bias_pool_spa"]),
              gj.fwd(t4m, p[m + "weights_pool_tem"]), gj.fwd(t4m, p[m + "bias_pool_tem"]))
    if L:
        adj0 = p[which[0] + "hyperTem1.adj"]
        Hm = adj0.shape[1]
        A_all = torch.empty(L, N, Hm * T, device=tidx.device)
        G_all = torch.empty(L, N, T, T, device=tidx.device)
        for k, pfx in enumerate(which):
            sthcn[pfx] = _sthcn_gen_jobs(p, pfx, embs[3 * k:3 * k + 3], jobs, A_all[4 * k:4 * k + 4], dims, G_all[4 * k:4 * k + 4], (k, len(which)))
    now.launch()    # generated parameters AND the temporal graphs: one launch (defer: the guide's alone; a deferred table with a temporal graph beyond
    #                 the job kernel's shapes, jobs.post, later launches on its own)
    return GenAll(sthcn, gd, jobs if defer else None)


def sthcn_fwd(p, pfx, tidx, x, dims, num_route, gen=None, head=None, next_gen=None, kl=None):
    """head: (x after hyperTem1, its saved state) when the previous STHCN's last chain already ran this one's first layer;
    next_gen: SthcnGen of the NEXT STHCN — its hyperTem1 rides on this one's last chain launch where the chain serves the shape;
    -> x, c1, saved, next head (None: nothing rode along).
    kl: the step's KlCarry (the chain launches carry the KL path's backward; the encoder's first cap assignment is its last input)."""
    if gen is None:
        gen = gen_all(p, tidx, dims, which=(pfx,), guide=False).sthcn[pfx]
    ht = gen.ht
    cap = lambda i, x: cap_core_fwd(p, gen.cps[i], x, gen.dadj[i], gen.dyn[i], *gen.Wn[i], dims, num_route, gen.HS, gen.HT)   # noqa: E731
    pairs = chain_fwd_ok(dims)       # hyperTem PAIRS on the slab: [2, 3] and [4, next 1] (the caps' node layers stay on the node-grouped apply64)
    nhead = None
    x, h1 = head if head is not None else hypertem_core_fwd(x, *ht(0), dims)
    x, c1, sc1 = cap(0, x)
    if pairs:
        if kl is not None and kl.c1 is None:
            kl.c1 = c1                                     # (the encoder's: GPTST.py:141, 426)
        (h2, h3), x = ht_chain_fwd(x, [ht(1), ht(2)], dims, kl)
    else:
        x, h2 = hypertem_core_fwd(x, *ht(1), dims)
        x, h3 = hypertem_core_fwd(x, *ht(2), dims)
    x, _, sc2 = cap(1, x)
    if pairs and next_gen is not None:
        (h4, h1n), xn = ht_chain_fwd(x, [ht(3), next_gen.ht(0)], dims, kl)
        x, nhead = h4.out, (xn, h1n)
    else:
        x, h4 = hypertem_core_fwd(x, *ht(3), dims)
    return x, c1, SthcnSaved(h1, h2, h3, h4, sc1, sc2, gen.emb, gen, gen.slot), nhead


def _grad_buffers(red, slot, N, T, HmT, ref, nsG):
    """dG (4, nsG, N,T,T) partial graph gradients and dA (4,N,Hm*T) of one STHCN.  Both STHCNs of a step get adjacent halves of one
    buffer each, so that Reductions.flush() turns their temporal-graph gradients into the factor gradients with ONE gram_bwd launch."""
    if slot is None:
        return torch.empty(4, nsG, N, T, T, device=ref.device), torch.empty(4, N, HmT, device=ref.device)
    k, n = slot
    if red._dG is None or red._dG.shape[0] != 4 * n:
        red._dG = torch.empty(4 * n, nsG, N, T, T, device=ref.device)
        red._dA = torch.empty(4 * n, N, HmT, device=ref.device)
    return red._dG[4 * k:4 * k + 4], red._dA[4 * k:4 * k + 4]


def sthcn_bwd(p, g, pfx, tidx, sv, dout, dims, red, chain=False, premul_in=False, defer_h1=False, after_pending=None):
    """chain: dout already is dPre of the last layer and every layer hands dPre down;  premul_in (chain only): the returned input gradient
    is multiplied by lrelu'(input) — True when the STHCN's input is itself a LeakyReLU output (the decoder's: the encoder embedding).
    defer_h1 (chain, premul_in): hyperTem1's backward is NOT run — a PendingH1 is returned and the STHCN below runs it in the pair launch
    with its own hyperTem4 (dout: that PendingH1)."""
    B, T, N, C = dims
    time_eb, teb, tes = sv.emb
    gn = sv.gen
    A_all, hts, cps, d, Hm, ds, HS, HT = gn.A_all, gn.hts, gn.cps, gn.d, gn.Hm, gn.ds, gn.HS, gn.HT
    ne, nes = p[pfx + "node_embeddings"], p[pfx + "node_embeddings_spg"]
    dne, dnes = g[pfx + "node_embeddings"], g[pfx + "node_embeddings_spg"]
    d_te, d_teb, d_tes = _zeros(time_eb, *time_eb.shape), _zeros(teb, *teb.shape), _zeros(tes, *tes.shape)
    nsG = graph_grad_splits(dims)
    dG_all, dA_all = _grad_buffers(red, sv.slot, N, T, Hm * T, dout, nsG)
    # ---- gradient reductions of the generated parameters: queued as soon as a layer's partials have been launched (r05: the routing backward launches
    # further down the chain carry them as role workgroups, red.take_carry), executed by red.flush() at the latest ----
    J = red.jobs
    e_te, e_node, e_spg, e_teb = (time_eb, d_te), (nes, dnes), (tes, d_tes), (teb, d_teb)

    if isinstance(dout, PendingH1):                 # the STHCN above left its first layer to the pair launch with this one's last layer
        up = dout
        dd, _, hp4 = ht_pair_bwd(up.saved, sv.h4, up.dd, up.dG, dG_all[3], dims, dWb1=up.dWb)
        red.keep.append(up)
        if after_pending is not None:               # the STHCN above is complete only now (data parallel: its gradient bucket closes here)
            after_pending()
    else:
        dd, hp4 = hypertem_core_bwd(sv.h4, dout, dG_all[3], dims, chain, True)
    queue_ht(J, p, g, hts[3], hp4, *e_te)
    dd, cp2 = cap_core_bwd(p, g, cps[1], sv.c2, dd, dims, HS, HT, red, chain)
    queue_cap(J, p, g, cps[1], cp2, e_node, e_spg, e_teb)
    pair = ht_pair_bwd(sv.h3, sv.h2, dd, dG_all[2], dG_all[1], dims) if chain and pair_bwd_on() else None
    if pair is not None:                            # hyperTem3 + hyperTem2: nothing in between (GPTST.py:267-268) -> one launch on the slab
        dd, hp3, hp2 = pair
    else:
        dd, hp3 = hypertem_core_bwd(sv.h3, dd, dG_all[2], dims, chain, True)
        dd, hp2 = hypertem_core_bwd(sv.h2, dd, dG_all[1], dims, chain, True)
    queue_ht(J, p, g, hts[2], hp3, *e_te)
    queue_ht(J, p, g, hts[1], hp2, *e_te)
    dd, cp1 = cap_core_bwd(p, g, cps[0], sv.c1, dd, dims, HS, HT, red, chain)
    queue_cap(J, p, g, cps[0], cp1, e_node, e_spg, e_teb)
    if isinstance(sv.h1, EncIn):                 # the encoder's first layer on the low-rank input form: no input gradient tensor
        assert chain
        e = sv.h1
        w, bi = p["encoder.dim_in_flow.weight"], p["encoder.dim_in_flow.bias"]
        # tail roles, level 1: nothing is on the data-gradient chain behind this launch, and every reduction queued so far reads what earlier
        # launches wrote — they ride here instead of waiting for the reduction launch (what is queued from here on: level 2, Reductions._run)
        carry = red.take_all() if red.tail else None
        if nsG == B:
            dWb, _, dinp = ops.encin_ht1_bwd(dd.view(B, T, N, C), e.source, e.mask, e.fill, w, bi, e.Wbt, e.ab, e.wv, dG=dG_all[0], jobs=carry)
        else:       # (C = 128: the other layers write ONE graph-gradient partial; this kernel writes one per sample)
            dWb, dGb, dinp = ops.encin_ht1_bwd(dd.view(B, T, N, C), e.source, e.mask, e.fill, w, bi, e.Wbt, e.ab, e.wv)
            torch.sum(dGb, 0, out=dG_all[0][0])
        hp1 = _wb_parts(dWb, C)
        wb = _wb_view(g["encoder.dim_in_flow.weight"], g["encoder.dim_in_flow.bias"])
        if wb is not None:
            red.jobs.bwd_pool(_ones(dd.device, dinp.shape[0]), dinp, wb)
        else:
            g["encoder.dim_in_flow.weight"].add_(dinp[:, :C].sum(0).view(C, 1))
            g["encoder.dim_in_flow.bias"].add_(dinp[:, C:].sum(0))
        red.keep.append((dinp, dWb))
        dd = None
    elif defer_h1:
        assert chain and premul_in
        ns = ops.wgrad_nsplit(MODE_TIME, B * T, N, C)
        dWb = torch.empty(ns * B * T, C * C + C, device=dd.device, dtype=torch.float32)
        hp1 = _wb_parts(dWb, C, ns)
        dd = PendingH1(sv.h1, dd, dG_all[0], dWb)
    else:
        dd, hp1 = hypertem_core_bwd(sv.h1, dd, dG_all[0], dims, chain, premul_in)
    queue_ht(J, p, g, hts[0], hp1, *e_te)                      # (a deferred hyperTem1: its partials are written by the pair launch that opens the STHCN below)
    red.gram(A_all.view(4 * N, Hm, T), dG_all, dA_all.view(4 * N, Hm, T), N, nsG)
    for i, h in enumerate(hts):                                  # (dA_all is written by gram_bwd at flush time: the late table)
        red.late.bwd_pool(ne, dA_all[i], g[h + "adj"].view(d, Hm * T))
        red.late.bwd_emb(dA_all[i], p[h + "adj"].view(d, Hm * T), dne)
    red.timefeat(p, g, pfx + "time_feature1.", tidx, d_te)
    red.timefeat(p, g, pfx + "time_feature1_.", tidx, d_teb)
    red.timefeat(p, g, pfx + "time_feature2.", tidx, d_tes, spg=True)
    red.keep.append((sv, hp1, hp2, hp3, hp4, cp1, cp2, dout))
    return dd


# ---- whole model ---------------------------------------------------------------------------------------------------
class EncIn:
    """saved state of the encoder's first layer when it ran on the low-rank input form (ops.encin_ht1_fwd) instead of lin_in + hyperTem"""

    def __init__(self, source, mask, fill, Wbt, ab, wv):
        self.source, self.mask, self.fill, self.Wbt, self.ab, self.wv = source, mask, fill, Wbt, ab, wv


ENCIN = os.environ.get("GPTST_ENCIN", "1") == "1"


def encin_ok(dims, base):
    """input projection + encoder hyperTem1 as one rank-2 kernel pair (encin.hip): base = 1 and the dPre chain in the backward"""
    return ENCIN and base == 1 and dims[3] in (64, 128) and dims[1] == 12 and chain_ok(dims)       # node-local: serves node shards too (r05)


GUIDEIN = os.environ.get("GPTST_GUIDEIN", "1") == "1"
GUIDE_HEAD = os.environ.get("GPTST_GUIDE_HEAD", "1") == "1"     # r06: the classifier's forward as node vectors + ONE (b,t)-grouped pass (gptst_guide_head_fwd)


class LowRankIn(NamedTuple):
    """saved state of the guide's input projection + node layer when they ran on the low-rank form (ops.guide_in_fwd / guide_head_fwd)"""
    Wspa: Any


class GuideSaved(NamedTuple):
    t4m: Any        # the guide's time embedding
    spa: Any        # node-conditioned layer: CondLinSaved, or LowRankIn
    tem: Any        # time-conditioned layer: CondLinSaved
    h2: Any         # its output, the classifier's input
    label: Any      # int32 argmax of the probabilities per row


def guide_fwd(p, source, tidx, dims, base, gen=None, lowrank_in=False):
    """softmax(MLP_RL(raw flow, teb4mask(t), neb4mask)) — GPTST.py:326-332 / 337-343.  -> prob (BTN,HS), GuideSaved.
    lowrank_in (the caller's backward is the dPre chain): input projection + node-conditioned layer as the elementwise low-rank form of
    guidein.hip (base = 1): saved.spa is then a LowRankIn instead of the layer's CondLinSaved."""
    B, T, N, C = dims
    if gen is None:
        gen = gen_all(p, tidx, dims, which=(), guide=True).guide
    t4m, Wspa, bspa, Wtem, btem = gen
    m = "encoder.MLP_RL."
    if lowrank_in and GUIDEIN and GUIDE_HEAD and base == 1 and C == 64:
        # r06: u_n / c_n, then ONE (b,t)-grouped pass for :22-:33, the softmax and the labels (bit-identical to the three launches below)
        r = ops.guide_head_fwd(source, p[m + "ln1.weight"], p[m + "ln1.bias"], Wspa, bspa, Wtem, btem, p[m + "ln3.weight"], p[m + "ln3.bias"])
        if r is not None:
            h1, h2, prob, label = r
            return prob, GuideSaved(t4m, LowRankIn(Wspa), CondLinSaved(h1, h2, Wtem), h2, label)
    if lowrank_in and GUIDEIN and base == 1 and C in (64, 128):
        h1 = ops.guide_in_fwd(source, p[m + "ln1.weight"], p[m + "ln1.bias"], Wspa, bspa)                 # :22 + :24-27, elementwise
        s1 = LowRankIn(Wspa)
    else:
        h0 = ops.lin_in(source, base + 2, base, p[m + "ln1.weight"], p[m + "ln1.bias"], C)                # :22
        h1, s1 = condlin_fwd(h0, Wspa, bspa, MODE_NODE, dims)                                             # :24-27
    h2, s2 = condlin_fwd(h1, Wtem, btem, MODE_TIME, dims)                                                 # :29-32
    prob, label = ops.rowdot(h2, p[m + "ln3.weight"], p[m + "ln3.bias"], softmax=True, want_label=True)   # :33, :332, :344-345
    return prob, GuideSaved(t4m, s1, s2, h2, label)


def _wb_view(gw, gb):
    """[weight | bias] gradient of an nn.Linear as ONE (1, J*C + J) row when the two tensors are adjacent in the flat buffer."""
    n = gw.numel() + gb.numel()
    if gb.data_ptr() != gw.data_ptr() + 4 * gw.numel():
        return None
    return torch.as_strided(gw, (1, n), (n, 1))


def fused_tails_ok(p, C, base, HS):
    """The fused loss heads (tails.hip) serve C in {64, 128} and J, HS <= 16 with [weight | bias] adjacent in the flat buffer."""
    return (C in (64, 128) and base <= ops.TAIL_MAXJ and HS <= ops.TAIL_MAXJ
            and _wb_view(p["decoder.dim_flow_out.weight"], p["decoder.dim_flow_out.bias"]) is not None
            and _wb_view(p["encoder.MLP_RL.ln3.weight"], p["encoder.MLP_RL.ln3.bias"]) is not None)


def loss_tail(p, g, dec, source, mask, base, sigma, mu, thresh, sws, red, chain=False):
    """dim_flow_out + masked MAE + their backward in one pass over dec (GPTST.py:455, Run.py:92-100) -> out (BTN, base), d_dec.
    sws: the step's loss-statistics scratch (ops.tail_sws / arena zeros), folded into stats by ops.stats_fold.
    chain: d_dec is returned multiplied by lrelu'(dec) (the dPre of the decoder's last hyperTem layer)."""
    wo = "decoder.dim_flow_out."
    out, dd, part = ops.tail_mae(dec, p[wo + "weight"], p[wo + "bias"], source, base + 2, mask, sigma, mu, thresh, sws, premul=chain)
    red.jobs.bwd_pool(_ones(dec.device, part.shape[0]), part, _wb_view(g[wo + "weight"], g[wo + "bias"]))
    red.keep.append((part, dd))
    return out, dd


def kl_head(p, g, sv_g, prob, c1, N, w, sws, red, chain=False, carried=None):
    """0.1 KL(eb || prob) and the backward through softmax + MLP_RL.ln3 in one pass over h2 -> d_h2 (guide_bwd(dh2=...));
    chain: multiplied by lrelu'(h2).  carried: (d_h2, part) already computed by an earlier launch (KlCarry): only the reduction is queued."""
    m = "encoder.MLP_RL."
    dh2, part = carried if carried is not None else ops.tail_kl(sv_g.h2, p[m + "ln3.weight"], prob, c1, N, w, sws, premul=chain)
    red.jobs.bwd_pool(_ones(prob.device, part.shape[0]), part, _wb_view(g[m + "ln3.weight"], g[m + "ln3.bias"]))
    red.keep.append((part, dh2))
    return dh2


def _linear_out_bwd(p, g, pfx, h, dy, C, chain, d_h=None):
    """Backward of an output Linear(C -> J) on the LeakyReLU output h (decoder.dim_flow_out, GPTST.py:455; MLP_RL.ln3, :33) from the gradient
    dy (rows, J) of its result: weight / bias gradients into g, -> d_h [+ d_h, a gradient that reaches h directly];  chain: times lrelu'(h),
    i.e. the dPre the layers below expect."""
    J = dy.shape[1]
    dh = ops.lin_in(dy, J, J, p[pfx + "weight"], None, C, wlayout=1)
    ops.rowouter(dy, J, J, h, g[pfx + "weight"], 1, asum=g[pfx + "bias"])
    if d_h is not None:
        dh = dh + d_h
    if chain:
        dh = dh * torch.where(h > 0, 1.0, 0.01)
    return dh


def guide_bwd(p, g, source, tidx, saved, dlogit, dims, base, red, dh2=None, chain=False, carried=None):
    """dlogit (BTN,HS): gradient of the logits — or dh2 (BTN,C) when kl_head already went through ln3 (chain: dh2 is dPre; from dlogit it is
    made so here).
    carried: KlOut — outputs of the time-conditioned layer's and of the low-rank input layers' launches already run by earlier launches (KlCarry)."""
    B, T, N, C = dims
    carried = carried or KlOut()
    t4m, s1, s2, h2 = saved.t4m, saved.spa, saved.tem, saved.h2
    m = "encoder.MLP_RL."
    if dh2 is None:
        dh2 = _linear_out_bwd(p, g, m + "ln3.", h2, dlogit, C, chain)
    d_t4m = _zeros(t4m, *t4m.shape)
    dh1 = condlin_bwd(s2, dh2, t4m, p[m + "weights_pool_tem"], p[m + "bias_pool_tem"], g[m + "weights_pool_tem"],
                      g[m + "bias_pool_tem"], d_t4m, MODE_TIME, dims, red, chain, True, carried=carried.tem)
    if isinstance(s1, LowRankIn):   # node layer + input projection on the low-rank form: p_n, q_n per node instead of dh0 / h0
        assert chain
        neb, wpool, bpool = p["encoder.neb4mask"], p[m + "weights_pool_spa"], p[m + "bias_pool_spa"]
        dWb, dinp = carried.inp if carried.inp is not None else ops.guide_in_bwd(dh1, source, p[m + "ln1.weight"], p[m + "ln1.bias"], s1.Wspa)
        queue_generated(red.jobs, neb, _wb_parts(dWb, C), wpool, bpool, g[m + "weights_pool_spa"], g[m + "bias_pool_spa"], g["encoder.neb4mask"])
        wb = _wb_view(g[m + "ln1.weight"], g[m + "ln1.bias"])
        if wb is not None:
            red.jobs.bwd_pool(_ones(dh1.device, N), dinp, wb)
        else:
            g[m + "ln1.weight"].add_(dinp[:, :C].sum(0).view(C, 1))
            g[m + "ln1.bias"].add_(dinp[:, C:].sum(0))
        red.keep.append((dWb, dinp))
        dh0 = None
    else:
        dh0 = condlin_bwd(s1, dh1, p["encoder.neb4mask"], p[m + "weights_pool_spa"], p[m + "bias_pool_spa"],
                          g[m + "weights_pool_spa"], g[m + "bias_pool_spa"], g["encoder.neb4mask"], MODE_NODE, dims, red, chain, False)
        _in_proj_grads(source, base, dh0, g[m + "ln1.weight"], g[m + "ln1.bias"], None, 0.0, red)
    red.timefeat(p, g, GUIDE_TF, tidx, d_t4m)
    red.keep.append((saved, dlogit, dh2, dh1, dh0))


def kl_carry_ok(dims, HS, sv_g):
    """the guest form serves this step's KL path: the two-layer chain forward, the dPre chain, C = 64, T = 12, the low-rank guide input"""
    B, T, N, C = dims
    return (CARRY_KL and C == 64 and T == 12 and HS <= ops.TAIL_MAXJ and chain_fwd_ok(dims) and chain_ok(dims)
            and sv_g is not None and isinstance(sv_g.spa, LowRankIn))


class KlOut:
    """outputs of the KlCarry stages launched so far, as the stand-alone launches return them (None: not carried)"""

    def __init__(self):
        self.head = None    # (dh2, part): kl_head(carried=)
        self.tem = None     # (dh1, WgradParts) of the time-conditioned layer: condlin_bwd(carried=)
        self.inp = None     # (dWb, dinp) of the low-rank input layers


class KlCarry:
    """The KL term's backward (kl_head + guide_bwd: 0.1 KL + softmax / ln3 -> the time-conditioned layer -> node layer + ln1) run as GUEST
    workgroups of the forward's two-layer hyperTem chain launches, one stage per launch in stage order (gptst_hypertem_chain_fwd_kl).  Its inputs —
    the guide's forward and the encoder's first cap assignment (detached, GPTST.py:141) — exist before the first chain launch, and nothing in the
    STHCNs reads its results, so it only fills slots the one-round chain grids leave idle.  The reductions are queued where the stand-alone launches
    queue them (kl_head / guide_bwd carried=): the gradients' summation order does not change."""

    def __init__(self, p, sv_g, prob, source, dims, w, sws):
        self.p, self.sv_g, self.prob, self.source, self.dims, self.w, self.sws = p, sv_g, prob, source, dims, w, sws
        self.c1 = None              # set by sthcn_fwd once the encoder's first cap has run
        self.stage = 0              # stages launched so far
        self.out = KlOut()

    def guest(self):
        """-> the next stage as ops.hypertem_chain_fwd(guest=...), its outputs allocated; None when none is due (or every stage is out)"""
        if self.c1 is None or self.stage == 3:
            return None
        B, T, N, C = self.dims
        m = "encoder.MLP_RL."
        p, sv_g, dev = self.p, self.sv_g, self.prob.device
        HS = self.prob.shape[1]
        st = self.stage + 1
        f = dict(device=dev, dtype=torch.float32)
        if st == 1:
            h2, W3 = sv_g.h2, p[m + "ln3.weight"]
            dh2 = torch.empty_like(h2)
            part = torch.empty(ops.tail_parts(B * T * N), HS * C + HS, **f)
            self.out.head = (dh2, part)
            ts = [h2, W3, self.prob, self.c1, dh2, part, self.sws]
        elif st == 2:
            h1, Wtem = sv_g.tem.x, sv_g.tem.W
            dh2, _ = self.out.head
            ns = _C.lib().value("gptst_apply_wgrad_nsplit", MODE_TIME, B * T, N)
            dh1, dW, db = torch.empty_like(h1), torch.empty(ns * B * T, C * C, **f), torch.empty(ns * B * T, C, **f)
            self.out.tem = (dh1, WgradParts(dW, ns, db))
            ts = [dh2, h1, Wtem, dh1, dW, db]
        else:
            dh1, _ = self.out.tem
            dWb, dinp = torch.empty(N, C * C + C, **f), torch.empty(N, 2 * C, **f)
            self.out.inp = (dWb, dinp)
            ts = [dh1, self.source, p[m + "ln1.weight"], p[m + "ln1.bias"], sv_g.spa.Wspa, dWb, dinp]
        self.stage = st
        return (st, ts, 0, ops.kl_guest_blocks(st, B, T, N), HS, self.source.shape[-1], self.w)


def _in_proj_grads(source, base, dY, gW, gb, mask, fill, red):
    """Weight / bias gradient of an input projection Linear(base -> C) on the (masked) raw flow (GPTST.py:22, :416-418): gW (C, base) +=
    dY^T a', gb += colsum(dY).  base = 1: the row-chunk partials [gW | gb] fold as ONE job of the step's reduction launch; else the
    two-launch rowouter."""
    wb = _wb_view(gW, gb)
    if base == 1 and wb is not None:
        C = dY.shape[1]
        part = ops.rowouter_part(source, base + 2, base, dY, mask=mask, fill=fill)
        red.jobs.bwd_pool(_ones(dY.device, part.shape[0]), part[:, :2 * C], wb)
        red.keep.append(part)
    else:
        ops.rowouter(source, base + 2, base, dY, gW, 0, csum=gb, mask=mask, fill=fill)


class Forward(NamedTuple):
    """what autoencoder_fwd returns, whichever launches it chose"""
    emb: Any        # (BTN, C) encoder output
    c1: Any         # (BT, HS, N) the encoder's first cap assignment
    dec: Any        # (BTN, C) decoder STHCN output (None: encoder only)
    out: Any        # (BTN, base) reconstruction (None: the head was not asked for)
    sv_e: Any
    sv_d: Any


def autoencoder_fwd(p, source, mask, dims, base, num_route, scaler_zeros, gen=None, tidx=None, lowrank_in=False, kl=None, head=True,
                    decoder=True, join=True):
    """Masked-autoencoder body — GPTST.py:415-421 + 453-456 -> Forward.  mask (BTN*base) fp32, 1 = visible; None -> no masking (eval).
    gen: the step's GenAll (None: generated here).  decoder=False: the encoder alone (fine-tuning's embedding).  head: also
    decoder.dim_flow_out (False: the caller's loss_tail goes through it).
    lowrank_in: the caller's backward is the dPre chain (model_bwd(chain=True)) — the input projection + encoder hyperTem1 then run as the
    rank-2 kernel pair of encin.hip where the shape allows.  kl: the step's KlCarry (sthcn_fwd).
    join: the decoder's first hyperTem layer rides on the encoder's last chain launch where the chain serves the shape (False: callers that
    have always run the two layers as launches of their own)."""
    B, T, N, C = dims
    if tidx is None:
        tidx = source[:, :, 0, base:base + 2].contiguous()
    gen_e, gen_d = (gen.sthcn[ENC], gen.sthcn[DEC] if decoder else None) if gen is not None else (None, None)
    first = None
    if lowrank_in and gen_e is not None and encin_ok(dims, base):
        # input projection + encoder hyperTem1 on the rank-2 structure of the input: no x0, no GEMM (ops.encin_ht1_fwd)
        w, bi = p["encoder.dim_in_flow.weight"], p["encoder.dim_in_flow.bias"]
        G1, Wbt1, bbt1 = gen_e.ht(0)
        o1, ab, wv = ops.encin_ht1_fwd(source, base, mask, 0.0 if mask is None else scaler_zeros, w, bi, G1, Wbt1, bbt1)
        first = (o1.view(-1, C), EncIn(source, mask, 0.0 if mask is None else scaler_zeros, Wbt1, ab, wv))
        x0 = None
    else:
        x0 = ops.lin_in(source, base + 2, base, p["encoder.dim_in_flow.weight"], p["encoder.dim_in_flow.bias"], C,
                        mask=mask, fill=scaler_zeros)                                                      # :416-418
    emb, c1, sv_e, dec_h1 = sthcn_fwd(p, ENC, tidx, x0, dims, num_route, gen=gen_e, head=first, next_gen=gen_d if join else None, kl=kl)   # :421
    if not decoder:
        return Forward(emb, c1, None, None, sv_e, None)
    dec, _, sv_d, _ = sthcn_fwd(p, DEC, tidx, emb, dims, num_route, gen=gen_d, head=dec_h1, kl=kl)         # :454
    out = ops.rowdot(dec, p["decoder.dim_flow_out.weight"], p["decoder.dim_flow_out.bias"]) if head else None   # :455
    return Forward(emb, c1, dec, out, sv_e, sv_d)


def model_bwd(p, g, source, mask, tidx, sv_e, sv_d, dec, d_out, d_dec, dims, base, scaler_zeros, red, dd=None, chain=False):
    """Backward of autoencoder_fwd given d_out (BTN, base) [and optional d_dec (BTN, C)] — or given dd, the gradient
    w.r.t. the decoder STHCN output, when loss_tail already went through dim_flow_out.  Parameter-gradient reductions are queued
    on ``red`` (Reductions): the caller runs red.flush(tidx) once the whole backward is enqueued.
    chain: the dPre chain, see chain_ok() (dd from loss_tail(chain=True), or made from d_out here)."""
    B, T, N, C = dims
    if dd is None:
        dd = _linear_out_bwd(p, g, "decoder.dim_flow_out.", dec, d_out, C, chain, d_h=d_dec)
    # the decoder's hyperTem1 and the encoder's hyperTem4 are adjacent (GPTST.py:271 -> :454): one pair launch, unless the decoder's gradient
    # bucket must be complete when its backward ends (data-parallel overlap / a side stream flush the decoder's reductions right here)
    # r05: also under the data-parallel bucket overlap — the decoder's bucket then closes ONE LAUNCH later, behind the pair launch that finishes its
    # first layer (the bucket's reductions and its forked all-reduce still run under the rest of the encoder's backward)
    defer = (chain and (red.on_bucket is None or PAIR_UNDER_DP) and not isinstance(sv_d.h1, EncIn)
             and ht_pair_ok(sv_d.h1, sv_e.h4, dims))
    late = defer and red.on_bucket is not None
    d_emb = sthcn_bwd(p, g, DEC, tidx, sv_d, dd, dims, red, chain, True, defer_h1=defer)     # the decoder's input is the encoder's last LeakyReLU output
    if not late:
        red.flush_async(tidx)                               # the decoder's reductions overlap with the encoder's backward chain
    d_x0 = sthcn_bwd(p, g, ENC, tidx, sv_e, d_emb, dims, red, chain, False,  # the encoder's input is a plain Linear: no premultiplication
                     after_pending=(lambda: red.flush_async(tidx)) if late else None)
    red.flush_async(tidx)                                   # ... and the encoder's with the guide's
    if d_x0 is not None:                                    # (None: the low-rank first layer produced the input-projection gradient itself)
        _in_proj_grads(source, base, d_x0, g["encoder.dim_in_flow.weight"], g["encoder.dim_in_flow.bias"], mask, scaler_zeros, red)


def encoder_bwd(p, g, source, tidx, sv_e, d_emb, dims, base, red):
    """Backward of autoencoder_fwd(decoder=False, lowrank_in=False, mask=None) given d_emb (BTN, C), the gradient of the encoder's embedding
    (fine-tuning the encoder downstream: model._EncoderFn): the encoder STHCN in the non-chain forms the module path runs, then the input
    projection on the unmasked flow.  The caller runs red.flush(tidx)."""
    d_x0 = sthcn_bwd(p, g, ENC, tidx, sv_e, d_emb, dims, red, chain=False, premul_in=False)
    _in_proj_grads(source, base, d_x0, g["encoder.dim_in_flow.weight"], g["encoder.dim_in_flow.bias"], None, 0.0, red)


def step_bwd(p, g, source, mask, tidx, fw, prob, sv_g, dims, base, scaler_zeros, red, loss, stats, sws=None, with_kl=False, kl=None):
    """The pretraining loss (masked MAE [+ 0.1 KL], Run.py:92-100) and the whole backward behind autoencoder_fwd / guide_fwd, for the steppers.
    loss: (sigma, mu, mape threshold).  sws (the step's per-workgroup loss statistics, zeroed): the FUSED heads — loss_tail and kl_head go
    through dim_flow_out / ln3 with their backward in one pass each (fw.out is not needed), on the dPre chain where chain_ok(dims); the caller
    folds sws into the statistics.  sws None: the loss kernels on fw.out, sums straight into `stats`.  kl: the step's KlCarry, whose stages
    the forward's chain launches already ran."""
    B, T, N, C = dims
    sigma, mu, thresh = loss
    if sws is not None:
        chain = chain_ok(dims)                                                 # dPre chain: no backward kernel re-reads its layer's output
        done = kl.out if kl is not None else KlOut()                           # outputs of the stages the chain launches carried
        _, dd = loss_tail(p, g, fw.dec, source, mask, base, sigma, mu, thresh, sws, red, chain=chain)
        red.tail = chain and tail_roles_ok(red, dims, fw.sv_e)
        # tail roles: the inputs of a carried KL path's reductions have existed since the forward — queued first, they ride at level 1
        kl_first = red.tail and with_kl and None not in (done.head, done.tem, done.inp)
        if kl_first:
            dh2 = kl_head(p, g, sv_g, prob, fw.c1, N, 0.1, sws, red, chain=chain, carried=done.head)
            guide_bwd(p, g, source, tidx, sv_g, None, dims, base, red, dh2=dh2, chain=chain, carried=done)
        model_bwd(p, g, source, mask, tidx, fw.sv_e, fw.sv_d, fw.dec, None, None, dims, base, scaler_zeros, red, dd=dd, chain=chain)
        if with_kl and not kl_first:
            dh2 = kl_head(p, g, sv_g, prob, fw.c1, N, 0.1, sws, red, chain=chain, carried=done.head)
            guide_bwd(p, g, source, tidx, sv_g, None, dims, base, red, dh2=dh2, chain=chain, carried=done)
    else:
        M = B * T * N
        ops.mae_fwd(fw.out, source, base + 2, mask, sigma, mu, thresh, M, base, stats)
        d_out = ops.mae_bwd(fw.out, source, base + 2, mask, sigma, mu, thresh, M, base, stats, normalize=False)
        model_bwd(p, g, source, mask, tidx, fw.sv_e, fw.sv_d, fw.dec, d_out, None, dims, base, scaler_zeros, red)
        if with_kl:
            dlogit = ops.kl(prob, fw.c1, N, 0.1, stats)
            guide_bwd(p, g, source, tidx, sv_g, dlogit, dims, base, red)


def module_bwd(p, g, source, mask, tidx, fw, prob, sv_g, dims, base, scaler_zeros, red, d_out, d_dec=None, d_prob=None, chain=False):
    """The backward behind autoencoder_fwd / guide_fwd when the loss is the caller's (GPTST_Model under autograd): d_out (BTN, base),
    d_dec (BTN, C) and d_prob (BTN, HS) are the gradients of the returned reconstruction, decoder state and guide probabilities (None:
    did not enter the loss).  chain: on the dPre chain (the forward ran with lowrank_in=True)."""
    model_bwd(p, g, source, mask, tidx, fw.sv_e, fw.sv_d, fw.dec, d_out, d_dec, dims, base, scaler_zeros, red, chain=chain)
    if d_prob is not None:      # softmax backward: dlogit = prob * (d_prob - sum(d_prob * prob)), then MLP_RL.ln3 (GPTST.py:33)
        dlogit = (prob * (d_prob - (d_prob * prob).sum(-1, keepdim=True))).contiguous()
        guide_bwd(p, g, source, tidx, sv_g, dlogit, dims, base, red, chain=chain)


def warm_up(fn):
    """Before a graph capture: run fn twice on a side stream (allocator, lazy kernel attributes), then synchronise."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()


_GC_LOCK, _GC_HELD = threading.Lock(), [0, False]      # captures under way (ranks emulated by threads capture side by side), collector was on


@contextlib.contextmanager
def quiet_gc():
    """Around a graph capture: collect Python's dead cycles first, then keep the cyclic collector off until the last capture under way has ended.
    A collection that starts in the middle of a capture runs the destructors of whatever dead cycle it finds — another stepper's CUDAGraph
    objects, tensors of another stream, events — on the capturing thread, and the runtime aborts the process on calls a capture does not allow.
    ``torch.cuda.graph`` collects on entry only under ``torch.compiler.config.force_cudagraph_gc`` and never holds the collector off."""
    with _GC_LOCK:
        if _GC_HELD[0] == 0:
            gc.collect()
            _GC_HELD[1] = gc.isenabled()
            gc.disable()
        _GC_HELD[0] += 1
    try:
        yield
    finally:
        with _GC_LOCK:
            _GC_HELD[0] -= 1
            if _GC_HELD[0] == 0 and _GC_HELD[1]:
                gc.enable()
