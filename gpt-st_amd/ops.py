"""Thin Python wrappers over the C ABI (include/gptst_hip.h): one function per kernel entry point.

All tensors are contiguous fp32 CUDA tensors; calls enqueue on torch's current stream and never synchronise,
so they are hipGraph-capturable.  No CPU path exists here by design.
"""
import contextlib
import ctypes
import math
from typing import Any, NamedTuple

import torch

from . import _C

MODE_TIME, MODE_NODE, MODE_SHARED = 0, 1, 2
PRO_NONE, PRO_DPRE = 0, 1
EPI_PLAIN, EPI_RES_LRELU, EPI_ADD_DPRE, EPI_LRELU, EPI_ADD_PREMUL, EPI_PREMUL = 0, 1, 2, 3, 4, 5

_p = _C.ptr


TIMER = None      # bench.py sets this to a list to collect (name, tag, start_event, end_event, bytes) per launch
LAST_CALL = {}    # (name, tag) -> argument tuple of the most recent timed launch (bench.py replays the dominant kernel)


CALL_LOCK = None  # tests that emulate ranks with threads set a threading.Lock: one C-ABI call (= all launches of one op) at a time


def _call(name, *args, tag="", nbytes=0, entry=None):
    """entry: the C entry point to call when it is not `name` — a form of `name` that carries a job table (jobs= below).  The launch is
    recorded under `name`, the table goes into the tag; LAST_CALL keeps no arguments for it (they are another entry point's)."""
    fn = entry or name
    if CALL_LOCK is not None:
        with CALL_LOCK:
            _C.lib().call(fn, *args, _C.stream())
        return
    if TIMER is None:
        _C.lib().call(fn, *args, _C.stream())
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _C.lib().call(fn, *args, _C.stream())
    e1.record()
    TIMER.append((name, tag, e0, e1, nbytes))
    if entry is None:
        LAST_CALL[(name, tag)] = args


def _nb(*ts):
    """Algorithmic bytes of a launch: every tensor operand read or written once."""
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


def _chk(*ts):
    for t in ts:
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())


# ---- poolgen -------------------------------------------------------------------------------------------------
def poolgen(emb, pool, pool2=None):
    """emb (R,K); pool (K, ...) -> out (R, ...) [and out2 for pool2]."""
    _chk(emb, pool, pool2)
    R, K = emb.shape
    cols = pool.numel() // K
    out = torch.empty((R,) + tuple(pool.shape[1:]), device=emb.device, dtype=torch.float32)
    out2, cols2 = None, 0
    if pool2 is not None:
        cols2 = pool2.numel() // K
        out2 = torch.empty((R,) + tuple(pool2.shape[1:]), device=emb.device, dtype=torch.float32)
    _call("gptst_poolgen_fwd", _p(emb), _p(pool), _p(out), cols, _p(pool2), _p(out2), cols2, R, K, nbytes=_nb(emb, pool, out, pool2, out2))
    return (out, out2) if pool2 is not None else out


def poolgen_bwd_pool(emb, dW, dpool, dW2=None, dpool2=None, nsplit=1):
    """dpool += emb^T dW (summing wgrad splits); dpool2 += emb^T dW2."""
    _chk(emb, dW, dpool, dW2, dpool2)
    R, K = emb.shape
    cols = dpool.numel() // K
    cols2 = dpool2.numel() // K if dpool2 is not None else 0
    _call("gptst_poolgen_bwd_pool", _p(emb), _p(dW), _p(dpool), cols, _p(dW2), _p(dpool2), cols2, R, nsplit, K,
          nbytes=_nb(emb, dW, dpool, dW2, dpool2))


def poolgen_bwd_emb(dW, pool, demb, dW2=None, pool2=None, nsplit=1):
    """demb += dW pool^T (+ dW2 pool2^T)."""
    _chk(dW, pool, demb, dW2, pool2)
    R, K = demb.shape
    cols = pool.numel() // K
    cols2 = pool2.numel() // K if pool2 is not None else 0
    _call("gptst_poolgen_bwd_emb", _p(dW), _p(pool), cols, _p(dW2), _p(pool2), cols2, _p(demb), R, nsplit, K,
          nbytes=_nb(dW, pool, dW2, pool2, demb))


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _ints(vs):
    return (ctypes.c_int * len(vs))(*[int(v) for v in vs])


def poolgen_multi(emb, pools, outs=None):
    """One launch for up to 8 problems sharing emb: outs[p] (R, ...) = emb @ pools[p] (K, ...)."""
    _chk(emb, *pools)
    R, K = emb.shape
    if outs is None:
        outs = [torch.empty((R,) + tuple(pl.shape[1:]), device=emb.device, dtype=torch.float32) for pl in pools]
    cols = [pl.numel() // K for pl in pools]
    _call("gptst_poolgen_fwd_multi", _p(emb), len(pools), _ptrs(pools), _ptrs(outs), _ints(cols), R, K, nbytes=_nb(emb, *pools, *outs))
    return outs


def poolgen_bwd_pool_multi(emb, dWs, dpools, nsplits=None):
    """dpools[p] += emb^T dWs[p] (summing nsplits[p] row blocks of R rows)."""
    _chk(emb, *dWs, *dpools)
    R, K = emb.shape
    cols = [dp.numel() // K for dp in dpools]
    ns = nsplits if nsplits is not None else [1] * len(dWs)
    _call("gptst_poolgen_bwd_pool_multi", _p(emb), len(dWs), _ptrs(dWs), _ptrs(dpools), _ints(cols), _ints(ns), R, K,
          nbytes=_nb(emb, *dWs, *dpools))


def poolgen_bwd_emb_multi(dWs, pools, demb, nsplits=None):
    """demb += sum_p dWs[p] pools[p]^T."""
    _chk(demb, *dWs, *pools)
    R, K = demb.shape
    cols = [pl.numel() // K for pl in pools]
    ns = nsplits if nsplits is not None else [1] * len(dWs)
    _call("gptst_poolgen_bwd_emb_multi", len(dWs), _ptrs(dWs), _ptrs(pools), _ints(cols), _ints(ns), _p(demb), R, K,
          nbytes=_nb(demb, *dWs, *pools))


class PoolJob(NamedTuple):
    """one row of a PoolJobs table: the fields are the columns of the C ABI's job table (gptst_pool_jobs), in its order"""
    kind: int
    emb: Any
    dW: Any
    pool: Any
    out: Any
    R: int
    K: int
    cols: int
    nsplit: int
    ldx: int


class PoolJobs:
    """A list of independent poolgen problems (forward generation and/or gradient reductions, each with its own embedding) that
    run as ONE launch per 112 jobs (gptst_pool_jobs).  Tensors are kept referenced until launch()."""
    FWD, BWD_POOL, BWD_EMB, GRAM = 0, 1, 2, 3

    def __init__(self):
        self.jobs = []
        self.post = []           # (A, G, rows, Hm): temporal graphs built by gptst_gram_fwd behind the launch (shapes beyond the job kernel)

    def fwd(self, emb, pool, out=None):
        """out (R, ...) = emb (R,K) @ pool (K, ...)"""
        _chk(emb, pool, out)
        R, K = emb.shape
        if out is None:
            out = torch.empty((R,) + tuple(pool.shape[1:]), device=emb.device, dtype=torch.float32)
        self.jobs.append(PoolJob(self.FWD, emb, None, pool, out, R, K, pool.numel() // K, 1, 0))
        return out

    def gram(self, emb, pool, out, A=None):
        """out (R,12,12) = A_r^T A_r, A_r = (emb @ pool)[r] viewed (cols/12, 12) — hyperTem's temporal graph (= gram_fwd of the fwd() job's output).
        A: that forward job's output (R, cols) — used when the shape does not fit the job kernel's LDS scratch (more than 20 hyperedges at
        embed_dim 16): the graph is then built by gptst_gram_fwd right behind the job launch."""
        _chk(emb, pool, out, A)
        R, K = emb.shape
        cols = pool.numel() // K
        assert cols % 12 == 0 and out.numel() == R * 144 and out.is_contiguous()
        if _C.lib().value("gptst_pool_jobs_gram_rows", K, cols) <= 0:
            assert A is not None and A.numel() == R * cols, "gram job does not fit and no forward output was given"
            self.post.append((A, out, R, cols // 12))
            return out
        self.jobs.append(PoolJob(self.GRAM, emb, None, pool, out, R, K, cols, 1, 0))
        return out

    @staticmethod
    def _ldx(dW, cols):
        """dW is a (rows, cols) matrix or a column window of a wider row-major one: -> its row stride"""
        assert dW.is_cuda and dW.dtype == torch.float32 and dW.dim() == 2 and dW.shape[1] == cols and dW.stride(1) == 1, (dW.shape, dW.stride(), cols)
        return dW.stride(0)

    def bwd_pool(self, emb, dW, dpool, nsplit=1):
        """dpool (K, ...) += emb^T dW, summing nsplit row blocks of R rows.  (Owned, non-atomic update: one job per dpool.)"""
        _chk(emb, dpool)
        R, K = emb.shape
        cols = dpool.numel() // K
        self.jobs.append(PoolJob(self.BWD_POOL, emb, dW, None, dpool, R, K, cols, nsplit, self._ldx(dW, cols)))

    def bwd_emb(self, dW, pool, demb, nsplit=1):
        """demb (R,K) += (sum of nsplit row blocks of dW) @ pool^T"""
        _chk(pool, demb)
        R, K = demb.shape
        cols = pool.numel() // K
        self.jobs.append(PoolJob(self.BWD_EMB, None, dW, pool, demb, R, K, cols, nsplit, self._ldx(dW, cols)))

    @staticmethod
    def columns(js, fields=PoolJob._fields):
        """-> the ctypes arguments of a job table: the job count, then one array per field of `fields`, in the ABI's column order"""
        return [len(js)] + [(_ptrs0 if f in ("emb", "dW", "pool", "out") else _ints)([getattr(j, f) for j in js])
                            for f in PoolJob._fields if f in fields]

    def take_reductions(self):
        """-> (the ctypes columns of this table, its tag, its bytes, the jobs) for a launch that carries it (jobs= of encin_ht1_bwd / gram_bwd /
        timefeat_jobs_bwd: gradient reductions only), and empties the table.  The caller holds the returned jobs until its call has been enqueued:
        they are the last reference to some operands (a routing backward's dWp / dbp), the columns are raw pointers, and memory freed before the
        enqueue can be handed to another thread's launch that the stream runs first (ranks emulated by threads)."""
        assert not self.post and all(j.kind in (self.BWD_POOL, self.BWD_EMB) for j in self.jobs)
        js, self.jobs = self.jobs, []
        return self.columns(js), "+jobs%d" % len(js), _nb(*[t for j in js for t in (j.emb, j.dW, j.pool, j.out)]), js

    def launch(self):
        js, self.jobs = self.jobs, []
        post, self.post = self.post, []
        if js:
            _call("gptst_pool_jobs", *self.columns(js), nbytes=_nb(*[t for j in js for t in (j.emb, j.dW, j.pool, j.out)]))
        for A, G, rows, Hm in post:                      # temporal graphs whose shape is beyond the job kernel
            _call("gptst_gram_fwd", _p(A), _p(G), rows, Hm)


def _ptrs0(ts):
    return (ctypes.c_void_p * len(ts))(*[(t.data_ptr() if t is not None else None) for t in ts])


# ---- MFMA contractions ---------------------------------------------------------------------------------------
def apply(A, W, mode, BT, N, bias=None, resid=None, A2=None, transw=False, pro=PRO_NONE, epi=EPI_PLAIN, colsum=None,
          out=None, resid2=None):
    """colsum=True -> (out, cs, ns): cs (ns*G, C) holds ns row-split partials of the column sums of pro(A) per group (the bias
    gradient; consumers sum the splits: PoolJobs.bwd_pool / bwd_emb nsplit=ns).  colsum=<tensor (G,C)>: the summed partials are
    added to it (convenience for tests)."""
    _chk(A, W, bias, resid, A2, resid2)
    C = A.shape[-1]
    if out is None:
        out = torch.empty_like(A)
    cs, ns = None, 0
    if colsum is not None:
        G = BT if mode == MODE_TIME else (N if mode == MODE_NODE else 1)
        ns = _C.lib().value("gptst_apply_nsplit", mode, BT, N, C)
        cs = torch.empty(ns * G, C, device=A.device, dtype=torch.float32)
    _call("gptst_apply", _p(A), _p(A2), _p(W), int(W.dim() == 3), int(transw), _p(bias), _p(resid), _p(resid2), _p(out), _p(cs),
          mode, pro, epi, BT, N, C, tag="mode%d pro%d epi%d" % (mode, pro, epi), nbytes=_nb(A, A2, W, bias, resid, resid2, out))
    if colsum is True:
        return out, cs, ns
    if colsum is not None:
        colsum.add_(cs.view(ns, -1, C).sum(0).view_as(colsum))
    return out


def apply_wgrad(dOut, Y, S, W, mode, BT, N, premul=False):
    """Fused backward of a generated-weight layer (C = 64): -> (dS (rows,C), dW (ns*G, C*C), dbias (ns*G, C), ns).
    Y=None: dOut already is dPre;  premul: dS is returned multiplied by lrelu'(S)."""
    _chk(dOut, Y, S, W)
    C = dOut.shape[-1]
    G = BT if mode == MODE_TIME else N
    ns = _C.lib().value("gptst_apply_wgrad_nsplit", mode, BT, N)
    dS = torch.empty_like(dOut)
    dW = torch.empty(ns * G, C * C, device=dOut.device, dtype=torch.float32)
    db = torch.empty(ns * G, C, device=dOut.device, dtype=torch.float32)
    _call("gptst_apply_wgrad", _p(dOut), _p(Y), _p(S), _p(W), _p(dS), _p(dW), _p(db), int(premul), mode, BT, N, C, tag="mode%d" % mode,
          nbytes=_nb(dOut, Y, S, W, dS, dW))
    return dS, dW, db, ns


def linear_bwd(dY, X, Wp, dOut, out, premul=False):
    """Fused backward of cap's entry Linear + the layer's residual branch (C = 64): -> (dX, dWp (ns, C*C), dbp (ns, C), ns).
    out=None: dOut already is dPre;  premul: dX is returned multiplied by lrelu'(X)."""
    _chk(dY, X, Wp, dOut, out)
    rows, C = dY.shape
    ns = _C.lib().value("gptst_linear_bwd_nsplit", rows)
    dX = torch.empty_like(dY)
    dWp = torch.empty(ns, C * C, device=dY.device, dtype=torch.float32)
    dbp = torch.empty(ns, C, device=dY.device, dtype=torch.float32)
    _call("gptst_linear_bwd", _p(dY), _p(X), _p(Wp), _p(dOut), _p(out), _p(dX), _p(dWp), _p(dbp), int(premul), rows, C,
          nbytes=_nb(dY, X, dOut, out, dX, dWp))
    return dX, dWp, dbp, ns


def wgrad_nsplit(mode, BT, N, C=64):
    return _C.lib().value("gptst_wgrad_nsplit", mode, BT, N, C)


def wgrad(A, D, mode, BT, N, D2=None, pro=PRO_NONE, colsum_a=False, colsum_d=False):
    """-> (dW (nsplit*G, C, C), nsplit);  colsum_a / colsum_d: rows become [dW (C*C) | column sums of A / of pro(D) (C)]."""
    _chk(A, D, D2)
    C = A.shape[-1]
    ns = wgrad_nsplit(mode, BT, N, C)
    G = BT if mode == MODE_TIME else (N if mode == MODE_NODE else 1)
    if colsum_a or colsum_d:
        dW = torch.empty(ns * G, C * C + C, device=A.device, dtype=torch.float32)
        _call("gptst_wgrad_colsum", _p(A), _p(D), _p(D2), _p(dW), mode, pro, 1 if colsum_a else 2, BT, N, C,
              tag="mode%d pro%d cs" % (mode, pro), nbytes=_nb(A, D, D2, dW))
    else:
        dW = torch.empty(ns * G, C, C, device=A.device, dtype=torch.float32)
        _call("gptst_wgrad", _p(A), _p(D), _p(D2), _p(dW), mode, pro, BT, N, C, tag="mode%d pro%d" % (mode, pro), nbytes=_nb(A, D, D2, dW))
    return dW, ns


# ---- temporal hypergraph -------------------------------------------------------------------------------------
def gram_fwd(A):
    N, Hm, T = A.shape
    G = torch.empty(N, T, T, device=A.device, dtype=torch.float32)
    _call("gptst_gram_fwd", _p(A), _p(G), N, Hm)
    return G


def gram_bwd(A, dG, out=None, layers=1, nsplit=1, jobs=None):
    """A (L*N,Hm,T); dG (L, nsplit, N, T, T) partial graph gradients (summed in a fixed order) -> dA (L*N,Hm,T).
    jobs: a PoolJobs table of gradient reductions that neither read dA nor write A / dG — launched here, as further workgroups of this launch
    (gptst_gram_bwd_jobs), and emptied."""
    LN, Hm, T = A.shape
    dA = out if out is not None else torch.empty_like(A)
    if jobs is not None and jobs.jobs:
        cols, tag, nb, held = jobs.take_reductions()
        _call("gptst_gram_bwd", _p(A), _p(dG), _p(dA), layers, LN // layers, Hm, nsplit, *cols, tag=tag, nbytes=nb, entry="gptst_gram_bwd_jobs")
        del held
    else:
        _call("gptst_gram_bwd", _p(A), _p(dG), _p(dA), layers, LN // layers, Hm, nsplit)
    return dA


def tmix(X, G, dOut=None, Y=None):
    _chk(X, G, dOut, Y)
    B, T, N, C = X.shape
    out = torch.empty_like(X)
    _call("gptst_tmix", _p(X), _p(G), _p(dOut), _p(Y), _p(out), B, T, N, C, tag="bwd" if dOut is not None else "fwd",
          nbytes=_nb(X, G, dOut, Y, out))
    return out


def hypertem_fwd(X, G, Wbt, bbt, want_R=True):
    """Fused hyperTem forward -> (R, out), both (B,T,N,C); want_R=False -> (None, out): the backward rebuilds R from X."""
    _chk(X, G, Wbt, bbt)
    B, T, N, C = X.shape
    R = torch.empty_like(X) if want_R else None
    out = torch.empty_like(X)
    _call("gptst_hypertem_fwd", _p(X), _p(G), _p(Wbt), _p(bbt), _p(R), _p(out), B, T, N, C, nbytes=_nb(X, G, Wbt, bbt, R, out))
    return R, out


def hypertem_chain_fwd(X, stages, want_R=True, guest=None):
    """Consecutive hyperTem layers in ONE launch on the (sample, 16-node) slab (gptst_hypertem_chain_fwd, C = 64).  X (B,T,N,C): input of the
    first layer;  stages: [(G, Wbt, bbt), ...] (1..3)  ->  [(R or None, out), ...], all (B,T,N,C).
    guest: (stage, operand tensors, v0, v1, HS, lda, w) — virtual blocks [v0, v1) of one KL-path stage ride in the same launch
    (gptst_hypertem_chain_fwd_kl, two layers only; engine.KlCarry)."""
    B, T, N, C = X.shape
    _chk(X, *[t for st in stages for t in st])
    f = lambda: torch.empty(B, T, N, C, device=X.device, dtype=torch.float32)
    Rs = [f() if want_R else None for _ in stages]
    outs = [f() for _ in stages]
    chain = (_p(X), len(stages), _ptrs0([st[0] for st in stages]), _ptrs0([st[1] for st in stages]), _ptrs0([st[2] for st in stages]),
             _ptrs0(Rs), _ptrs0(outs), B, T, N, C)
    if guest is None:
        _call("gptst_hypertem_chain_fwd", *chain, tag="x%d" % len(stages), nbytes=_nb(X, *Rs, *outs))
    else:
        stage, ts, v0, v1, HS, lda, w = guest
        _chk(*ts)
        _call("gptst_hypertem_chain_fwd_kl", *chain, stage, _ptrs0(ts), v0, v1, HS, lda, float(w), tag="x%d+kl%d" % (len(stages), stage),
              nbytes=_nb(X, *Rs, *outs))
    return list(zip(Rs, outs))


def kl_guest_blocks(stage, B, T, N):
    """workgroups of KL-path stage 1..3 at this shape (gptst_kl_guest_blocks)"""
    return _C.lib().value("gptst_kl_guest_blocks", stage, B, T, N)


def encin_ht1_fwd(source, base, mask, fill, w, bi, G, Wbt, bbt):
    """Encoder input projection + hyperTem1 on the rank-2 structure of the input (base = 1) -> out (B,T,N,C), (ab, wv) for the backward."""
    B, T, N, F = source.shape
    C = Wbt.shape[-1]
    assert base == 1
    _chk(source, mask, w, bi, G, Wbt, bbt)
    f = dict(device=source.device, dtype=torch.float32)
    out, ab, wv = torch.empty(B, T, N, C, **f), torch.empty(B * T * N, 2, **f), torch.empty(B * T, 2 * C, **f)
    _call("gptst_encin_ht1_fwd", _p(source), F, _p(mask), float(fill), _p(w), _p(bi), _p(G), _p(Wbt), _p(bbt), _p(out), _p(ab), _p(wv), B, T, N, C,
          nbytes=_nb(Wbt, out))
    return out, ab, wv


def encin_ht1_bwd(dPre, source, mask, fill, w, bi, Wbt, ab, wv, dG=None, jobs=None):
    """-> dWb (B*T, C*C + C) rows [dW_bt | db_bt], dG (B,N,T,T) per-sample partials, dinp (B*T, 2C) partials of d(dim_in_flow.weight | bias).
    jobs: a PoolJobs table of gradient reductions whose inputs earlier launches wrote — launched here, as further workgroups of this launch
    (gptst_encin_ht1_bwd_jobs), and emptied."""
    B, T, N, F = source.shape
    C = Wbt.shape[-1]
    _chk(dPre, source, mask, w, bi, Wbt, ab, wv, dG)
    f = dict(device=source.device, dtype=torch.float32)
    dWb, dinp = torch.empty(B * T, C * C + C, **f), torch.empty(B * T, 2 * C, **f)
    if dG is None:
        dG = torch.empty(B, N, T, T, **f)
    host = (_p(dPre), _p(source), F, _p(mask), float(fill), _p(w), _p(bi), _p(Wbt), _p(ab), _p(wv), _p(dWb), _p(dG), _p(dinp), B, T, N, C)
    if jobs is not None and jobs.jobs:
        cols, tag, nb, held = jobs.take_reductions()
        _call("gptst_encin_ht1_bwd", *host, *cols, tag=tag, nbytes=_nb(dPre, Wbt, dWb, dG) + nb, entry="gptst_encin_ht1_bwd_jobs")
        del held
    else:
        _call("gptst_encin_ht1_bwd", *host, nbytes=_nb(dPre, Wbt, dWb, dG))
    return dWb, dG, dinp


def guide_in_fwd(source, w1, b1, Wn, bn):
    """MLP_RL input projection + node-conditioned layer on the low-rank input form (base = 1) -> h1 (B*T*N, C)."""
    B, T, N, F = source.shape
    C = Wn.shape[-1]
    _chk(source, w1, b1, Wn, bn)
    h1 = torch.empty(B * T * N, C, device=source.device, dtype=torch.float32)
    _call("gptst_guide_in_fwd", _p(source), F, _p(w1), _p(b1), _p(Wn), _p(bn), _p(h1), B * T, N, C, nbytes=_nb(Wn, h1))
    return h1


def guide_head_fwd(source, w1, b1, Wn, bn, Wbt, bbt, W3, b3):
    """MLP_RL's whole forward on the low-rank input form (base = 1, C = 64) in two launches -> h1, h2 (B*T*N, C), prob (B*T*N, J), label int32 —
    or None when the shape needs the three launches (guide_in_fwd, apply, rowdot)."""
    B, T, N, F = source.shape
    C, J = Wn.shape[-1], W3.shape[0]
    if C != 64 or J > 16:
        return None
    _chk(source, w1, b1, Wn, bn, Wbt, bbt, W3, b3)
    dev = source.device
    f = dict(device=dev, dtype=torch.float32)
    uc = torch.empty(N, 2 * C, **f)
    h1, h2 = torch.empty(B * T * N, C, **f), torch.empty(B * T * N, C, **f)
    prob = torch.empty(B * T * N, J, **f)
    label = torch.empty(B * T * N, device=dev, dtype=torch.int32)
    _call("gptst_guide_head_fwd", _p(source), F, _p(w1), _p(b1), _p(Wn), _p(bn), _p(Wbt), _p(bbt), _p(W3), _p(b3), _p(uc), _p(h1), _p(h2), _p(prob),
          _p(label), B * T, N, C, J, nbytes=_nb(Wbt, h1, h2, prob))
    return h1, h2, prob, label


def guide_in_bwd(dPre, source, w1, b1, Wn):
    """-> dWb (N, C*C + C) rows [dW_n | db_n], dinp (N, 2C) partials of d(ln1.weight | ln1.bias)."""
    B, T, N, F = source.shape
    C = Wn.shape[-1]
    _chk(dPre, source, w1, b1, Wn)
    f = dict(device=source.device, dtype=torch.float32)
    dWb, dinp = torch.empty(N, C * C + C, **f), torch.empty(N, 2 * C, **f)
    _call("gptst_guide_in_bwd", _p(dPre), _p(source), F, _p(w1), _p(b1), _p(Wn), _p(dWb), _p(dinp), B * T, N, C, nbytes=_nb(dPre, Wn, dWb))
    return dWb, dinp


def hypertem_ntiles(N):
    return _C.lib().value("gptst_hypertem_ntiles", N)


def hypertem_bwd(dOut, Y, X, G, Wbt, dG=None, want_dbias=True, premul=False):
    """Fused hyperTem backward -> (dX, dbias (ntiles*BT, C) node-tile partials or None, dG (B,N,T,T) per-sample partials); dG may
    be a preallocated (B,N,T,T) buffer.  No atomics: consumers sum the partials (nsplit = ntiles / B).
    Y=None: dOut already is dPre = dOut*lrelu'(out);  premul: dX is returned multiplied by lrelu'(X) (the dPre of the layer below)."""
    _chk(dOut, Y, X, G, Wbt, dG)
    B, T, N, C = X.shape
    dX = torch.empty_like(X)
    nt = hypertem_ntiles(N)
    dbias = torch.empty(nt * B * T, C, device=X.device, dtype=torch.float32) if want_dbias else None
    if dG is None:
        dG = torch.empty(B, N, T, T, device=X.device, dtype=torch.float32)
    _call("gptst_hypertem_bwd", _p(dOut), _p(Y), _p(X), _p(G), _p(Wbt), _p(dX), _p(dbias), _p(dG), int(premul), B, T, N, C,
          nbytes=_nb(dOut, Y, X, G, Wbt, dX))
    return dX, dbias, dG


def hypertem_bwd_wgrad(dOut, Y, X, G, Wbt, R, dG=None, premul=False):
    """Whole backward of a hyperTem layer in ONE launch (C = 64): -> (dX, dWb (ns*BT, C*C+C) rows [dW_bt | db_bt], ns, dG (B,N,T,T)
    per-sample partials) — hypertem_bwd(want_dbias=False) and wgrad(R, dOut, MODE_TIME, D2=Y, pro=PRO_DPRE, colsum_d=True) side by side.
    Y=None / premul: as hypertem_bwd.  R=None: the weight-gradient role rebuilds R from X (one row split only)."""
    _chk(dOut, Y, X, G, Wbt, R, dG)
    B, T, N, C = X.shape
    dX = torch.empty_like(X)
    if dG is None:
        dG = torch.empty(B, N, T, T, device=X.device, dtype=torch.float32)
    ns = wgrad_nsplit(MODE_TIME, B * T, N, C)
    dWb = torch.empty(ns * B * T, C * C + C, device=X.device, dtype=torch.float32)
    _call("gptst_hypertem_bwd_wgrad", _p(dOut), _p(Y), _p(X), _p(G), _p(Wbt), _p(R), _p(dX), _p(dG), _p(dWb), int(premul), B, T, N, C,
          nbytes=_nb(dOut, Y, X, G, Wbt, R, dX, dWb))
    return dX, dWb, ns, dG


def hypertem_bwd_pair(dOut1, X1, G1, Wbt1, R1, X0, G0, Wbt0, R0, dG1, dG0, cnt, dWb1=None):
    """Backward of two consecutive hyperTem layers (1 above 0; dPre chain, both input gradients times lrelu'(input)) in ONE launch ->
    (dXmid, dX0, dWb1, dWb0, ns) or None where the pair form does not serve.  cnt: B ZEROED 32-bit words;  dWb1: optional output buffer
    (ns * B*T, C*C + C) of the upper layer's [dW_bt | db_bt] rows."""
    _chk(dOut1, X1, G1, Wbt1, R1, X0, G0, Wbt0, R0, dG1, dG0, cnt, dWb1)
    B, T, N, C = X1.shape
    if C != 64:
        return None
    dXmid, dX0 = torch.empty_like(X1), torch.empty_like(X0)
    ns = wgrad_nsplit(MODE_TIME, B * T, N, C)
    dWb0 = torch.empty(ns * B * T, C * C + C, device=X1.device, dtype=torch.float32)
    if dWb1 is None:
        dWb1 = torch.empty_like(dWb0)
    assert dWb1.shape == dWb0.shape
    try:
        _call("gptst_hypertem_bwd_pair", _p(dOut1), _p(X1), _p(G1), _p(Wbt1), _p(R1), _p(X0), _p(G0), _p(Wbt0), _p(R0), _p(dXmid), _p(dX0),
              _p(dG1), _p(dG0), _p(dWb1), _p(dWb0), _p(cnt), B, T, N, C, nbytes=_nb(dOut1, X1, R1, X0, R0, dXmid, dX0, dWb0, dWb1))
    except _C.GptstError as e:
        if e.code != _C.ESHAPE:
            raise
        return None
    return dXmid, dX0, dWb1, dWb0, ns


def tmix_bwd(dR, X, G, dOut, Y, dG=None):
    """Backward of the temporal mixing in one pass: -> (dX = dOut*lrelu'(Y) + G (*) dR, dG (N,T,T) = sum_b dR X^T)."""
    _chk(dR, X, G, dOut, Y, dG)
    B, T, N, C = X.shape
    dX = torch.empty_like(X)
    if dG is None:
        dG = torch.empty(N, T, T, device=X.device, dtype=torch.float32)
    _call("gptst_tmix_bwd", _p(dR), _p(X), _p(G), _p(dOut), _p(Y), _p(dX), _p(dG), B, T, N, C, nbytes=_nb(dR, X, dOut, Y, dX))
    return dX, dG


def tmix_bwd_chain(dR, X, G, dPre, premul=False, dG=None):
    """dPre-chain form of tmix_bwd: -> (dX = (dPre + G (*) dR) [* lrelu'(X)], dG); the layer's output is not read."""
    _chk(dR, X, G, dPre, dG)
    B, T, N, C = X.shape
    dX = torch.empty_like(X)
    if dG is None:
        dG = torch.empty(N, T, T, device=X.device, dtype=torch.float32)
    _call("gptst_tmix_bwd_chain", _p(dR), _p(X), _p(G), _p(dPre), int(bool(premul)), _p(dX), _p(dG), B, T, N, C, nbytes=_nb(dR, X, dPre, dX))
    return dX, dG


def tmix_dgraph(dR, X, out=None):
    _chk(dR, X, out)
    B, T, N, C = X.shape
    dG = out if out is not None else torch.empty(N, T, T, device=X.device, dtype=torch.float32)
    _call("gptst_tmix_dgraph", _p(dR), _p(X), _p(dG), B, T, N, C, nbytes=_nb(dR, X, dG))
    return dG


# ---- cap -----------------------------------------------------------------------------------------------------
FORCE_CAP_BIG = False      # tests: take the streaming (capbig) path even when the (b,t) capsule matrix would fit LDS


def cap_fits_lds(N, C, HS):
    return (not FORCE_CAP_BIG) and bool(_C.lib().value("gptst_cap_fits_lds", N, C, HS))


def _lds_or_stream(lds_call, stream_call):
    """Try the one-workgroup-per-(b,t) LDS kernel; when it reports that the shape does not fit (ESHAPE, nothing was launched),
    take the streaming capbig path.  (gptst_cap_fits_lds is a conservative bound over all four cap kernels together.)"""
    if FORCE_CAP_BIG:
        return stream_call()
    try:
        return lds_call()
    except _C.GptstError as e:
        if e.code != _C.ESHAPE:
            raise
        return stream_call()


def _capbig_linear(X, Wp, bp):
    """Y = X Wp^T + bp over all rows (ln_p, GPTST.py:102) on the shared-weight apply kernel."""
    B, T, N, C = X.shape
    return apply(X.reshape(-1, C), Wp, MODE_SHARED, B * T, N, bias=bp, transw=True)


def _capbig_type1(cs, P, S, BT, HS, N, C, reduce_nodes=None):
    _call("gptst_capbig_type1", _p(cs), _p(P), _p(S), BT, HS, N, C)
    if reduce_nodes is not None:            # node-sharded run: the one sum over nodes is completed across ranks here
        reduce_nodes(S)


def _cap_route_fwd_big(X, Wp, bp, dadj, HS, R, reduce_nodes=None):
    B, T, N, C = X.shape
    BT, dev = B * T, X.device
    P = _capbig_linear(X, Wp, bp)
    _call("gptst_capbig_squash_rows", _p(P), BT * N, C)
    f = dict(device=dev, dtype=torch.float32)
    cs, c = torch.empty(BT, HS, N, **f), torch.empty(BT, HS, N, **f)
    S, V0, V, s = (torch.empty(BT, HS, C, **f) for _ in range(4))
    bl = torch.zeros(BT, HS, N, **f)
    _call("gptst_capbig_softmax", None, _p(dadj), _p(cs), BT, HS, N, 0, 1)                  # c0 = softmax_h(dadj)        :105
    _capbig_type1(cs, P, S, BT, HS, N, C, reduce_nodes)
    _call("gptst_capbig_post", _p(S), None, _p(V0), BT * HS, C, 1)                          # v0 = squash(c0 . P)         :105-106
    for r in range(R):                                                                      # routing (no grad)           :113-118
        if r > 0:
            _call("gptst_capbig_type2", _p(V), _p(P), _p(bl), BT, HS, N, C)                 # b += v . P^T
        _call("gptst_capbig_softmax", _p(bl), None, _p(cs), BT, HS, N, 1, 0)
        _capbig_type1(cs, P, S, BT, HS, N, C, reduce_nodes)
        _call("gptst_capbig_post", _p(S), _p(V0), _p(V), BT * HS, C, 2)                     # v = squash(v0 (.) c.P)
    if R > 0:
        _call("gptst_capbig_type2", _p(V), _p(P), _p(bl), BT, HS, N, C)
    _call("gptst_capbig_softmax", _p(bl), _p(dadj), _p(c), BT, HS, N, 1, 1)                 # c = softmax_h(b + dadj)     :120
    _capbig_type1(c, P, S, BT, HS, N, C, reduce_nodes)
    _call("gptst_capbig_post", _p(S), None, _p(s), BT * HS, C, 0)                           # s = c . P                   :123
    return c, s


CAP_FLOW = True            # streaming cap on the fused MFMA passes of capflow.hip (False: first-generation cap_big.hip kernels)


def capflow_ok(HS, C):
    return CAP_FLOW and bool(_C.lib().value("gptst_capflow_supported", HS, C))


def _capflow_post(part, nparts, prow, V0, Vout, mode, BT, HS, C, reduce_nodes):
    """Ordered fold of the node-chunk partials + the cluster-level step; a node-sharded run completes the sums across ranks in between."""
    if reduce_nodes is not None:
        full = torch.empty(BT, prow, C, device=part.device, dtype=torch.float32)
        _call("gptst_capflow_post", _p(part), nparts, prow, None, _p(full), 3, BT, HS, C)
        reduce_nodes(full)
        part, nparts = full, 1
    _call("gptst_capflow_post", _p(part), nparts, prow, _p(V0), _p(Vout), mode, BT, HS, C)


def _cap_route_fwd_flow(X, Wp, bp, dadj, HS, R, reduce_nodes=None):
    """-> c, s, Y (pre-squash capsules, kept for the backward).  One pass over the capsule matrix per routing iteration (capflow.hip)."""
    B, T, N, C = X.shape
    BT, dev = B * T, X.device
    f = dict(device=dev, dtype=torch.float32)
    Y = _capbig_linear(X, Wp, bp)
    P = torch.empty_like(Y)
    npart = _C.lib().value("gptst_capflow_nparts", N)
    part = torch.empty(BT, npart, HS + 1, C, **f)
    c = torch.empty(BT, HS, N, **f)
    V0, V, s = (torch.empty(BT, HS, C, **f) for _ in range(3))
    _call("gptst_capflow_squash", _p(Y), _p(dadj), _p(P), _p(part), BT, HS, N, C)                          # P, c0, [c0 P ; colsum P]   :102-105
    _capflow_post(part, npart, HS + 1, V0, V if R > 0 else None, 0, BT, HS, C, reduce_nodes)               # v0; v of iteration 0        :106,:113-118
    bl = None
    for r in range(1, R):                                                                                  # b += v P^T; cs; v           :113-118
        bl2 = torch.empty(BT, HS, N, **f)
        _call("gptst_capflow_route", _p(P), _p(V), _p(bl), _p(bl2), None, None, None, _p(part), BT, HS, N, C)
        bl = bl2
        _capflow_post(part, npart, HS, V0, V, 1, BT, HS, C, reduce_nodes)
    _call("gptst_capflow_route", _p(P), _p(V) if R > 0 else None, _p(bl), None, _p(dadj), None, _p(c), _p(part), BT, HS, N, C)   # :120-123
    _capflow_post(part, npart, HS, None, s, 2, BT, HS, C, reduce_nodes)
    return c, s, Y


def cap_route_fwd(X, Wp, bp, dadj, HS, R, reduce_nodes=None, want_Y=False):
    """X (B,T,N,C); Wp (C,C) ln_p.weight; dadj (BT, HS*N) logits = teb . adj -> c (BT,HS,N), s (BT,HS,C)
    [, Y (BT*N,C) = X Wp^T + bp when the streaming path computed it, else None]."""
    _chk(X, Wp, bp, dadj)
    B, T, N, C = X.shape

    def stream():
        if capflow_ok(HS, C):
            return _cap_route_fwd_flow(X, Wp, bp, dadj, HS, R, reduce_nodes)
        return _cap_route_fwd_big(X, Wp, bp, dadj, HS, R, reduce_nodes) + (None,)

    def lds():
        c = torch.empty(B * T, HS, N, device=X.device, dtype=torch.float32)
        s = torch.empty(B * T, HS, C, device=X.device, dtype=torch.float32)
        _call("gptst_cap_route_fwd", _p(X), _p(Wp), _p(bp), _p(dadj), _p(c), _p(s), B * T, N, C, HS, R, nbytes=_nb(X, Wp, bp, dadj, c, s))
        return c, s, None
    out = stream() if reduce_nodes is not None else _lds_or_stream(lds, stream)
    return out if want_Y else out[:2]


def cap_cross_fwd(s, dyn, tmpl, B, T, HS, HT):
    _chk(s, dyn, tmpl)
    C = s.shape[-1]
    v = torch.empty_like(s)
    Ht = torch.empty(B, HT, C, device=s.device, dtype=torch.float32)
    Rt = torch.empty_like(s)
    _call("gptst_cap_cross_fwd", _p(s), _p(dyn), _p(tmpl), _p(v), _p(Ht), _p(Rt), B, T, C, HS, HT)
    return v, Ht, Rt


def cap_cross_rec_fwd(s, dyn, tmpl, c, B, T, N, HS, HT):
    """Cross-time block + cluster -> node scatter in one launch -> (v, Ht, Rt, rec) or None when the shape needs the two-launch path."""
    _chk(s, dyn, tmpl, c)
    C = s.shape[-1]
    if C != 64 or FORCE_CAP_BIG:
        return None
    v, Rt = torch.empty_like(s), torch.empty_like(s)
    Ht = torch.empty(B, HT, C, device=s.device, dtype=torch.float32)
    rec = torch.empty(B * T * N, C, device=s.device, dtype=torch.float32)
    try:
        _call("gptst_cap_cross_rec_fwd", _p(s), _p(dyn), _p(tmpl), _p(c), _p(v), _p(Ht), _p(Rt), _p(rec), B, T, N, C, HS, HT,
              nbytes=_nb(s, dyn, c, v, Rt, rec))
    except _C.GptstError as e:
        if e.code != _C.ESHAPE:
            raise
        return None
    return v, Ht, Rt, rec


def cap_cross_bwd(dv, s, Rt, Ht, dyn, tmpl, B, T, HS, HT):
    _chk(dv, s, Rt, Ht, dyn, tmpl)
    C = s.shape[-1]
    dS = torch.empty_like(s)
    ddyn = torch.empty_like(dyn)
    nws = _C.lib().value("gptst_cap_cross_ws_floats", B, T, C, HS, HT)      # 0 while the cluster tokens fit LDS
    ws = torch.empty(nws, device=s.device, dtype=torch.float32) if nws else None
    _call("gptst_cap_cross_bwd", _p(dv), _p(s), _p(Rt), _p(Ht), _p(dyn), _p(tmpl), _p(dS), _p(ddyn), _p(ws), B, T, C, HS, HT)
    return dS, ddyn


def cap_rec_fwd(c, v, N, C):
    _chk(c, v)
    BT, HS = c.shape[0], c.shape[1]
    rec = torch.empty(BT * N, C, device=c.device, dtype=torch.float32)

    def stream():
        if capflow_ok(HS, C):
            return _call("gptst_capflow_rec_fwd", _p(c), _p(v), _p(rec), BT, HS, N, C)
        return _call("gptst_capbig_rec_fwd", _p(c), _p(v), _p(rec), BT, HS, N, C)
    _lds_or_stream(lambda: _call("gptst_cap_rec_fwd", _p(c), _p(v), _p(rec), BT, N, C, HS, nbytes=_nb(c, v, rec)), stream)
    return rec


def cap_rec_bwd(drec, c, v, reduce_nodes=None):
    _chk(drec, c, v)
    BT, HS, N = c.shape
    C = v.shape[-1]
    dc1 = torch.empty_like(c)
    dv = torch.empty_like(v)

    def stream():
        if capflow_ok(HS, C):            # dc1 = drec . v^T and the partials of dv = sum_n c drec in ONE pass over drec
            npart = _C.lib().value("gptst_capflow_nparts", N)
            part = torch.empty(BT, npart, HS, C, device=c.device, dtype=torch.float32)
            _call("gptst_capflow_route", _p(drec), _p(v), None, _p(dc1), None, _p(c), None, _p(part), BT, HS, N, C)
            _capflow_post(part, npart, HS, None, dv, 2, BT, HS, C, reduce_nodes)
            return
        _call("gptst_capbig_rec_bwd_dc", _p(drec), _p(v), _p(dc1), BT, HS, N, C)
        _capbig_type1(c, drec, dv, BT, HS, N, C, reduce_nodes)                       # dv = sum_n c drec: a sum over nodes
    if reduce_nodes is not None or (HS > 16 and capflow_ok(HS, C)):     # HS > 16: the LDS kernel is the VALU first generation (172 vs 64 us at HS = 40)
        stream()
    else:
        _lds_or_stream(lambda: _call("gptst_cap_rec_bwd", _p(drec), _p(c), _p(v), _p(dc1), _p(dv), BT, N, C, HS, nbytes=_nb(drec, c, v, dc1, dv)),
                       stream)
    return dc1, dv


def cap_route_bwd(X, Wp, bp, c, dc1, dS, Y=None):
    """Y: the pre-squash capsules X Wp^T + bp when the forward kept them (streaming path); recomputed otherwise."""
    _chk(X, Wp, bp, c, dc1, dS)
    B, T, N, C = X.shape
    HS = c.shape[1]
    dY = torch.empty(B * T * N, C, device=X.device, dtype=torch.float32)
    dlogit = torch.empty_like(c)

    def stream():
        Yv = Y if Y is not None else _capbig_linear(X, Wp, bp)
        name = "gptst_capflow_route_bwd" if capflow_ok(HS, C) else "gptst_capbig_route_bwd_rows"
        _call(name, _p(Yv), _p(c), _p(dc1), _p(dS), _p(dY), _p(dlogit), B * T, HS, N, C)
    if Y is not None:
        stream()
    else:
        _lds_or_stream(lambda: _call("gptst_cap_route_bwd", _p(X), _p(Wp), _p(bp), _p(c), _p(dc1), _p(dS), _p(dY), _p(dlogit), B * T, N, C, HS,
                                     nbytes=_nb(X, Wp, bp, c, dc1, dS, dY, dlogit)), stream)
    return dY, dlogit


def cap_cross_route_bwd(X, Wp, bp, c, dc1, dv, s, Rt, Ht, dyn, tmpl, B, T, HS, HT, flags=None):
    """Cross-time backward + routing backward in one launch -> (dY, dlogit, ddyn) or None when the shape needs the two-launch path.
    flags: 4 B ZEROED 32-bit words (a float32 tensor of zeros will do) — the cross-time backward then runs as a role of the launch (once per
    sample, overlapped with the routing workgroups' capsule GEMM) instead of a prologue repeated by every (b,t) workgroup."""
    _chk(X, Wp, bp, c, dc1, dv, s, Rt, Ht, dyn, tmpl)
    N, C = X.shape[2], X.shape[3]
    if C != 64 or FORCE_CAP_BIG:
        return None
    dY = torch.empty(B * T * N, C, device=X.device, dtype=torch.float32)
    dlogit = torch.empty_like(c)
    ddyn = torch.empty_like(dyn)
    try:
        dS_ws = torch.empty(B * T, HS, C, device=X.device, dtype=torch.float32) if flags is not None else None
        _call("gptst_cap_cross_route_bwd", _p(X), _p(Wp), _p(bp), _p(c), _p(dc1), _p(dv), _p(s), _p(Rt), _p(Ht), _p(dyn), _p(tmpl), _p(dY),
              _p(dlogit), _p(ddyn), _p(dS_ws), _p(flags), B, T, N, C, HS, HT, nbytes=_nb(X, Wp, bp, c, dc1, dv, s, Rt, dY, dlogit))
    except _C.GptstError as e:
        if e.code != _C.ESHAPE:
            raise
        return None
    return dY, dlogit, ddyn


def cap_cross_route_lin_bwd(X, Wp, bp, c, dc1, dv, s, Rt, Ht, dyn, tmpl, dPre, out, premul, B, T, HS, HT, flags=None, jobs=None, nsplit=None):
    """cap_cross_route_bwd + linear_bwd in one launch (r05) -> (dX (B*T*N, C), dWp (rows, C*C), dbp (rows, C), dlogit, ddyn), or None when the shape
    needs the separate launches.  dPre: the cap layer's output gradient (already dPre when out is None; premul: dX times lrelu'(X)).
    rows = B*T + nsplit partial rows (r06: the last nsplit (b,t) run as two node halves with a partial row each; None = what the device's kernels want,
    gptst_cap_split_units).
    jobs: a PoolJobs table of gradient reductions (bwd_pool / bwd_emb) whose inputs are complete — launched here, as role workgroups of this launch where
    that form serves (gptst_cap_cross_route_lin_bwd_jobs); left untouched when None is returned."""
    _chk(X, Wp, bp, c, dc1, dv, s, Rt, Ht, dyn, tmpl, dPre, out)
    N, C = X.shape[2], X.shape[3]
    if C != 64 or FORCE_CAP_BIG:
        return None
    dev = X.device
    if nsplit is None:
        nsplit = _C.lib().value("gptst_cap_split_units", B * T, N, C, HS)
    rows = B * T + nsplit
    dX = torch.empty(B * T * N, C, device=dev, dtype=torch.float32)
    dWp = torch.empty(rows, C * C, device=dev, dtype=torch.float32)
    dbp = torch.empty(rows, C, device=dev, dtype=torch.float32)
    dlogit = torch.empty_like(c)
    ddyn = torch.empty_like(dyn)
    try:
        dS_ws = torch.empty(B * T, HS, C, device=dev, dtype=torch.float32) if flags is not None else None
        js = jobs.jobs if jobs is not None and not jobs.post and all(j.kind in (PoolJobs.BWD_POOL, PoolJobs.BWD_EMB) for j in jobs.jobs) else []
        _call("gptst_cap_cross_route_lin_bwd_split", _p(X), _p(Wp), _p(bp), _p(c), _p(dc1), _p(dv), _p(s), _p(Rt), _p(Ht), _p(dyn), _p(tmpl),
              _p(dPre), _p(out), int(bool(premul)), _p(dX), _p(dWp), _p(dbp), _p(dlogit), _p(ddyn), _p(dS_ws), _p(flags), B, T, N, C, HS, HT, nsplit,
              *PoolJobs.columns(js), nbytes=_nb(X, Wp, bp, c, dc1, dv, s, Rt, dPre, out, dX, dWp, dlogit))
        if js:
            jobs.jobs = []
    except _C.GptstError as e:
        if e.code != _C.ESHAPE:
            raise
        return None
    return dX, dWp, dbp, dlogit, ddyn


# ---- mask generation (integer path) -----------------------------------------------------------------------------
_MASK_WS = {}


def _mask_ws(dev):
    """Persistent scratch for the radix-select histograms (stream-ordered reuse; allocated once per device)."""
    if dev not in _MASK_WS:
        _MASK_WS[dev] = torch.zeros(_C.lib().value("gptst_mask_ws_bytes") // 4, dtype=torch.int32, device=dev)
    return _MASK_WS[dev]


def mask_ws_floats():
    """size (in 4-byte words) of the scratch of mask_random / mask_adaptive: pass a ZEROED fp32 tensor of this size as `ws` to save the
    zeroing launch (PretrainStep takes it from the step's zero-initialised arena)."""
    return _C.lib().value("gptst_mask_ws_bytes") // 4


def _fused_jobs(jobs, u24):
    """-> the column lists of a PoolJobs table that may ride in the mask launch (gptst_mask_u24_fwd_jobs: forward and temporal-graph jobs), or None after launching
    it on its own"""
    if jobs is None or not (jobs.jobs or jobs.post):
        return None
    if not u24 or jobs.post or any(j.kind not in (PoolJobs.FWD, PoolJobs.GRAM) for j in jobs.jobs):
        jobs.launch()
        return None
    odd = [j for j in jobs.jobs if j.kind == PoolJobs.FWD and j.cols % 4]        # scalar-column forward jobs (HS * N = 2070 at METR_LA): a small launch of
    if odd:                                                                      # their own, so that the rest still rides in the mask launch
        rest = [j for j in jobs.jobs if not (j.kind == PoolJobs.FWD and j.cols % 4)]
        jobs.jobs = odd
        jobs.launch()
        jobs.jobs = rest
        if not rest:
            return None
    js, jobs.jobs = jobs.jobs, []
    return js, PoolJobs.columns(js, ("kind", "emb", "pool", "out", "R", "K", "cols"))


def mask_random(noise, k, ws=None, u24=False, jobs=None):
    """u24: every noise value is k * 2^-24 (Philox / torch.rand) — the select runs on the integers with two digit passes instead of three
    (checked on the device: NaN mask otherwise).  jobs: a PoolJobs table of forward jobs, independent of the mask, launched here — inside the mask's
    launch when that is the cooperative one (r05)."""
    _chk(noise)
    mask = torch.empty_like(noise)
    fj = _fused_jobs(jobs, u24)
    if fj is not None:
        _call("gptst_mask_u24_fwd_jobs", 0, None, None, None, None, _p(noise), None, 0, noise.numel(), 0, 1, int(k), None, None, _p(mask),
              _p(ws if ws is not None else _mask_ws(noise.device)), int(ws is not None), *fj[1])
        return mask
    _call("gptst_mask_random_u24" if u24 else "gptst_mask_random", _p(noise), noise.numel(), int(k), _p(mask),
          _p(ws if ws is not None else _mask_ws(noise.device)), int(ws is not None))
    return mask


MASK_SMALL = 1 << 13      # cells up to which the whole mask generation is one single-workgroup launch (masksel.hip MSS_MAXM)


def mask_labels(prob):
    """prob (rows, HS) -> label int32 (rows), counts int32 (HS)."""
    _chk(prob)
    rows, HS = prob.shape
    label = torch.empty(rows, device=prob.device, dtype=torch.int32)
    counts = torch.empty(HS, device=prob.device, dtype=torch.int32)
    _call("gptst_mask_labels", _p(prob), rows, HS, _p(label), _p(counts))
    return label, counts


def mask_adaptive(label, counts, list_c, nums, noise_a, noise_r, ada_all, base, ws=None, u24=False, jobs=None):
    """-> (m_ada (M), m_rnd (M), mask (M*base)) fp32 {0,1}.  ws: see mask_ws_floats().  u24: lattice noise, jobs: see mask_random."""
    M, HS = label.numel(), list_c.numel()
    m_ada = torch.empty(M, device=label.device, dtype=torch.float32)
    m_rnd = torch.empty_like(m_ada)
    mask = torch.empty(M * base, device=label.device, dtype=torch.float32)
    fj = _fused_jobs(jobs, u24)
    if fj is not None:
        _call("gptst_mask_u24_fwd_jobs", 1, _p(label), _p(counts), _p(list_c), _p(nums), _p(noise_a), _p(noise_r), int(ada_all), M, HS, base, 0,
              _p(m_ada), _p(m_rnd), _p(mask), _p(ws if ws is not None else _mask_ws(label.device)), int(ws is not None), *fj[1])
        return m_ada, m_rnd, mask
    _call("gptst_mask_adaptive_u24" if u24 else "gptst_mask_adaptive", _p(label), _p(counts), _p(list_c), _p(nums), _p(noise_a), _p(noise_r),
          int(ada_all), M, HS, base, _p(m_ada), _p(m_rnd), _p(mask), _p(ws if ws is not None else _mask_ws(label.device)), int(ws is not None))
    return m_ada, m_rnd, mask


# ---- thin projections -------------------------------------------------------------------------------------------
def lin_in(a, lda, J, W, b, C, mask=None, fill=0.0, wlayout=0, rows=None):
    rows = rows if rows is not None else a.numel() // lda
    Y = torch.empty(rows, C, device=a.device, dtype=torch.float32)
    _call("gptst_lin_in", _p(a), lda, _p(mask), float(fill), _p(W), wlayout, _p(b), _p(Y), rows, J, C, nbytes=_nb(a, mask, W, b, Y))
    return Y


def rowdot(X, W, b, softmax=False, want_label=False):
    """Z = X W^T + b [softmax over the J outputs]; want_label -> (Z, int32 argmax per row: first maximum)."""
    rows, C = X.shape
    J = W.shape[0]
    Z = torch.empty(rows, J, device=X.device, dtype=torch.float32)
    label = torch.empty(rows, device=X.device, dtype=torch.int32) if want_label else None
    _call("gptst_rowdot", _p(X), _p(W), _p(b), _p(Z), rows, J, C, int(softmax), _p(label), nbytes=_nb(X, W, b, Z))
    return (Z, label) if want_label else Z


def rowouter(a, lda, J, X, out, olayout, csum=None, asum=None, mask=None, fill=0.0):
    rows, C = X.shape
    ws = torch.empty(_C.lib().value("gptst_rowouter_ws_floats", J, C), device=X.device, dtype=torch.float32)
    _call("gptst_rowouter", _p(a), lda, _p(mask), float(fill), _p(X), _p(out), olayout, _p(csum), _p(asum), _p(ws), rows, J, C,
          nbytes=_nb(a, mask, X, out))


def rowouter_part(a, lda, J, X, mask=None, fill=0.0, want_asum=False):
    """First stage of rowouter -> part (nparts, J*C + C + J): [sum a'^T X (j,c) | column sums of X | sums of a'] per row chunk."""
    rows, C = X.shape
    nparts = _C.lib().value("gptst_rowouter_nparts", rows)
    part = torch.empty(nparts, J * C + C + J, device=X.device, dtype=torch.float32)
    _call("gptst_rowouter_part", _p(a), lda, _p(mask), float(fill), _p(X), _p(part), int(want_asum), rows, J, C, nbytes=_nb(X))
    return part


# ---- time features ----------------------------------------------------------------------------------------------
def timefeat_fwd(params, tidx, rows, K):
    """params: the 10 nn.Linear tensors in module order; tidx (B,T,2) contiguous."""
    E = params[1].numel()
    out = torch.empty(rows, E, device=tidx.device, dtype=torch.float32)
    _call("gptst_timefeat_fwd", *[_p(t) for t in params], _p(tidx), _p(out), rows, K, E)
    return out


def timefeat_bwd(params, grads, tidx, dout, rows, K):
    E = params[1].numel()
    _call("gptst_timefeat_bwd", *[_p(t) for t in params], *[_p(t) for t in grads], _p(tidx), _p(dout), rows, K, E)


class TimefeatJob(NamedTuple):
    """one time-feature MLP of a job table: params (its 10 nn.Linear tensors) on rows x K time indices; the backward also has grads and dout"""
    params: Any
    rows: int
    K: int
    grads: Any = None
    dout: Any = None

    @property
    def E(self):
        return self.params[1].numel()


def timefeat_jobs_fwd(jobs, tidx):
    """jobs: [TimefeatJob] -> list of outputs (rows, E); ONE launch."""
    outs = [torch.empty(j.rows, j.E, device=tidx.device, dtype=torch.float32) for j in jobs]
    _call("gptst_timefeat_jobs", len(jobs), 0, _ptrs([t for j in jobs for t in j.params]), None, _p(tidx), _ptrs(outs),
          _ints([j.rows for j in jobs]), _ints([j.K for j in jobs]), _ints([j.E for j in jobs]))
    return outs


def timefeat_jobs_bwd(tf, tidx, jobs=None):
    """tf: [TimefeatJob with grads and dout]; gradients are accumulated; ONE launch.
    jobs: a PoolJobs table of gradient reductions whose inputs earlier launches wrote and which do not touch the time features' tensors —
    launched here, as further workgroups of this launch (gptst_timefeat_jobs_bwd_jobs), and emptied."""
    if not tf:
        if jobs is not None:
            jobs.launch()
        return
    a = (_ptrs([t for j in tf for t in j.params]), _ptrs([t for j in tf for t in j.grads]), _p(tidx),
         _ptrs([j.dout for j in tf]), _ints([j.rows for j in tf]), _ints([j.K for j in tf]), _ints([j.E for j in tf]))
    if jobs is not None and jobs.jobs:
        cols, tag, nb, held = jobs.take_reductions()
        _call("gptst_timefeat_jobs", len(tf), *a, *cols, tag=tag, nbytes=nb, entry="gptst_timefeat_jobs_bwd_jobs")
        del held
    else:
        _call("gptst_timefeat_jobs", len(tf), 1, *a)


# ---- loss / optimiser -------------------------------------------------------------------------------------------
def mae_fwd(out, src, lda, mask, sigma, mu, thresh, rows, J, stats):
    _call("gptst_mae_fwd", _p(out), _p(src), lda, _p(mask), float(sigma), float(mu), float(thresh), rows, J, _p(stats))


def mae_bwd(out, src, lda, mask, sigma, mu, thresh, rows, J, stats, normalize=True):
    dOut = torch.empty_like(out)
    _call("gptst_mae_bwd", _p(out), _p(src), lda, _p(mask), float(sigma), float(mu), float(thresh), rows, J, _p(stats), int(normalize),
          _p(dOut))
    return dOut


def kl(prob, c, N, w, stats, want_grad=True):
    rows, HS = prob.shape
    dlogit = torch.empty_like(prob) if want_grad else None
    _call("gptst_kl", _p(prob), _p(c), rows, N, HS, float(w), _p(dlogit), _p(stats))
    return dlogit


TAIL_MAXJ = 16


def set_deterministic(on):
    """Bit-reproducible steps: the reductions that end in float atomics by default (embedding gradients of the pool jobs, time-feature
    weight gradients) run as single-owner kernels with a fixed summation order.  Thread-local in the library."""
    _C.lib().call("gptst_set_deterministic", int(bool(on)))


@contextlib.contextmanager
def deterministic():
    """the launches enqueued inside run in the fixed-order mode on THIS thread (autograd runs a backward node on a thread of its own, which
    does not see the caller's set_deterministic); the thread's setting is put back afterwards"""
    keep = _C.lib().value("gptst_deterministic_state")
    set_deterministic(True)
    try:
        yield
    finally:
        set_deterministic(keep)


def tail_parts(rows):
    return _C.lib().value("gptst_tail_parts", rows)


def tail_sws(rows, device):
    """zeroed per-workgroup loss-statistics scratch (nparts, 4) shared by tail_mae / tail_kl of one step -> stats_fold"""
    return torch.zeros(_C.lib().value("gptst_tail_parts", rows), 4, device=device, dtype=torch.float32)


def tail_mae(dec, W, b, src, lda, mask, sigma, mu, thresh, sws, premul=False):
    """Fused output head + masked-MAE + its backward (tails.hip) -> out (rows,J), d_dec (rows,C) [gradient of the SUM loss],
    part (nparts, J*C+J) partials of (gW, gb); the workgroups' (sum |y-p|, kept count) go to sws[:, 0:2] (see stats_fold)."""
    rows, C = dec.shape
    J = W.shape[0]
    nparts = _C.lib().value("gptst_tail_parts", rows)
    out = torch.empty(rows, J, device=dec.device, dtype=torch.float32)
    d_dec = torch.empty_like(dec)
    part = torch.empty(nparts, J * C + J, device=dec.device, dtype=torch.float32)
    _call("gptst_tail_mae", _p(dec), _p(W), _p(b), _p(src), lda, _p(mask), float(sigma), float(mu), float(thresh), _p(out), _p(d_dec),
          _p(part), _p(sws), int(premul), rows, J, C, nbytes=_nb(dec, d_dec))
    return out, d_dec, part


def tail_kl(h2, W3, prob, c, N, w, sws, premul=False):
    """Fused KL + softmax/ln3 backward (tails.hip) -> d_h2 (rows,C), part (nparts, HS*C+HS) partials of (gW3, gb3); KL sums -> sws[:, 2]."""
    rows, C = h2.shape
    HS = W3.shape[0]
    nparts = _C.lib().value("gptst_tail_parts", rows)
    d_h2 = torch.empty_like(h2)
    part = torch.empty(nparts, HS * C + HS, device=h2.device, dtype=torch.float32)
    _call("gptst_tail_kl", _p(h2), _p(W3), _p(prob), _p(c), float(w), _p(d_h2), _p(part), _p(sws), int(premul), rows, N, HS, C, nbytes=_nb(h2, d_h2))
    return d_h2, part


def stats_fold(sws, stats):
    """stats[0..2] += column sums of sws in a fixed order"""
    _call("gptst_stats_fold", _p(sws), sws.shape[0], _p(stats))


_ADAM_WS = {}


def step_begin(z0, z1, src, base, noise=None, rng=None):
    """Zero z0 (and z1, may be None), gather the time index of node 0 -> tidx (B,T,2), and (noise given) fill `noise` with uniform [0,1)
    numbers from Philox4x32-10 keyed by the int32 device words rng = [seed, step counter].  One launch."""
    B, T, N, lda = src.shape
    tidx = torch.empty(B, T, 2, device=src.device, dtype=torch.float32)
    _call("gptst_step_begin", _p(z0), z0.numel(), _p(z1), z1.numel() if z1 is not None else 0, _p(src), _p(tidx), B * T, N, lda, base,
          _p(noise), noise.numel() if noise is not None else 0, _p(rng))
    return tidx


class PinnedRing:
    """Per-step host scalars on their way into a device buffer: a ring of pinned records, each guarded by an event recorded behind its H2D copy.
    Steppers never synchronise, so with a single pinned record the host could rewrite the scalars of step k+j (Adam bias corrections, class
    order) before the DMA of step k has read them."""

    def __init__(self, words, rows=None, slots=4, dtype=torch.int32):
        """records of `words` elements, or of (rows, words)"""
        self._host = [torch.zeros((words,) if rows is None else (rows, words), dtype=dtype).pin_memory() for _ in range(slots)]
        self._np = [h.numpy() for h in self._host]             # written without a torch dispatch per element
        self._ev = [None] * slots
        self._i = -1

    def next(self):
        """-> the next record (numpy); waits, host side, until the copy that last used it has run"""
        self._i = (self._i + 1) % len(self._host)
        if self._ev[self._i] is not None:
            self._ev[self._i].synchronize()
        return self._np[self._i]

    def send(self, dev):
        """the record next() handed out -> the device buffer (asynchronous)"""
        dev.copy_(self._host[self._i], non_blocking=True)
        if self._ev[self._i] is None:
            self._ev[self._i] = torch.cuda.Event()
        self._ev[self._i].record()


def adam_scalars(lr, tA, tB, b1, b2, eps, clip, kl, sum_loss):
    """hyper[0..12] of gptst_clip_adam for optimiser step tA of the reconstruction path and tB of the KL path (0: never stepped).  kl: this step
    carries the KL path; sum_loss: the gradient is that of the SUM loss, the optimiser divides path A by the kept-cell count."""
    return (lr / (1 - b1 ** tA), math.sqrt(1 - b2 ** tA), lr / (1 - b1 ** tB) if tB else 0.0, math.sqrt(1 - b2 ** tB) if tB else 1.0,
            b1, b2, eps, clip, 1.0 if kl else 0.0, 1.0 if sum_loss else 0.0, 1.0,
            1 - b1, 1 - b2)          # as the host rounds them (torch passes python's 1 - beta): 1.f - 0.999f is 1.3e-5 low


def clip_adam(p, g, m, v, nA, nB, hyper, stats, ws=None, stats_out=None, sws=None):
    """clip_grad_norm_ + Adam over the flat buffers; stats[3] (in): extra squared-norm terms — with hyper[13] != 0 the total
    squared norm itself, taken as given (node shards) —, stats[4] (out): total squared norm.
    ws: gptst_clip_adam_ws_floats() floats of scratch (default: one cached buffer per device — stream-ordered reuse).
    sws: the step's per-workgroup loss statistics (tail_sws): folded into stats[0..2] by the first launch instead of a separate stats_fold."""
    if ws is None:
        if p.device not in _ADAM_WS:
            _ADAM_WS[p.device] = torch.empty(_C.lib().value("gptst_clip_adam_ws_floats"), device=p.device, dtype=torch.float32)
        ws = _ADAM_WS[p.device]
    _call("gptst_clip_adam", _p(p), _p(g), _p(m), _p(v), int(nA), int(nB), _p(hyper), _p(stats), _p(ws), _p(stats_out), _p(sws),
          sws.shape[0] if sws is not None else 0)


# ---- evaluation metrics (Trainer.test) ---------------------------------------------------------------------------------
def metrics_new(T, N, device):
    return torch.zeros(T, 5, device=device, dtype=torch.float64), torch.zeros(T, N, 6, device=device, dtype=torch.float64)


def metrics_accum(out, src, lda, vis, sigma, mu, mae_thresh, mape_thresh, B, T, N, D, sums_t, sums_tn):
    """Add one batch to the metric sums: out (B*T*N, D), src (B,T,N,lda) normalised input (label = first D channels), vis fp32 mask or None."""
    _call("gptst_metrics_accum", _p(out), _p(src), lda, _p(vis), float(sigma), float(mu), int(mae_thresh is not None),
          float(mae_thresh if mae_thresh is not None else 0.0), float(mape_thresh), B, T, N, D, _p(sums_t), _p(sums_tn))


def metrics_report(sums_t, sums_tn):
    """-> (T+1, 4) float64 rows [mae, rmse, mape, corr]: one per horizon, then the average over all horizons
    (BasicTrainer.py:241-248; CORR per lib/metrics.py:52-77: per node over (batch, [time,] channel), unbiased std, nodes with
    constant truth skipped, mean over nodes)."""
    st, sn = sums_t.cpu(), sums_tn.cpu()

    def rows_of(a, m):
        mae, rmse, mape = a[..., 1] / a[..., 0], torch.sqrt(a[..., 2] / a[..., 0]), a[..., 4] / a[..., 3]
        K, sp, sy, spp, syy, spy = (m[..., k] for k in range(6))
        pm, ym = sp / K, sy / K
        cov = spy / K - pm * ym
        pvar, yvar = (spp - K * pm * pm) / (K - 1), (syy - K * ym * ym) / (K - 1)
        c = cov / torch.sqrt(pvar.clamp_min(0) * yvar.clamp_min(0))
        ok = yvar > 1e-9 * (syy / K).clamp_min(1e-30)                     # true_std != 0
        corr = torch.stack([c[i][ok[i]].mean() for i in range(c.shape[0])]) if c.dim() == 2 else c[ok].mean()
        return torch.stack([mae, rmse, mape, corr], -1)

    per_t = rows_of(st, sn)
    avg = rows_of(st.sum(0), sn.sum(0))
    return torch.cat([per_t, avg[None]], 0)


# ---- the downstream STGCN predictor (csrc/stgcn.hip) -------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_GLU = 0, 1, 2, 3


def _dts(taps):
    assert 1 <= len(taps) <= 4
    return tuple(int(t) for t in taps) + (0,) * (4 - len(taps))


def stgcn_tapgemm(X, W, bias, taps, act, T, N, res=None, res_w=0, keep=False):
    """Y (rows, co) = act(sum_j X[row + taps[j] N] W_j + bias + res[:, :res_w]); W (co | 2 co (GLU), len(taps) * ci), tap-major columns.
    keep (GLU): -> (Y, S = sigmoid(Q), A = P + bias + res), what the backward needs."""
    _chk(X, W, bias, res)
    rows, ci = X.shape
    co = W.shape[0] // 2 if act == ACT_GLU else W.shape[0]
    assert W.shape[1] == len(taps) * ci
    Y = torch.empty(rows, co, device=X.device, dtype=torch.float32)
    S, A = (torch.empty_like(Y), torch.empty_like(Y)) if keep else (None, None)
    _call("gptst_stgcn_tapgemm", _p(X), ci, ci, len(taps), *_dts(taps), _p(W), _p(bias), _p(res), res.shape[1] if res is not None else 0, res_w,
          _p(Y), co, _p(S), _p(A), act, rows, T, N, tag="ci%d co%d k%d act%d" % (ci, co, len(taps), act), nbytes=_nb(X, W, Y, S, A))
    return (Y, S, A) if keep else Y


def stgcn_gate_bwd(dOut, act, out=None, S=None, A=None):
    """dPre (rows, co | 2 co (GLU)) of a tap GEMM's epilogue from dOut and the kept tensors"""
    _chk(dOut, out, S, A)
    rows, co = dOut.shape
    dPre = torch.empty(rows, 2 * co if act == ACT_GLU else co, device=dOut.device, dtype=torch.float32)
    _call("gptst_stgcn_gate_bwd", _p(dOut), _p(out), _p(S), _p(A), _p(dPre), act, rows, co, tag="act%d co%d" % (act, co), nbytes=_nb(dOut, out, S, A, dPre))
    return dPre


def stgcn_wgrad(D, X, taps, T, N, want_bias=True):
    """-> (dW (cw, len(taps) * ci) = D^T X_shift, db (cw) = column sums of D): row-split partials summed in a fixed order"""
    _chk(D, X)
    rows, cw = D.shape
    ci = X.shape[1]
    K = len(taps) * ci
    ns = _C.lib().value("gptst_stgcn_wgrad_nsplit", rows, cw, K)
    part = torch.empty(ns, cw, K, device=D.device, dtype=torch.float32)
    bpart = torch.empty(ns, cw, device=D.device, dtype=torch.float32) if want_bias else None
    _call("gptst_stgcn_wgrad", _p(D), cw, _p(X), ci, ci, len(taps), *_dts(taps), _p(part), _p(bpart), ns, rows, T, N,
          tag="cw%d ci%d k%d" % (cw, ci, len(taps)), nbytes=_nb(D, X, part))
    return part.sum(0), (bpart.sum(0) if want_bias else None)


def stgcn_nodemix(Lp, In, N, c, reduce, res=None):
    """Lp (ks, Np, Np) zero-padded; reduce False: In (rows, c) -> (rows, ks c) = [L_k In]_k;  True: In (rows, ks c) -> (rows, c) = sum_k L_k In_k + res"""
    _chk(Lp, In, res)
    ks, Np = Lp.shape[0], Lp.shape[1]
    rows = In.shape[0]
    assert In.shape[1] == (ks * c if reduce else c) and rows % N == 0
    Out = torch.empty(rows, c if reduce else ks * c, device=In.device, dtype=torch.float32)
    _call("gptst_stgcn_nodemix", _p(Lp), Np, ks, _p(In), _p(Out), _p(res), c, int(reduce), rows // N, N, tag="c%d r%d" % (c, int(reduce)),
          nbytes=_nb(In, Out, res))
    return Out


def stgcn_ln_fwd(X, gamma, beta, units, eps, keep=True):
    """LayerNorm over each unit's M = X.numel() / units values -> (Y, mean, rstd) (mean, rstd None when not kept)"""
    _chk(X, gamma, beta)
    M = X.numel() // units
    Y = torch.empty_like(X)
    mean, rstd = (torch.empty(units, device=X.device, dtype=torch.float32) for _ in range(2)) if keep else (None, None)
    _call("gptst_stgcn_ln_fwd", _p(X), _p(gamma), _p(beta), _p(Y), _p(mean), _p(rstd), units, M, float(eps), tag="M%d" % M, nbytes=_nb(X, Y))
    return Y, mean, rstd


def stgcn_ln_bwd(dY, X, gamma, mean, rstd, units):
    """-> dX of the LayerNorm over each unit"""
    _chk(dY, X, gamma, mean, rstd)
    M = X.numel() // units
    dX = torch.empty_like(X)
    _call("gptst_stgcn_ln_bwd", _p(dY), _p(X), _p(gamma), _p(mean), _p(rstd), _p(dX), units, M, tag="M%d" % M, nbytes=_nb(dY, X, dX))
    return dX


def stgcn_ln_bwd_param(dY, X, mean, rstd, units):
    """-> (dgamma, dbeta) (M values each), summed over the units in a fixed order"""
    _chk(dY, X, mean, rstd)
    M = X.numel() // units
    ns = _C.lib().value("gptst_stgcn_ln_nsplit", units)
    pg, pb = (torch.empty(ns, M, device=X.device, dtype=torch.float32) for _ in range(2))
    _call("gptst_stgcn_ln_bwd_param", _p(dY), _p(X), _p(mean), _p(rstd), _p(pg), _p(pb), ns, units, M, tag="M%d" % M, nbytes=_nb(dY, X))
    return pg.sum(0), pb.sum(0)


# ---- the downstream TGCN predictor's recurrence (csrc/tgcn.hip) ---------------------------------------------------------------------
# step tensors are (B*N, Hp), seq tensors (B*T*N, width) with row (b T + t) N + n; outputs are the caller's buffers (the loop reuses them)
def _tg_nb(Lp, W, step, k):
    """algorithmic bytes of a step launch: the graph, the weights, and k step-sized (B*N, Hp) blocks read or written"""
    return _nb(Lp, W) + k * step.numel() * 4


def tgcn_fwd_gates(Lp, W0h, h, Gx0, t, u, q, B, T, N, r=None, z=None, zoff=0, tiles=0):
    """[r, u] = sigmoid((L h) W0h^T + Gx0[:, t]) -> u, q = r h, and when given r and z[(b, t) rows, zoff:zoff + Hp] = L h"""
    _chk(Lp, W0h, h, Gx0, u, q, r, z)
    Hp = h.shape[1]
    assert W0h.shape == (2 * Hp, Hp) and h.shape[0] == B * N and Gx0.shape == (B * T * N, 2 * Hp) and u.shape == q.shape == h.shape
    _call("gptst_tgcn_fwd_gates", _p(Lp), Lp.shape[0], _p(W0h), _p(h), _p(Gx0), _p(u), _p(r), _p(q), _p(z), z.shape[1] if z is not None else 0, zoff,
          B, T, N, Hp, t, tiles, tag="Hp%d" % Hp, nbytes=_tg_nb(Lp, W0h, h, 5 + (r is not None) + (z is not None)))      # h, Gx0 (2), u, q


def tgcn_fwd_state(Lp, W1h, q, Gx1, t, u, h, h_out, B, T, N, c=None, z=None, zoff=0, tiles=0):
    """c = tanh((L q) W1h^T + Gx1[:, t]) -> h_out = u h + (1 - u) c, and when given c and z[(b, t) rows, zoff:zoff + Hp] = L q"""
    _chk(Lp, W1h, q, Gx1, u, h, h_out, c, z)
    Hp = h.shape[1]
    assert W1h.shape == (Hp, Hp) and h.shape[0] == B * N and Gx1.shape == (B * T * N, Hp) and u.shape == q.shape == h_out.shape == h.shape
    _call("gptst_tgcn_fwd_state", _p(Lp), Lp.shape[0], _p(W1h), _p(q), _p(Gx1), _p(u), _p(h), _p(h_out), _p(c), _p(z),
          z.shape[1] if z is not None else 0, zoff, B, T, N, Hp, t, tiles, tag="Hp%d" % Hp,
          nbytes=_tg_nb(Lp, W1h, h, 5 + (c is not None) + (z is not None)))      # q, Gx1, u, h, h_out


def tgcn_bwd_cand(LpT, W1hT, dh, u, c, r, h, t, dpre1, dpre0, dh_part, B, T, N, tiles=0):
    """dpre1[:, t] = dh (1 - u)(1 - c^2);  dq = (L^T dpre1) W1h;  dpre0[:, t] = [dq h r (1 - r) | dh (h - c) u (1 - u)];  dh_part = dh u + dq r"""
    _chk(LpT, W1hT, dh, u, c, r, h, dpre1, dpre0, dh_part)
    Hp = h.shape[1]
    assert W1hT.shape == (Hp, Hp) and h.shape[0] == B * N and dpre1.shape == (B * T * N, Hp) and dpre0.shape == (B * T * N, 2 * Hp)
    assert dh.shape == u.shape == c.shape == r.shape == dh_part.shape == h.shape
    _call("gptst_tgcn_bwd_cand", _p(LpT), LpT.shape[0], _p(W1hT), _p(dh), _p(u), _p(c), _p(r), _p(h), _p(dpre1), _p(dpre0), _p(dh_part),
          B, T, N, Hp, t, tiles, tag="Hp%d" % Hp, nbytes=_tg_nb(LpT, W1hT, h, 9))      # dh, u, c, r, h; dpre1, dpre0 (2), dh_part


def tgcn_bwd_state(LpT, W0hT, dpre0, dh_part, t, dh_out, B, T, N, tiles=0):
    """dh_out = dh_part + (L^T dpre0[:, t]) W0h"""
    _chk(LpT, W0hT, dpre0, dh_part, dh_out)
    Hp = dh_part.shape[1]
    assert W0hT.shape == (Hp, 2 * Hp) and dh_part.shape[0] == B * N and dpre0.shape == (B * T * N, 2 * Hp) and dh_out.shape == dh_part.shape
    _call("gptst_tgcn_bwd_state", _p(LpT), LpT.shape[0], _p(W0hT), _p(dpre0), _p(dh_part), _p(dh_out), B, T, N, Hp, t, tiles, tag="Hp%d" % Hp,
          nbytes=_tg_nb(LpT, W0hT, dh_part, 4))      # dpre0 (2), dh_part, dh_out


# ---- the downstream CCRNN predictor's graph-GRU cell (csrc/ccrnn.hip) ------------------------------------------------------------------------
# P (ks, Np, Np) the polynomial stack; step tensors (B*N, width), seq tensors (B*T*N, width) as for TGCN; Cp = the width of the cell's input
# inside the slab (0: the input half is hoisted into g)
def _cc_g(g, NO):
    """(Gx, bias) of a launch: g is the hoisted seq tensor (2-D) or the bias vector (1-D)"""
    assert g.shape[-1] == NO
    return (g, None) if g.dim() == 2 else (None, g)


def ccrnn_fwd_gates(P, W0, h, g, t, u, q, B, T, N, inp=None, fb=None, inp_out=None, r=None, z=None, tiles=0):
    """[r, u] = sigmoid([z | P_j z]_j W0^T + g), z = [h | inp] -> u, q = r h, and when given r and z (seq, W0.shape[1]).  fb = (h_top, W, b):
    inp = h_top W^T + b formed on load and stored in inp_out"""
    Hp = h.shape[1]
    Gx, bias = _cc_g(g, 2 * Hp)
    fh, fW, fbias = fb if fb is not None else (None, None, None)
    Cp = inp.shape[1] if inp is not None else (fW.shape[0] if fb is not None else 0)
    _chk(P, W0, h, g, u, q, r, z, inp, fh, fW, fbias, inp_out)
    assert W0.shape == (2 * Hp, (P.shape[0] + 1) * (Hp + Cp)) and h.shape[0] == B * N and u.shape == q.shape == h.shape
    assert (Gx is None or Gx.shape[0] == B * T * N) and (z is None or z.shape == (B * T * N, W0.shape[1]))
    assert fb is None or (fh.shape == h.shape and fW.shape == (Cp, Hp) and fbias.shape == (Cp,) and inp_out.shape == (B * N, Cp))
    assert inp is None or inp.shape == (B * N, Cp)
    _call("gptst_ccrnn_fwd_gates", _p(P), P.shape[1], P.shape[0], _p(W0), _p(h), _p(inp), Cp, _p(fh), _p(fW), _p(fbias), _p(inp_out), _p(Gx), _p(bias),
          _p(u), _p(r), _p(q), _p(z), B, T, N, Hp, t, tiles, tag="Hp%d Cp%d k%d" % (Hp, Cp, P.shape[0]),
          nbytes=_tg_nb(P, W0, h, 5 + (r is not None)) + (z.shape[1] * B * N * 4 if z is not None else 0))


def ccrnn_fwd_state(P, W1, q, g, t, u, h, h_out, B, T, N, inp=None, c=None, z=None, tiles=0):
    """c = tanh([z | P_j z]_j W1^T + g), z = [q | inp] -> h_out = u h + (1 - u) c, and when given c and z"""
    Hp = h.shape[1]
    Gx, bias = _cc_g(g, Hp)
    Cp = inp.shape[1] if inp is not None else 0
    _chk(P, W1, q, g, u, h, h_out, c, z, inp)
    assert W1.shape == (Hp, (P.shape[0] + 1) * (Hp + Cp)) and h.shape[0] == B * N and u.shape == q.shape == h_out.shape == h.shape
    assert (Gx is None or Gx.shape[0] == B * T * N) and (z is None or z.shape == (B * T * N, W1.shape[1])) and (inp is None or inp.shape[0] == B * N)
    _call("gptst_ccrnn_fwd_state", _p(P), P.shape[1], P.shape[0], _p(W1), _p(q), _p(inp), Cp, _p(Gx), _p(bias), _p(u), _p(h), _p(h_out), _p(c), _p(z),
          B, T, N, Hp, t, tiles, tag="Hp%d Cp%d k%d" % (Hp, Cp, P.shape[0]),
          nbytes=_tg_nb(P, W1, h, 5 + (c is not None)) + (z.shape[1] * B * N * 4 if z is not None else 0))


def ccrnn_bwd_cand(PT, W1T, dh, u, c, r, h, t, dpre1, dpre0, dh_part, B, T, N, dh2=None, dinp=None, tiles=0):
    """dpre1[:, t] = (dh + dh2)(1 - u)(1 - c^2);  [dq | dinp] = [dpre1 | P_j^T dpre1]_j W1T^T;  dpre0[:, t] = [dq h r (1 - r) | (dh + dh2)(h - c) u (1 - u)];
    dh_part = (dh + dh2) u + dq r"""
    _chk(PT, W1T, dh, dh2, u, c, r, h, dpre1, dpre0, dh_part, dinp)
    Hp = h.shape[1]
    Cp = dinp.shape[1] if dinp is not None else 0
    assert W1T.shape == (Hp + Cp, (PT.shape[0] + 1) * Hp) and h.shape[0] == B * N and dpre1.shape == (B * T * N, Hp) and dpre0.shape == (B * T * N, 2 * Hp)
    assert dh.shape == u.shape == c.shape == r.shape == dh_part.shape == h.shape and (dh2 is None or dh2.shape == h.shape)
    assert dinp is None or dinp.shape[0] == B * N
    _call("gptst_ccrnn_bwd_cand", _p(PT), PT.shape[1], PT.shape[0], _p(W1T), Cp, _p(dh), _p(dh2), _p(u), _p(c), _p(r), _p(h), _p(dpre1), _p(dpre0),
          _p(dh_part), _p(dinp), B, T, N, Hp, t, tiles, tag="Hp%d Cp%d k%d" % (Hp, Cp, PT.shape[0]), nbytes=_tg_nb(PT, W1T, h, 9 + (dh2 is not None)))


def ccrnn_bwd_state(PT, W0T, dpre0, dh_part, t, dh_out, B, T, N, dinp=None, tiles=0):
    """dh_out = dh_part + dstate, dinp += dinput of [dpre0[:, t] | P_j^T dpre0[:, t]]_j W0T^T"""
    _chk(PT, W0T, dpre0, dh_part, dh_out, dinp)
    Hp = dh_part.shape[1]
    Cp = dinp.shape[1] if dinp is not None else 0
    assert W0T.shape == (Hp + Cp, (PT.shape[0] + 1) * 2 * Hp) and dh_part.shape[0] == B * N and dpre0.shape == (B * T * N, 2 * Hp)
    assert dh_out.shape == dh_part.shape and (dinp is None or dinp.shape[0] == B * N)
    _call("gptst_ccrnn_bwd_state", _p(PT), PT.shape[1], PT.shape[0], _p(W0T), Cp, _p(dpre0), _p(dh_part), _p(dh_out), _p(dinp), B, T, N, Hp, t, tiles,
          tag="Hp%d Cp%d k%d" % (Hp, Cp, PT.shape[0]), nbytes=_tg_nb(PT, W0T, dh_part, 4))


# ---- the downstream MTGNN predictor (csrc/mtgnn.hip): tensors are (B * T * N rows, width) with T the tensor's own frame ----------------------
def mtgnn_tapgemm(X, W, bias, offs, B, Tsrc, Tdst, N, gated=False, xmask=None, omask=None, res=None, res_frame=None, res_off=0, out=None,
                  keep=False):
    """Y (B Tdst N, co)[b, to, n] = epi(sum_j (X xmask)[b, to + offs[j], n] W_j + bias); W (co | 2 co (gated), len(offs) * ci), tap-major columns.
    plain: epi(v) = (v + res[b, to + res_off, n]) omask, res of frame res_frame (default Tdst); out: the caller's buffer (out = res of the same frame
    accumulates in place).
    gated: tanh(P) sigmoid(Q) omask; keep -> (Y, tanh, sigmoid), what the backward needs."""
    _chk(X, W, bias, xmask, omask, res, out)
    ci = X.shape[1]
    co = W.shape[0] // 2 if gated else W.shape[0]
    assert X.shape[0] == B * Tsrc * N and W.shape[1] == len(offs) * ci and (xmask is None or xmask.shape == X.shape)
    Tr = Tdst if res_frame is None else res_frame
    assert res is None or (res.shape == (B * Tr * N, co) and not gated)
    Y = torch.empty(B * Tdst * N, co, device=X.device, dtype=torch.float32) if out is None else out
    assert Y.shape == (B * Tdst * N, co) and (omask is None or omask.shape == Y.shape)
    Tn, S = (torch.empty_like(Y), torch.empty_like(Y)) if keep else (None, None)
    _call("gptst_mtgnn_tapgemm", _p(X), ci, ci, _p(xmask), len(offs), _ints(offs), _p(W), _p(bias), _p(res), co, Tr, int(res_off), _p(omask), _p(Y),
          co, _p(Tn), _p(S), int(gated), B, Tsrc, Tdst, N, tag="ci%d co%d k%d g%d T%d>%d" % (ci, co, len(offs), int(gated), Tsrc, Tdst),
          nbytes=_nb(X, W, Y, Tn, S, xmask, omask, res))
    return (Y, Tn, S) if keep else Y


def mtgnn_gate_bwd(dG, Tn, S, omask=None):
    """dPre (rows, 2 co) = [dG omask S (1 - Tn^2) | dG omask Tn S (1 - S)]"""
    _chk(dG, Tn, S, omask)
    rows, co = dG.shape
    dPre = torch.empty(rows, 2 * co, device=dG.device, dtype=torch.float32)
    _call("gptst_mtgnn_gate_bwd", _p(dG), _p(Tn), _p(S), _p(omask), _p(dPre), rows, co, tag="co%d" % co, nbytes=_nb(dG, Tn, S, omask, dPre))
    return dPre


def mtgnn_wgrad(D, X, offs, B, Tsrc, Tdst, N, xmask=None, want_bias=True):
    """-> (dW (cw, len(offs) * ci) = sum D[b, to, n]^T (X xmask)[b, to + offs[j], n], db (cw)): row-split partials summed in a fixed order"""
    _chk(D, X, xmask)
    cw, ci = D.shape[1], X.shape[1]
    K = len(offs) * ci
    assert D.shape[0] == B * Tdst * N and X.shape[0] == B * Tsrc * N
    ns = _C.lib().value("gptst_stgcn_wgrad_nsplit", D.shape[0], cw, K)
    part = torch.empty(ns, cw, K, device=D.device, dtype=torch.float32)
    bpart = torch.empty(ns, cw, device=D.device, dtype=torch.float32) if want_bias else None
    _call("gptst_mtgnn_wgrad", _p(D), cw, _p(X), ci, ci, _p(xmask), len(offs), _ints(offs), _p(part), _p(bpart), ns, B, Tsrc, Tdst, N,
          tag="cw%d ci%d k%d T%d>%d" % (cw, ci, len(offs), Tsrc, Tdst), nbytes=_nb(D, X, part, xmask))
    return part.sum(0), (bpart.sum(0) if want_bias else None)


def mtgnn_graphgrad(D, X, N, c, ks, dcol0=0):
    """-> dM (ks, N, N), dM_k[v, w] = sum_{unit, ch} D[unit N + v, dcol0 + k c + ch] X[unit N + w, ch]: unit-split partials summed in a fixed order.
    X may be wider than c: its first c columns are read at its own row pitch (no copy of a column slice)"""
    _chk(D, X)
    rows = X.shape[0]
    assert D.shape[0] == rows and rows % N == 0 and X.shape[1] >= c and D.shape[1] >= dcol0 + ks * c
    units = rows // N
    ns = _C.lib().value("gptst_mtgnn_graphgrad_nsplit", units, N, ks)
    part = torch.empty(ns, ks, N, N, device=D.device, dtype=torch.float32)
    _call("gptst_mtgnn_graphgrad", _p(D), D.shape[1], dcol0, _p(X), X.shape[1], c, ks, _p(part), ns, units, N, tag="c%d ks%d" % (c, ks),
          nbytes=rows * (ks + 1) * c * 4 + part.numel() * 4)
    return part.sum(0)


# ---- the downstream ASTGCN predictor (csrc/astgcn.hip) ----------------------------------------------------------------------------------
def astgcn_attmix(Tp, S, In, T, c, reduce, res=None):
    """node mixing with the per-sample masked graph T_k * S_b (never written).  Tp (ks, Np, Np) zero-padded, S (B, N, N).
    reduce False: In (rows, c) -> (rows, ks c), Out[(b,t,n), k c + ch] = sum_m T_k[m,n] S[b,m,n] In[(b,t,m), ch];
    True: In (rows, ks c) -> (rows, c), Out[(b,t,m), ch] = sum_k sum_n T_k[m,n] S[b,m,n] In[(b,t,n), k c + ch] + res"""
    _chk(Tp, S, In, res)
    ks, Np = Tp.shape[0], Tp.shape[1]
    B, N = S.shape[0], S.shape[1]
    rows = In.shape[0]
    assert In.shape[1] == (ks * c if reduce else c) and rows == B * T * N and S.shape[2] == N
    Out = torch.empty(rows, c if reduce else ks * c, device=In.device, dtype=torch.float32)
    _call("gptst_astgcn_attmix", _p(Tp), Np, ks, _p(S), _p(In), _p(Out), _p(res), c, int(reduce), B, T, N, tag="c%d r%d" % (c, int(reduce)),
          nbytes=_nb(In, Out, res, S, Tp))
    return Out


def astgcn_attgrad(Tp, X, G, B, T, N):
    """-> dS (B, N, N) = sum_k T_k[m,n] sum_{t,ch} X[(b,t,m), ch] G[(b,t,n), k c + ch]: the gradient of astgcn_attmix (reduce False: X = In,
    G = dOut) with respect to S"""
    _chk(Tp, X, G)
    ks, Np = Tp.shape[0], Tp.shape[1]
    c = X.shape[1]
    assert X.shape[0] == B * T * N and G.shape == (B * T * N, ks * c)
    dS = torch.empty(B, N, N, device=X.device, dtype=torch.float32)
    _call("gptst_astgcn_attgrad", _p(Tp), Np, ks, _p(X), _p(G), _p(dS), c, B, T, N, tag="c%d" % c, nbytes=_nb(X, G, dS, Tp))
    return dS


def astgcn_rowln_fwd(X, gamma, beta, eps, keep=True):
    """LayerNorm over the c values of each row of X (rows, c) -> (Y, mean, rstd) (mean, rstd None when not kept)"""
    _chk(X, gamma, beta)
    rows, c = X.shape
    Y = torch.empty_like(X)
    mean, rstd = (torch.empty(rows, device=X.device, dtype=torch.float32) for _ in range(2)) if keep else (None, None)
    _call("gptst_astgcn_rowln_fwd", _p(X), _p(gamma), _p(beta), _p(Y), _p(mean), _p(rstd), rows, c, float(eps), tag="c%d" % c, nbytes=_nb(X, Y))
    return Y, mean, rstd


def astgcn_rowln_bwd(dY, X, gamma, mean, rstd):
    """-> dX of the LayerNorm over each row"""
    _chk(dY, X, gamma, mean, rstd)
    rows, c = X.shape
    dX = torch.empty_like(X)
    _call("gptst_astgcn_rowln_bwd", _p(dY), _p(X), _p(gamma), _p(mean), _p(rstd), _p(dX), rows, c, tag="c%d" % c, nbytes=_nb(dY, X, dX))
    return dX


def astgcn_rowln_bwd_param(dY, X, mean, rstd):
    """-> (dgamma, dbeta) (c values each): row-split partials summed in a fixed order"""
    _chk(dY, X, mean, rstd)
    rows, c = X.shape
    ns = _C.lib().value("gptst_astgcn_rowln_nsplit", rows)
    pg, pb = (torch.empty(ns, c, device=X.device, dtype=torch.float32) for _ in range(2))
    _call("gptst_astgcn_rowln_bwd_param", _p(dY), _p(X), _p(mean), _p(rstd), _p(pg), _p(pb), ns, rows, c, tag="c%d" % c, nbytes=_nb(dY, X))
    return pg.sum(0), pb.sum(0)


# ---- the downstream STSGCN predictor (csrc/stsgcn.hip) ----------------------------------------------------------------------------------
# row layouts of a layer over T frames, W = T - 2 windows: frames (B T N), expanded (B W 3 N): block (w, k) stands for frame w + k, middle (B W N)
MIX_F2E, MIX_E2E, MIX_E2M, MIX_M2E, MIX_E2F = 0, 1, 2, 3, 4
_MIX_ROWS = {MIX_F2E: ("f", "e"), MIX_E2E: ("e", "e"), MIX_E2M: ("e", "m"), MIX_M2E: ("m", "e"), MIX_E2F: ("e", "f")}


def _win_mix(entry, graphs, In, mode, span, B, T, N):
    """what stsgcn_mix and stfgnn_mix share: the row counts by layout for windows of ``span`` frames, the output, the tag and the byte count"""
    _chk(*graphs, In)
    W, c, Np = T - span + 1, In.shape[1], graphs[0].shape[0]
    rows = {"f": B * T * N, "e": B * W * span * N, "m": B * W * N}
    src, dst = _MIX_ROWS[mode]
    assert In.shape[0] == rows[src] and graphs[0].dim() == 2 and all(g.shape == graphs[0].shape for g in graphs), (In.shape, mode, B, T, N)
    Out = torch.empty(rows[dst], c, device=In.device, dtype=torch.float32)
    _call(entry, *(_p(g) for g in graphs), Np, _p(In), _p(Out), c, mode, B, T, N, tag="m%d c%d T%d" % (mode, c, T), nbytes=_nb(In, Out))
    return Out


def stsgcn_mix(Lp, In, mode, B, T, N):
    """mix(S)_k = L S_k + [k >= 1] S_{k-1} + [k <= 1] S_{k+1} without the (3N, 3N) matrix; Lp (Np, Np) = A^ zero-padded (its transpose for the
    adjoints).  mode: MIX_F2E frames -> expanded, MIX_E2E, MIX_E2M (the middle block only), MIX_M2E (adjoint of E2M), MIX_E2F (adjoint of F2E)."""
    return _win_mix("gptst_stsgcn_mix", (Lp,), In, mode, 3, B, T, N)


def stsgcn_wingemm(X, Wt, bias, act, B, W, R, N, keep=False, best=None, which=None, opj=0):
    """Y (B W R, co) = act(X Wt[w]^T + bias[w]) for the rows of window w; Wt (W, cw, ci) — or (1, cw, ci): one weight for all windows — and bias
    (W | 1, cw) or None; act ACT_GLU (cw = 2 co) or ACT_NONE.  R = N (middle rows), 3 N (STSGCN's expanded rows) or 4 N (STFGNN's); the middle
    block is rows N .. 2N of a group.  keep (GLU): -> (Y, S, A).  best (B W N, co) / which (int32): the running max on
    the middle block and the operation that holds it, updated in place (opj = 0 writes, later operations replace where strictly greater)."""
    _chk(X, Wt, bias, best)
    ci = X.shape[1]
    cw = Wt.shape[1]
    co = cw // 2 if act == ACT_GLU else cw
    assert X.shape[0] == B * W * R and R in (N, 3 * N, 4 * N) and Wt.shape[2] == ci and Wt.shape[0] in (1, W) and (bias is None or bias.shape == Wt.shape[:2])
    assert which is None or (which.dtype == torch.int32 and which.is_contiguous() and which.shape == best.shape)
    assert best is None or best.shape == (B * W * N, co)
    Y = torch.empty(B * W * R, co, device=X.device, dtype=torch.float32)
    S, A = (torch.empty_like(Y), torch.empty_like(Y)) if keep else (None, None)
    _call("gptst_stsgcn_wingemm", _p(X), ci, _p(Wt), _p(bias), int(Wt.shape[0] == 1 and W > 1), _p(Y), co, _p(S), _p(A), act, _p(best), _p(which), opj,
          B, W, R, N, tag="ci%d co%d act%d R%d W%d" % (ci, co, act, R // N, W), nbytes=_nb(X, Wt, Y, S, A))
    return (Y, S, A) if keep else Y


def stsgcn_gate_bwd(up, dBest, which, opj, S, A, B, W, R, N):
    """dPre (B W R, 2 co) of operation opj: g = up (or 0) + dBest [which == opj] on the middle block, through the GLU derivative"""
    _chk(up, dBest, S, A)
    co = S.shape[1]
    assert S.shape[0] == B * W * R and R in (N, 3 * N, 4 * N) and dBest.shape == (B * W * N, co) and which.dtype == torch.int32 and which.shape == dBest.shape
    dPre = torch.empty(B * W * R, 2 * co, device=S.device, dtype=torch.float32)
    _call("gptst_stsgcn_gate_bwd", _p(up), _p(dBest), _p(which), opj, _p(S), _p(A), _p(dPre), B, W, R, N, co, tag="co%d R%d W%d" % (co, R // N, W),
          nbytes=_nb(up, dBest, S, A, dPre))
    return dPre


def stsgcn_winwgrad(D, X, B, W, R):
    """-> (dW (W, cw, ci), db (W, cw)) per window: row-split partials summed in a fixed order"""
    _chk(D, X)
    cw, ci = D.shape[1], X.shape[1]
    assert D.shape[0] == X.shape[0] == B * W * R
    ns = _C.lib().value("gptst_stsgcn_winwgrad_nsplit", B * R, cw, ci, W)
    part = torch.empty(W, ns, cw, ci, device=D.device, dtype=torch.float32)
    bpart = torch.empty(W, ns, cw, device=D.device, dtype=torch.float32)
    _call("gptst_stsgcn_winwgrad", _p(D), cw, _p(X), ci, _p(part), _p(bpart), ns, B, W, R, tag="cw%d ci%d R%d W%d" % (cw, ci, R, W), nbytes=_nb(D, X, part))
    return part.sum(1), bpart.sum(1)


# ---- the downstream STFGNN predictor (csrc/stfgnn.hip) ----------------------------------------------------------------------------------
# row layouts of a layer over T frames, W = T - 3 windows: frames (B T N), expanded (B W 4 N): block (w, k) stands for frame w + k, middle (B W N).
# The modes are stsgcn_mix's (MIX_F2E ... MIX_E2F); the grouped GEMM, its gate backward and weight gradient are stsgcn_wingemm / stsgcn_gate_bwd /
# stsgcn_winwgrad with R = 4 N.
def stfgnn_mix(Sp, Dp, In, mode, B, T, N):
    """the product with the (4N, 4N) fusion graph as blocks: mix(X)_0 = mix(X)_3 = D (X_0 + X_3) + X_1 + X_2, mix(X)_k = S X_k + the other three
    for k = 1, 2.  Sp, Dp (Np, Np) = S^ and D zero-padded (their transposes for the adjoints).  mode: MIX_F2E frames -> expanded, MIX_E2E,
    MIX_E2M (block 1 only), MIX_M2E (adjoint of E2M), MIX_E2F (adjoint of F2E)."""
    return _win_mix("gptst_stfgnn_mix", (Sp, Dp), In, mode, 4, B, T, N)


# ---- the downstream STGODE predictor (csrc/stgode.hip) ----------------------------------------------------------------------------------
# rows (B T N, c), channels last.  A block is BN_nodes(relu(step(relu(X)))); the batch norm's channel is the node.
def stgode_step(Lp, In, W, M, B, T, N, coef, oscale=None, sscale=None, mask=None, relu_in=False, relu_out=False, keep_at=False):
    """Out[n] = cn oscale[n] (L (sscale . src))[n] + cw src[n] W + sum_k (ct M[tau][k] + [k = tau] cs) src[b, k, n], src = In or relu(In); coef =
    (cn, cw, ct, cs); Lp (Np, Np) zero-padded; then relu (relu_out) and the mask [mask > 0].  keep_at: -> (Out, AT), AT the bare node product"""
    _chk(Lp, In, W, M, oscale, sscale, mask)
    c = In.shape[1]
    assert In.shape[0] == B * T * N and tuple(W.shape) == (c, c) and tuple(M.shape) == (T, T) and Lp.dim() == 2, (In.shape, W.shape, M.shape, B, T, N)
    Out = torch.empty_like(In)
    AT = torch.empty_like(In) if keep_at else None
    _call("gptst_stgode_step", _p(Lp), Lp.shape[0], _p(In), _p(Out), _p(AT), _p(W), _p(M), _p(oscale), _p(sscale), _p(mask),
          *(ctypes.c_float(float(v)) for v in coef), int(relu_in), int(relu_out), c, B, T, N, tag="c%d T%d r%d" % (c, T, int(relu_in)),
          nbytes=_nb(In, Out, AT, mask))
    return (Out, AT) if keep_at else Out


def stgode_wgrad(G, X):
    """-> (c, c) = relu(X)^T G: row-split partials summed in a fixed order"""
    _chk(G, X)
    rows, c = G.shape
    ns = _C.lib().value("gptst_stgode_wgrad_nsplit", rows, c)
    part = torch.empty(ns, c, c, device=G.device, dtype=torch.float32)
    _call("gptst_stgode_wgrad", _p(G), _p(X), c, _p(part), ns, rows, tag="c%d" % c, nbytes=_nb(G, X, part))
    return part.sum(0).t()


def stgode_reduce(G, X, AT, B, T, N):
    """-> ((T, T) = sum_{b, n, c} relu(X)[b, k, n, c] G[b, m, n, c], (N) = sum_{b, tau, c} G AT): partials per (b, node chunk) summed in a fixed order"""
    _chk(G, X, AT)
    c = G.shape[1]
    nparts = _C.lib().value("gptst_stgode_reduce_nparts", c, T, N)
    part2 = torch.empty(B * nparts, T, T, device=G.device, dtype=torch.float32)
    parta = torch.empty(B, N, device=G.device, dtype=torch.float32)
    _call("gptst_stgode_reduce", _p(G), _p(X), _p(AT), _p(part2), _p(parta), c, B, T, N, tag="c%d T%d" % (c, T), nbytes=_nb(G, X, AT))
    return part2.sum(0), parta.sum(0)


def stgode_bn_stats(Z, B, T, N):
    """-> part (N, nsplit, 2): (mean, sum of squared deviations from it) of each split of a node's B T rows"""
    _chk(Z)
    ns = _C.lib().value("gptst_stgode_bn_nsplit", B * T)
    part = torch.empty(N, ns, 2, device=Z.device, dtype=torch.float32)
    _call("gptst_stgode_bn_stats", _p(Z), _p(part), ns, Z.shape[1], B, T, N, tag="c%d" % Z.shape[1], nbytes=_nb(Z))
    return part


def stgode_bn_apply(Z, part, gamma, beta, rmean, rvar, training, momentum, eps, B, T, N, keep=False, best=None, which=None, idx=0, want_y=True):
    """batch norm over the node channel from the split statistics (part None: from the running ones) -> (Y | None, mean | None, rstd | None).
    training: rmean / rvar are updated in place.  best / which: the running max over the branches, branch ``idx``"""
    _chk(Z, part, gamma, beta, rmean, rvar, best)
    ns = _C.lib().value("gptst_stgode_bn_nsplit", B * T)
    assert part is None or tuple(part.shape) == (N, ns, 2)
    assert which is None or (which.dtype == torch.int32 and which.is_contiguous() and which.shape == Z.shape)
    Y = torch.empty_like(Z) if want_y else None
    mean, rstd = (torch.empty(N, device=Z.device, dtype=torch.float32) for _ in range(2)) if keep else (None, None)
    _call("gptst_stgode_bn_apply", _p(Z), _p(part), ns, _p(gamma), _p(beta), _p(rmean), _p(rvar), int(training), ctypes.c_float(float(momentum)),
          ctypes.c_float(float(eps)), _p(Y), _p(mean), _p(rstd), _p(best), _p(which), idx, Z.shape[1], B, T, N,
          tag="c%d m%d" % (Z.shape[1], int(best is not None)), nbytes=_nb(Z, Y, best))
    return Y, mean, rstd


def stgode_bn_bwd(dY, Z, gamma, mean, rstd, B, T, N, dBest=None, which=None, idx=0):
    """-> (G = [Z > 0] dZ of the batch norm over the node channel, dgamma (N), dbeta (N)); dY None: the upstream gradient is dBest where
    which == idx.  Two launches: the per-node sums as split partials, then the apply"""
    _chk(dY, Z, gamma, mean, rstd, dBest)
    ns = _C.lib().value("gptst_stgode_bn_nsplit", B * T)
    part = torch.empty(N, ns, 2, device=Z.device, dtype=torch.float32)
    G = torch.empty_like(Z)
    dg, db = (torch.empty(N, device=Z.device, dtype=torch.float32) for _ in range(2))
    for stage in (0, 1):
        _call("gptst_stgode_bn_bwd", _p(dY), _p(dBest), _p(which), idx, _p(Z), _p(gamma), _p(mean), _p(rstd), _p(part), ns, _p(G), _p(dg), _p(db),
              Z.shape[1], B, T, N, stage, tag="c%d s%d" % (Z.shape[1], stage), nbytes=_nb(Z, dY, dBest) + (stage and _nb(G)))
    return G, dg, db


# ---- the downstream MSDR predictor's multi-state recurrence (csrc/msdr.hip) -----------------------------------------------------------------
# TIME-major rows: a seq tensor is (T*B*N, width) with row (t B + b) N + n; the state ring Hs and its gradient dH are (T + K, B*N, Hp), slot
# K + t the output of step t.  Outputs are the caller's buffers (the loop owns them).
def msdr_groups(N, B, tiles=0):
    """workgroups per sample of the step launches: the length of a row of their partials"""
    return _C.lib().value("gptst_msdr_groups", N, B, tiles)


def msdr_fwd_step(Lp, Wh, W2, bvec, R, w, wr, Gx, Hs, sig, t, B, T, N, w2=None, sig2=None, c=None, z=None, a=None, tiles=0):
    """o = leaky_relu([h | L_k h]_k Wh^T + Gx[t]) W2^T + b + sum_k a_k (s_k + R_k) -> Hs[K + t], with s_k = Hs[t + k], h = s_{K-1} and
    a = softmax_k(sum(sig[t + k]) + wr[k]);  sig[K + t] (and sig2 with w2) = per-workgroup partials of w . o;  kept when given: c, z, a"""
    _chk(Lp, Wh, W2, bvec, R, w, w2, wr, Gx, Hs, sig, sig2, c, z, a)
    K, Hp, ks = R.shape[0], Hs.shape[2], Lp.shape[0]
    G = msdr_groups(N, B, tiles)
    assert Wh.shape == (Hp, (ks + 1) * Hp) and W2.shape == (Hp, Hp) and bvec.shape == w.shape == (N, Hp) and R.shape == (K, N, Hp)
    assert Hs.shape == (T + K, B * N, Hp) and sig.shape == (T + K, B, G) and Gx.shape == (T * B * N, Hp) and wr.shape == (K,)
    assert (w2 is None) == (sig2 is None) and (sig2 is None or (sig2.shape == sig.shape and w2.shape == w.shape))
    assert (c is None or c.shape == Gx.shape) and (z is None or z.shape == (T * B * N, (ks + 1) * Hp)) and (a is None or a.shape == (T, B, K))
    _call("gptst_msdr_fwd_step", _p(Lp), Lp.shape[1], ks, _p(Wh), _p(W2), _p(bvec), _p(R), _p(w), _p(w2), _p(wr), _p(Gx), _p(Hs), _p(sig),
          _p(sig2), _p(c), _p(z), (ks + 1) * Hp, _p(a), B, T, N, Hp, K, t, tiles, tag="Hp%d ks%d K%d" % (Hp, ks, K),
          nbytes=_nb(Lp, Wh, W2, bvec, R, w) + (K + 2 + (c is not None) + (ks + 1) * (z is not None)) * B * N * Hp * 4)


def msdr_bwd_pre(W, R, Hs, dH, c, dpre, pa, t, B, T, N, tiles=0):
    """dpre[t] = (dH[K + t] W^T) leaky'(c[t]);  pa[b, g, k] = the workgroup's share of <dH[K + t], Hs[t + k] + R_k>"""
    _chk(W, R, Hs, dH, c, dpre, pa)
    K, Hp = R.shape[0], Hs.shape[2]
    assert W.shape == (Hp, Hp) and Hs.shape == dH.shape == (T + K, B * N, Hp) and c.shape == dpre.shape == (T * B * N, Hp)
    assert pa.shape == (B, msdr_groups(N, B, tiles), 8)
    _call("gptst_msdr_bwd_pre", _p(W), _p(R), _p(Hs), _p(dH), _p(c), _p(dpre), _p(pa), B, T, N, Hp, K, t, tiles, tag="Hp%d K%d" % (Hp, K),
          nbytes=_nb(W, R) + (K + 3) * B * N * Hp * 4)


def msdr_bwd_state(LpT, WhT, w, a, pa, dpre, dH, de, t, B, T, N, tiles=0):
    """de[t] = a (dA - sum a dA) with dA = the fold of pa;  dH[t + k] += a_k dH[K + t] + de_k w, and dH[t + K - 1] += [dpre | L_k^T dpre]_k WhT^T"""
    _chk(LpT, WhT, w, a, pa, dpre, dH, de)
    K, Hp, ks = a.shape[2], dH.shape[2], LpT.shape[0]
    assert WhT.shape == (Hp, (ks + 1) * Hp) and w.shape == (N, Hp) and dH.shape == (T + K, B * N, Hp) and dpre.shape == (T * B * N, Hp)
    assert a.shape == de.shape == (T, B, K) and pa.shape == (B, msdr_groups(N, B, tiles), 8)
    _call("gptst_msdr_bwd_state", _p(LpT), LpT.shape[1], ks, _p(WhT), _p(w), _p(a), _p(pa), _p(dpre), _p(dH), _p(de), B, T, N, Hp, K, t, tiles,
          tag="Hp%d ks%d K%d" % (Hp, ks, K), nbytes=_nb(LpT, WhT, w) + (2 * K + 2) * B * N * Hp * 4)


# ---- the downstream ST-WA predictor's cuts (csrc/stwa.hip) ----------------------------------------------------------------------------------
# One cut of a Layer: two launches forward, three backward.  h (B, T, N, C); prox (2 cuts, N, C); Y (B, cuts, N, C) holds out_0 .. out_{cuts-1};
# co, cb (B, N, 4, 5); V (4, 6, C, C); u (4, 6, C); Wl, WlT (6, C, C); bl (6, C).  Outputs are the caller's buffers (the loop owns them).
def stwa_lds_bytes(N, C):
    """the dynamic LDS of the widest of the five launches (negative: the width is not served)"""
    return _C.lib().value("gptst_stwa_lds_bytes", N, C)


def stwa_slab_shape(B, N, C):
    """(workgroups, floats) of the weight-gradient slab: one row per workgroup, [dV (4, 6, C, C) | du (4, 6, C) | dWl (6, C, C) | dbl (6, C)]"""
    return B * ((N + 15) // 16), _C.lib().value("gptst_stwa_slab_floats", C)


def _stwa_dims(h, prox, Y, co, cb, V, u):
    B, T, N, C = h.shape
    cuts = Y.shape[1]
    assert prox.shape == (2 * cuts, N, C) and Y.shape == (B, cuts, N, C) and co.shape == cb.shape == (B, N, 4, 5)
    assert V.shape == (4, 6, C, C) and u.shape == (4, 6, C)
    return B, T, N, C, cuts


def stwa_local_fwd(h, prox, Y, co, cb, V, u, WlT, bl, Tq, Ks, Vs, cut, cs):
    """rows = [prox[2 cut : 2 cut + 2] + Y[:, cut - 1] | h[:, cut cs : (cut + 1) cs]];  Tq = tp2(tanh(tp1(temporal attention of the 2 proxy rows
    over all rows, keys and values by the generated maps 0, 1)));  Ks, Vs = the generated maps 2, 3 of Tq"""
    _chk(h, prox, Y, co, cb, V, u, WlT, bl, Tq, Ks, Vs)
    B, T, N, C, cuts = _stwa_dims(h, prox, Y, co, cb, V, u)
    assert WlT.shape == (6, C, C) and bl.shape == (6, C) and Tq.shape == Ks.shape == Vs.shape == (B, 2, N, C)
    _call("gptst_stwa_local_fwd", _p(h), _p(prox), _p(Y), _p(co), _p(cb), _p(V), _p(u), _p(WlT), _p(bl), _p(Tq), _p(Ks), _p(Vs), B, T, N, C, cuts,
          cut, cs, tag="C%d cs%d" % (C, cs), nbytes=_nb(Tq, Ks, Vs, V, u, WlT) + (3 + cs) * B * N * C * 4)


def stwa_spatial_fwd(Tq, Ks, Vs, WlT, bl, Y, cut, S=None, mx=None, sm=None):
    """Y[:, cut] = sum_p g U with U = sp2(relu(sp1(softmax_nodes(Tq Ks^T / sqrt(C / 8)) Vs))) per (sample, proxy, head), g = sigmoid(ag2(relu(
    ag1(U))));  kept when given: S (the mixed values), mx, sm (each softmax row's maximum and sum)"""
    _chk(Tq, Ks, Vs, WlT, bl, Y, S, mx, sm)
    B, _, N, C = Tq.shape
    assert Ks.shape == Vs.shape == Tq.shape and Y.shape[0] == B and Y.shape[2:] == (N, C) and (mx is None) == (sm is None)
    assert (S is None or S.shape == Tq.shape) and (mx is None or mx.shape == sm.shape == (B, 2, N, 8))
    _call("gptst_stwa_spatial_fwd", _p(Tq), _p(Ks), _p(Vs), _p(WlT), _p(bl), _p(Y), _p(S), _p(mx), _p(sm), B, N, C, Y.shape[1], cut,
          tag="C%d N%d" % (C, N), nbytes=_nb(Tq, Ks, Vs, S, mx, sm) + B * N * C * 4)


def stwa_spatial_bwd_q(Tq, Ks, Vs, S, mx, sm, Wl, WlT, bl, dY, carry, dS, Dq, dTq, slab, cut):
    """the gradient of Y[:, cut] (dY[:, cut] + carry) back through the gate and the spatial projections -> dS, Dq = <dS, S> per head, and the
    query side of the spatial attention -> dTq;  slab (may be None) += the four Linears' gradients"""
    _chk(Tq, Ks, Vs, S, mx, sm, Wl, WlT, bl, dY, carry, dS, Dq, dTq, slab)
    B, _, N, C = Tq.shape
    assert Ks.shape == Vs.shape == S.shape == dS.shape == dTq.shape == Tq.shape and mx.shape == sm.shape == Dq.shape == (B, 2, N, 8)
    assert dY.shape[0] == B and dY.shape[2:] == (N, C) and (carry is None or carry.shape == (B, N, C))
    assert slab is None or slab.shape == stwa_slab_shape(B, N, C)
    _call("gptst_stwa_spatial_bwd_q", _p(Tq), _p(Ks), _p(Vs), _p(S), _p(mx), _p(sm), _p(Wl), _p(WlT), _p(bl), _p(dY), _p(carry), _p(dS), _p(Dq),
          _p(dTq), _p(slab), B, N, C, dY.shape[1], cut, tag="C%d N%d" % (C, N), nbytes=_nb(Tq, Ks, Vs, S, dS, dTq, slab) + 2 * B * N * C * 4)


def stwa_spatial_bwd_kv(Tq, Ks, Vs, dS, Dq, mx, sm, dKs, dVs):
    """the key / value side of the spatial attention: a key's gradient summed over the query nodes of its sample in index order"""
    _chk(Tq, Ks, Vs, dS, Dq, mx, sm, dKs, dVs)
    B, _, N, C = Tq.shape
    assert Ks.shape == Vs.shape == dS.shape == dKs.shape == dVs.shape == Tq.shape and mx.shape == sm.shape == Dq.shape == (B, 2, N, 8)
    _call("gptst_stwa_spatial_bwd_kv", _p(Tq), _p(Ks), _p(Vs), _p(dS), _p(Dq), _p(mx), _p(sm), _p(dKs), _p(dVs), B, N, C, tag="C%d N%d" % (C, N),
          nbytes=_nb(Tq, Ks, Vs, dS, dKs, dVs))


def stwa_local_bwd(h, prox, Y, co, cb, V, u, Wl, WlT, bl, dTq, dKs, dVs, dh, dPb, carry, dco, dcb, slab, cut, cs):
    """the node-local half backwards (its forward recomputed): dh rows of the cut, dPb[:, 2 cut : 2 cut + 2] (the proxies' gradient per sample),
    carry = the gradient of Y[:, cut - 1] — each written when given;  dco, dcb +=;  slab (may be None) += dV, du, the temporal Linears"""
    _chk(h, prox, Y, co, cb, V, u, Wl, WlT, bl, dTq, dKs, dVs, dh, dPb, carry, dco, dcb, slab)
    B, T, N, C, cuts = _stwa_dims(h, prox, Y, co, cb, V, u)
    assert dTq.shape == dKs.shape == dVs.shape == (B, 2, N, C) and dco.shape == dcb.shape == co.shape
    assert (dh is None or dh.shape == h.shape) and (dPb is None or dPb.shape == (B, 2 * cuts, N, C)) and (carry is None or carry.shape == (B, N, C))
    assert slab is None or slab.shape == stwa_slab_shape(B, N, C)
    _call("gptst_stwa_local_bwd", _p(h), _p(prox), _p(Y), _p(co), _p(cb), _p(V), _p(u), _p(Wl), _p(WlT), _p(bl), _p(dTq), _p(dKs), _p(dVs), _p(dh),
          _p(dPb), _p(carry), _p(dco), _p(dcb), _p(slab), B, T, N, C, cuts, cut, cs, tag="C%d cs%d" % (C, cs),
          nbytes=_nb(dTq, dKs, dVs, slab, V, u) + (6 + 2 * cs) * B * N * C * 4)


# ---- the downstream ST-MGCN predictor's stacked LSTM (csrc/stmgcn.hip) ------------------------------------------------------------------------
# TIME-major: Gx0 (T, rows, 4H);  W the flat [W_hh0 (4H, H) | [W_ih_l | W_hh_l] (4H, 2H) ..], WT the transposes in the same order;  bias (L, 4H)
def stmgcn_lds_bytes(H, L, tiles):
    """the larger dynamic LDS of the two launches with `tiles` (1 or 2) 16-row tiles per workgroup"""
    return _C.lib().value("gptst_stmgcn_lds_bytes", H, L, tiles)


def stmgcn_tiles(rows, H, L, forced=0):
    """16-row tiles per workgroup of both launches (negative: the shape is not served)"""
    return _C.lib().value("gptst_stmgcn_tiles", rows, H, L, forced)


def stmgcn_wsize(H, L):
    return 4 * H * H + (L - 1) * 8 * H * H


def stmgcn_lstm_fwd(Gx0, W, bias, L, keep, tiles=0):
    """all T steps of all L layers in ONE launch -> (top (T, rows, H), gates, c, h): keep False: the top ring alone (the rest None); keep True:
    gates (L, T, rows, 4H), c (L, T, rows, H), h (L, T + 1, rows, H) with slot 0 zero, and top = h[L - 1, 1:]"""
    _chk(Gx0, W, bias)
    T, rows, H4 = Gx0.shape
    H = H4 // 4
    assert H4 == 4 * H and W.numel() == stmgcn_wsize(H, L) and bias.shape == (L, H4)
    top = gates = c = h = None
    if keep:
        gates, c, h = Gx0.new_empty(L, T, rows, H4), Gx0.new_empty(L, T, rows, H), Gx0.new_empty(L, T + 1, rows, H)
        h[:, 0] = 0
    else:
        top = Gx0.new_empty(T, rows, H)
    _call("gptst_stmgcn_lstm_fwd", _p(Gx0), _p(W), _p(bias), _p(top), _p(gates), _p(c), _p(h), rows, T, L, H, tiles, tag="H%d L%d T%d" % (H, L, T),
          nbytes=_nb(Gx0, W, bias, top, gates, c, h))
    return (h[L - 1, 1:] if keep else top), gates, c, h


def stmgcn_lstm_bwd(dTop, WT, gates, c, dG_layers, tiles=0):
    """ONE launch -> dG (dG_layers, T, rows, 4H): the gradient of the pre-activations of layers 0 .. dG_layers - 1 (dG[0] is dGx0)"""
    _chk(dTop, WT, gates, c)
    L, T, rows, H4 = gates.shape
    H = H4 // 4
    assert dTop.shape == (T, rows, H) and c.shape == (L, T, rows, H) and WT.numel() == stmgcn_wsize(H, L) and 1 <= dG_layers <= L
    dG = dTop.new_empty(dG_layers, T, rows, H4)
    _call("gptst_stmgcn_lstm_bwd", _p(dTop), _p(WT), _p(gates), _p(c), _p(dG), dG_layers, rows, T, L, H, tiles, tag="H%d L%d T%d" % (H, L, T),
          nbytes=_nb(dTop, WT, gates, c, dG))
    return dG


# ---- the downstream DMVSTNET predictor's semantic view (csrc/dmvstnet.hip) -----------------------------------------------------------------------
def dmvst_sen_fwd(x, V, c, N):
    """z (rows, O) = x[r] V[r mod N] + c[r mod N];  x (rows = units N, C), V (N, C, O), c (N, O)"""
    _chk(x, V, c)
    rows, C = x.shape
    O = V.shape[2]
    assert rows % N == 0 and V.shape == (N, C, O) and c.shape == (N, O)
    z = x.new_empty(rows, O)
    _call("gptst_dmvst_sen_fwd", _p(x), _p(V), _p(c), _p(z), rows // N, N, C, O, tag="C%d O%d" % (C, O), nbytes=_nb(x, V, c, z))
    return z


def dmvst_sen_bwd(x, V, dz, N):
    """-> (dx (rows, C) = dz V[n]^T, dV (N, C, O) = sum over the units of x^T dz, dc (N, O) = that of dz): unit-split partials summed in a
    fixed order"""
    _chk(x, V, dz)
    rows, C = x.shape
    O = V.shape[2]
    assert rows % N == 0 and V.shape == (N, C, O) and dz.shape == (rows, O)
    ns = _C.lib().value("gptst_dmvst_sen_nsplit", rows // N, N)
    dx, pV, pc = torch.empty_like(x), x.new_empty(ns, N, C, O), x.new_empty(ns, N, O)
    _call("gptst_dmvst_sen_bwd", _p(x), _p(V), _p(dz), _p(dx), _p(pV), _p(pc), ns, rows // N, N, C, O, tag="C%d O%d" % (C, O),
          nbytes=_nb(x, V, dz, dx, pV, pc))
    return dx, pV.sum(0), pc.sum(0)
