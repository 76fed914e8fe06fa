#!/usr/bin/env python
"""The downstream STSGCN predictor at the shapes of its confs — (B, T, N, C) = (64, 12, 170, 64), four layers of [64, 64, 64] (PEMS08), and
(64, 12, 266, 64), one layer (NYC_TAXI, two output channels): the HIP backend (csrc/stsgcn.hip + the tap GEMM of csrc/stgcn.hip for the first
embedding) against the torch backend of the same module, on the same GPU, in the same call.
usage (GPU box, repo root):
    python tools/mb_stsgcn.py                     per shape: predictor forward + backward and forward under no_grad, the two backends alternating,
                                                  device events, 7 rounds after warm-up; the peak memory of a forward + backward of each backend;
                                                  the launches of the HIP pass with the flops / bytes of their shapes — each launch for the one-layer
                                                  shape, summed by entry for the four-layer one; the heads, kept in torch, timed alone; the
                                                  EvalTrainer loop body at the first shape; [--out FILE] (default profiles/stsgcn_hip_ab.txt)
    python tools/mb_stsgcn.py --trace torch|hip   30 forward + backward passes of one backend at the first shape and nothing else"""
import statistics
import sys

import torch

import mb_downstream as mb
from mb_downstream import dev, events, med, say
from gptst_amd import graph, ops
from gptst_amd.config import make_args, predictor_args

from gptst_amd.predictors import STSGCN

SHAPES = [("PEMS08", (64, 12, 170, 64)), ("NYC_TAXI", (64, 12, 266, 64))]


def row_normalised(n):
    """a sensor-like graph with rows normalised to sum 1 (a raw 0/1 adjacency with a unit diagonal added grows the activations layer by layer)"""
    a = graph.synthetic_adjacency(n, 2)
    return a / a.sum(1, keepdims=True)


def make_predictor(ds):
    def predictor(backend):
        p = predictor_args(ds, "STSGCN")
        p.A = row_normalised(p.num_nodes)
        torch.manual_seed(0)
        m = STSGCN(p, dev, 64, make_args(ds).output_dim, backend=backend)
        with torch.no_grad():                                        # non-zero position embeddings, as after training
            for k, q in m.named_parameters():
                if k.endswith("_emb"):
                    q.normal_(0, 0.3)
        return m.train()
    return predictor


def flops_of(name, a):
    """useful floating-point operations of one launch from its arguments (the entry's argument order, include/gptst_hip.h)"""
    if name == "gptst_stgcn_tapgemm":
        ci, ntap, co, rows = a[2], a[3], a[14], a[18]
        return 2.0 * rows * ntap * ci * co
    if name == "gptst_stgcn_wgrad":
        cw, ci, ntap, rows = a[1], a[4], a[5], a[13]
        return 2.0 * rows * cw * ntap * ci
    if name == "gptst_stsgcn_mix":
        c, mode, b, t, n = a[4], a[5], a[6], a[7], a[8]
        units = b * t if mode in (ops.MIX_F2E, ops.MIX_E2F) else b * (t - 2) * (3 if mode == ops.MIX_E2E else 1)
        return 2.0 * units * n * n * c
    if name == "gptst_stsgcn_wingemm":
        ci, co, act, b, w, r = a[1], a[6], a[9], a[13], a[14], a[15]
        return 2.0 * b * w * r * ci * co * (2 if act == ops.ACT_GLU else 1)
    if name == "gptst_stsgcn_winwgrad":
        cw, ci, b, w, r = a[1], a[3], a[7], a[8], a[9]
        return 2.0 * b * w * r * cw * ci
    return 0.0


def by_entry(m, x, w, passes=5):
    """the launches of the HIP pass summed by entry point -> the sum, us per pass"""
    ops.TIMER = []
    for _ in range(passes):
        mb.fb(m, x, w)
    torch.cuda.synchronize()
    acc, order = {}, []
    for name, tag, e0, e1, nbytes in ops.TIMER:
        if name not in acc:
            order.append(name)
        d = acc.setdefault(name, {})
        d.setdefault(tag, []).append((e0.elapsed_time(e1) * 1e3, nbytes))
    ops.TIMER = None
    say("the launches of one HIP forward + backward, summed by entry (device events around each launch, %d passes; us = sum over the entry's launches" % passes)
    say("of each launch's median; bound = sum of max(flops / %.1f TFLOP/s, bytes / %.1f TB/s) per launch, bytes = every operand once):" % (mb.PEAK_TFLOPS, mb.PEAK_TBS))
    say("  %-26s %3s %9s %9s %9s %9s %7s" % ("entry", "n", "us", "GFLOP", "MB", "bound us", "share"))
    total = 0.0
    for name in order:
        n = us = fl = by = bound = 0.0
        for tag, v in acc[name].items():
            k = len(v) // passes
            f, b = flops_of(name, ops.LAST_CALL[(name, tag)]), v[0][1]
            n, us, fl, by = n + k, us + k * statistics.median(t for t, _ in v), fl + k * f, by + k * b
            bound += k * max(f / mb.PEAK_TFLOPS / 1e6, b / mb.PEAK_TBS / 1e6)
        total += us
        say("  %-26s %3d %9.1f %9.2f %9.1f %9.1f %6.1f%%" % (name[6:], n, us, fl / 1e9, by / 1e6, bound, 100 * bound / us))
    return total


def peak_memory(predictor, shape):
    """peak allocated bytes of one forward + backward of each backend, above what is allocated before it (the model, x, w)"""
    out = {}
    for k in ("torch", "hip"):
        m = predictor(k)
        x, w = mb.inputs(shape)
        mb.fb(m, x, w)
        for p in m.parameters():
            p.grad = None
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        mb.fb(m, x, w)
        torch.cuda.synchronize()
        out[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        del m, x, w
        torch.cuda.empty_cache()
    say("peak memory of one forward + backward above the model and its input: torch %.0f MiB, hip %.0f MiB" % (out["torch"], out["hip"]))


def heads(m, shape, t_out, pass_ms):
    B, _, N, _ = shape
    h = torch.randn(B, t_out, N, 64, device=dev, requires_grad=True)

    def f():
        h.grad = None
        m.head(h).square().sum().backward()
    for _ in range(3):
        f()
    th = [events(f, 5) for _ in range(5)]
    say("kept in torch, timed alone (forward + backward, device events, 5 rounds of 5), ms median (min - max): the stacked heads %s = %.1f%% of the pass"
        % (med(th), 100 * statistics.median(th) / pass_ms))


if __name__ == "__main__":
    if "--trace" in sys.argv:
        mb.trace(make_predictor("PEMS08"), SHAPES[0][1], sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    for i, (ds, shape) in enumerate(SHAPES):
        B, T, N, C = shape
        predictor = make_predictor(ds)
        layers = len(predictor_args(ds, "STSGCN").filter_list)
        say("STSGCN predictor (%s conf) at (B, T, N, C) = (%d, %d, %d, %d), %d layer(s) of [64, 64, 64], %s" % (ds, B, T, N, C, layers, torch.cuda.get_device_name(0)))
        mh, x, w, pass_ms = mb.ab_predictor(predictor, shape, warm=3, reps=5)
        if layers == 1:
            total = mb.per_kernel(mh, x, w, flops_of, passes=5)
        else:
            total = by_entry(mh, x, w)
        say("  sum of the launches above: %.1f us per pass = %.1f%% of the %.3f ms pass" % (total, total / 10 / pass_ms, pass_ms))
        heads(mh, shape, T - 2 * layers, pass_ms)
        del mh, x, w
        torch.cuda.empty_cache()
        peak_memory(predictor, shape)
        if i == 0:
            mb.ab_step(lambda backend, args: predictor(backend), shape, "STSGCN", "stsgcn_backend", warm=3, steps=10)
        say()
    mb.write_out("stsgcn_hip_ab.txt")
