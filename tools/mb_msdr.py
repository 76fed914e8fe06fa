#!/usr/bin/env python
"""The downstream MSDR predictor at the shapes of its confs — (B, T, N, C) = (64, 12, 170, 64) (PEMS08) and (64, 12, 266, 64) (NYC_TAXI, two
output channels): two encoder and two decoder layers of 12 cell steps, pre_k = 4, one scaled-Laplacian support and the adaptive graph: the HIP
backend (csrc/msdr.hip and the hoisted kernels) against the torch backend of the same module — the reference's own operations through
PyTorch-ROCm — on the same GPU, in the same call.  W, b and R are moved off their zero initialisation first (at it every state is 0).
usage (GPU box, repo root):
    python tools/mb_msdr.py                     per shape: predictor forward + backward and forward under no_grad, the two backends alternating,
                                                device events, rounds after warm-up; the peak memory of a forward + backward of each backend;
                                                the launches of the HIP pass summed by entry; the EvalTrainer loop body at the first shape;
                                                [--out FILE] (default profiles/msdr_hip_ab.txt)
    python tools/mb_msdr.py --trace torch|hip   30 forward + backward passes of one backend at the first shape and nothing else"""
import statistics
import sys

import torch

import mb_downstream as mb
import mb_stsgcn as ss
from mb_downstream import dev, say
from gptst_amd import graph, ops
from gptst_amd.config import predictor_args

from gptst_amd.predictors import MSDR

SHAPES = [("PEMS08", (64, 12, 170, 64)), ("NYC_TAXI", (64, 12, 266, 64))]


def make_predictor(ds):
    def predictor(backend):
        p = predictor_args(ds, "MSDR")
        p.supports = graph.msdr_supports(graph.synthetic_adjacency(p.num_nodes, 2), p.filter_type)
        torch.manual_seed(0)
        m = MSDR(p, dev, 64, backend=backend)
        with torch.no_grad():
            for c in m.cells():
                c.W.normal_(0, 1 / 32)
                c.b.normal_(0, 0.1)
                c.R.normal_(0, 0.1)
        return m.train()
    return predictor


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
        acc.setdefault(name, []).append((e0.elapsed_time(e1) * 1e3, nbytes))
    ops.TIMER = None
    say("the launches of one HIP forward + backward, summed by entry (device events around each launch, %d passes; us = launches x their median;" % passes)
    say("bytes = every operand once, against %.1f TB/s):" % mb.PEAK_TBS)
    say("  %-26s %4s %10s %10s %9s" % ("entry", "n", "us", "median us", "MB"))
    total = 0.0
    for name in order:
        v = acc[name]
        n, m_us = len(v) // passes, statistics.median(t for t, _ in v)
        total += n * m_us
        say("  %-26s %4d %10.1f %10.2f %9.1f" % (name[6:], n, n * m_us, m_us, sum(b for _, b in v) / passes / 1e6))
    return total


if __name__ == "__main__":
    if "--trace" in sys.argv:
        mb.trace(make_predictor("PEMS08"), SHAPES[0][1], sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    for i, (ds, shape) in enumerate(SHAPES):
        B, T, N, C = shape
        predictor = make_predictor(ds)
        pa = predictor_args(ds, "MSDR")
        say("MSDR predictor (%s conf) at (B, T, N, C) = (%d, %d, %d, %d), %d + %d layers of %d steps, rnn_units %d, pre_k %d, %s"
            % (ds, B, T, N, C, pa.num_rnn_layers, pa.num_rnn_layers, T, pa.rnn_units, pa.pre_k, torch.cuda.get_device_name(0)))
        mh, x, w, pass_ms = mb.ab_predictor(predictor, shape, warm=3, reps=5)
        total = by_entry(mh, x, w)
        say("  sum of the launches above: %.1f us per pass = %.1f%% of the %.3f ms pass" % (total, total / 10 / pass_ms, pass_ms))
        del mh, x, w
        torch.cuda.empty_cache()
        ss.peak_memory(predictor, shape)
        if i == 0:
            mb.ab_step(lambda backend, args: predictor(backend), shape, "MSDR", "msdr_backend", warm=3, steps=10)
        say()
    mb.write_out("msdr_hip_ab.txt")
