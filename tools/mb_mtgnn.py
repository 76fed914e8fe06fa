#!/usr/bin/env python
"""The downstream MTGNN predictor at the MTGNN conf's PEMS08 shape (B, T, N, C) = (64, 12, 170, 64 -> 12 x 1; conv = residual 32, skip 64, end 128,
three layers, subgraph_size 20), training mode with the conf's dropout 0.3: the HIP backend (csrc/mtgnn.hip + the node mix, one-tap GEMM, weight
gradient and LayerNorm of csrc/stgcn.hip) against the torch backend of the same module, on the same GPU, in the same call.
usage (GPU box, repo root):
    python tools/mb_mtgnn.py                      predictor forward + backward and forward under no_grad, the two backends alternating, device events,
                                                  7 rounds after warm-up; each launch of the HIP pass with the flops / bytes of its shapes; the
                                                  EvalTrainer loop body, frozen and fine-tuned; [--out FILE] (default profiles/mtgnn_hip_ab.txt)
    python tools/mb_mtgnn.py --trace torch|hip    30 forward + backward passes of one backend and nothing else (for tools/prof.sh)"""
import contextlib
import statistics
import sys
from types import SimpleNamespace

import torch

import mb_downstream as mb
from mb_downstream import PEAK_TBS, PEAK_TFLOPS, dev, fb, say
from gptst_amd import ops
from gptst_amd.config import predictor_args
from gptst_amd.predictors import MTGNN

B, T, N, C = SHAPE = 64, 12, 170, 64


def ap():
    return SimpleNamespace(**vars(predictor_args("PEMS08", "MTGNN")), adj_mx=None)


def predictor(backend):
    torch.manual_seed(0)
    return MTGNN(ap(), dev, C, 1, backend=backend).to(dev).train()


def step_predictor(backend, args):
    torch.manual_seed(0)
    return MTGNN(ap(), dev, args.hidden_dim, args.output_dim, backend=backend)


@contextlib.contextmanager
def no_dropout(ms):
    """the outputs are compared without dropout: the backends draw their masks from different streams"""
    for m in ms.values():
        m._keep = lambda tag, like: None
    yield
    for m in ms.values():
        del m._keep


def flops_of(name, a):
    """useful floating-point operations of one launch from its arguments (the entry's argument order, include/gptst_hip.h)"""
    if name == "gptst_mtgnn_tapgemm":                # a (row, tap) pair counts where the tap lies inside the source frame
        ci, ntap, offs, co, gated, b, tsrc, tdst, n = a[2], a[4], a[5], a[14], a[17], a[18], a[19], a[20], a[21]
        pairs = sum(1 for to in range(tdst) for j in range(ntap) if 0 <= to + offs[j] < tsrc)
        return 2.0 * b * n * pairs * ci * co * (2 if gated else 1)
    if name == "gptst_mtgnn_wgrad":
        cw, ci, ntap, b, tdst, n = a[1], a[4], a[6], a[11], a[13], a[14]
        return 2.0 * b * tdst * n * cw * ntap * ci
    if name == "gptst_mtgnn_graphgrad":
        c, ks, units, n = a[5], a[6], a[9], a[10]
        return 2.0 * units * ks * n * n * c
    if name == "gptst_stgcn_tapgemm":
        ci, ntap, co, rows = a[2], a[3], a[14], a[18]
        return 2.0 * rows * ntap * ci * co
    if name == "gptst_stgcn_wgrad":
        cw, ci, ntap, rows = a[1], a[4], a[5], a[13]
        return 2.0 * rows * cw * ntap * ci
    if name == "gptst_stgcn_nodemix":
        ks, c, units, n = a[2], a[6], a[8], a[9]
        return 2.0 * units * ks * n * n * c
    return 0.0                                     # gate_bwd, LayerNorm: a few operations per element, bound by their bytes


def per_kernel(m, x, w):
    """every launch of the HIP pass alone.  The same entry runs at several shapes in one pass (three layers), so a row is one (entry, shape, bytes)"""
    args_of, call = [], ops._call

    def recording(name, *args, tag="", nbytes=0):
        call(name, *args, tag=tag, nbytes=nbytes)
        args_of.append(args)
    ops.TIMER, ops._call = [], recording
    for _ in range(10):
        fb(m, x, w)
    torch.cuda.synchronize()
    acc, order = {}, []
    for (name, tag, e0, e1, nbytes), a in zip(ops.TIMER, args_of):
        key = (name, tag, nbytes)
        if key not in acc:
            order.append(key)
        acc.setdefault(key, []).append((e0.elapsed_time(e1) * 1e3, a))
    ops.TIMER, ops._call = None, call
    say("the launches of one HIP forward + backward (device events around each launch, 10 passes; us = median of a launch, n = launches per pass;")
    say("bound = max(flops / %.1f TFLOP/s, bytes / %.1f TB/s), bytes = every operand once).  Not listed: the torch ops of the path (the graph" % (PEAK_TFLOPS, PEAK_TBS))
    say("constructor, the weight packing, the pad, the head's two addmm, the sums of the partials):")
    say("  %-22s %-24s %2s %9s %9s %9s %9s %7s  %s" % ("entry", "shape", "n", "us", "GFLOP", "MB", "bound us", "share", "bound by"))
    total = 0.0
    for key in order:
        v = acc[key]
        us = statistics.median(t for t, _ in v)
        n = len(v) // 10
        total += us * n
        mb.kernel_row("  %-22s %-24s %2d %9.1f %9.2f %9.1f %9.1f %6.1f%%  %s", key[0], key[1], n, us, flops_of(key[0], v[0][1]), key[2])
    say("  sum of the launches above: %.1f us per pass" % total)


if __name__ == "__main__":
    if "--trace" in sys.argv:
        mb.trace(predictor, SHAPE, sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    say("MTGNN predictor at (B, T, N, C) = (%d, %d, %d, %d -> %d x 1), rows of layer 0 = %d, %s" % (B, T, N, C, T, B * 13 * N, torch.cuda.get_device_name(0)))
    mh, x, w, _ = mb.ab_predictor(predictor, SHAPE, compared=no_dropout, compared_note=" (no dropout)", mode_note="training mode, dropout 0.3, ")
    per_kernel(mh, x, w)
    del mh, x, w
    torch.cuda.empty_cache()
    mb.ab_step(step_predictor, SHAPE, "MTGNN", "mtgnn_backend")
    mb.write_out("mtgnn_hip_ab.txt")
