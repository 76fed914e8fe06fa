#!/usr/bin/env python
"""The downstream ASTGCN predictor at the ASTGCN conf's PEMS08 shape (B, T, N, C) = (64, 12, 170, 64 -> 12 x 1; 2 blocks, K 3, widths 64): the HIP
backend (csrc/astgcn.hip + the tap GEMM, gate backward and weight gradient of csrc/stgcn.hip) against the torch backend of the same module, on
the same GPU, in the same call.
usage (GPU box, repo root):
    python tools/mb_astgcn.py                     predictor forward + backward and forward under no_grad, the two backends alternating, device events,
                                                  7 rounds after warm-up; each launch of the HIP pass with the flops / bytes of its shapes; what
                                                  stays in torch (the score chains, final_conv) timed alone; the EvalTrainer loop body, frozen and
                                                  fine-tuned; [--out FILE] (default profiles/astgcn_hip_ab.txt)
    python tools/mb_astgcn.py --trace torch|hip   30 forward + backward passes of one backend and nothing else (for tools/prof.sh)"""
import statistics
import sys

import torch

import mb_downstream as mb
from mb_downstream import dev, events, med, say
from gptst_amd import graph
from gptst_amd.config import predictor_args
from gptst_amd.enhance import xavier_downstream_
from gptst_amd.predictors import ASTGCN, astgcn_hip

B, T, N, C = SHAPE = 64, 12, 170, 64


def ap():
    p = predictor_args("PEMS08", "ASTGCN")
    p.G = graph.astgcn_graph(graph.synthetic_adjacency(N, 2), p.K)
    return p


def predictor(backend):
    torch.manual_seed(0)
    m = ASTGCN(ap(), dev, C, 1, backend=backend)
    xavier_downstream_(m)                                        # the conf's xavier pass: the model has no other initial state
    with torch.no_grad():                                        # and the score vectors centred, so that the sigmoids pass gradient
        for blk in m.BlockList:
            for p in (blk.TAt.U1, blk.TAt.U3, blk.SAt.W1, blk.SAt.W3):
                p.copy_(0.25 * (p - 0.5))
    return m.train()


def flops_of(name, a):
    """useful floating-point operations of one launch from its arguments (the entry's argument order, include/gptst_hip.h)"""
    if name == "gptst_stgcn_tapgemm":
        ci, ntap, co, rows = a[2], a[3], a[14], a[18]
        return 2.0 * rows * ntap * ci * co
    if name == "gptst_stgcn_wgrad":
        cw, ci, ntap, rows = a[1], a[4], a[5], a[13]
        return 2.0 * rows * cw * ntap * ci
    if name == "gptst_astgcn_attmix":
        ks, c, b, t, n = a[2], a[7], a[9], a[10], a[11]
        return 2.0 * b * t * ks * n * n * c
    if name == "gptst_astgcn_attgrad":
        ks, c, b, t, n = a[2], a[6], a[7], a[8], a[9]
        return 2.0 * b * t * ks * n * n * c
    return 0.0


def per_kernel(m, x, w, pass_ms):
    total = mb.per_kernel(m, x, w, flops_of, passes=5)
    say("  sum of the launches above: %.1f us per pass = %.1f%% of the %.3f ms pass" % (total, total / 10 / pass_ms, pass_ms))
    # what stays in torch, alone: the score chains of both blocks and the head, forward + backward, on inputs of the pass's shapes
    h = torch.randn(B, T, N, 64, device=dev, requires_grad=True)

    def chains():
        h.grad = None
        sum(astgcn_hip.attention(blk, h).square().sum() for blk in m.BlockList).backward()

    def head():
        h.grad = None
        astgcn_hip.head(m, h).square().sum().backward()
    for f in (chains, head):
        for _ in range(3):
            f()
    tc, th = [events(chains, 5) for _ in range(5)], [events(head, 5) for _ in range(5)]
    say("kept in torch, timed alone (forward + backward, device events, 5 rounds of 5), ms median (min - max):")
    say("  the score chains of both blocks %s = %.1f%% of the pass;  final_conv %s = %.1f%%"
        % (med(tc), 100 * statistics.median(tc) / pass_ms, med(th), 100 * statistics.median(th) / pass_ms))


if __name__ == "__main__":
    if "--trace" in sys.argv:
        mb.trace(predictor, SHAPE, sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    say("ASTGCN predictor at (B, T, N, C) = (%d, %d, %d, %d -> %d x 1), 2 blocks, K 3, rows = %d, %s" % (B, T, N, C, T, B * T * N, torch.cuda.get_device_name(0)))
    mh, x, w, pass_ms = mb.ab_predictor(predictor, SHAPE, warm=3, reps=5)
    per_kernel(mh, x, w, pass_ms)
    del mh, x, w
    torch.cuda.empty_cache()
    mb.ab_step(lambda backend, args: predictor(backend), SHAPE, "ASTGCN", "astgcn_backend", warm=3, steps=10)
    mb.write_out("astgcn_hip_ab.txt")
