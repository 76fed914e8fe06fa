#!/usr/bin/env python
"""The downstream STGCN predictor at the STGCN conf's PEMS08 shape (B, T, N, C) = (64, 12, 170, 64 -> 1): the HIP backend (csrc/stgcn.hip) against
the torch modules.  usage (GPU box, repo root):
    python tools/mb_stgcn.py                      predictor forward + backward and the EvalTrainer loop body, the two backends alternating; then
                                                  each new kernel's time with the flops / bytes of its shapes; [--out FILE] (default profiles/stgcn_hip_ab.txt)
    python tools/mb_stgcn.py --trace torch|hip    30 forward + backward passes of one backend and nothing else (for tools/prof.sh)"""
import sys
from types import SimpleNamespace

import torch

import mb_downstream as mb
from mb_downstream import dev, say
from gptst_amd import graph, ops
from gptst_amd.predictors import STGCN

B, T, N, C = SHAPE = 64, 12, 170, 64


def ap():
    return SimpleNamespace(Ks=3, Kt=3, num_nodes=N, G=graph.stgcn_graph(graph.synthetic_adjacency(N, 2)), blocks1=[64, 32, 128], drop_prob=0, outputl_ks=3)


def predictor(backend):
    torch.manual_seed(0)
    return STGCN(ap(), dev, C, 1, backend=backend).to(dev).train()


def step_predictor(backend, args):
    torch.manual_seed(0)
    return STGCN(ap(), dev, args.hidden_dim, args.output_dim, backend=backend)


def flops_of(name, a):
    """useful floating-point operations of one launch from its arguments (the entry's argument order, include/gptst_hip.h)"""
    if name == "gptst_stgcn_tapgemm":
        ci, ntap, co, act, rows = a[2], a[3], a[14], a[17], a[18]
        return 2.0 * rows * ntap * ci * co * (2 if act == ops.ACT_GLU else 1)
    if name == "gptst_stgcn_wgrad":
        cw, ci, ntap, rows = a[1], a[4], a[5], a[13]
        return 2.0 * rows * cw * ntap * ci
    if name == "gptst_stgcn_nodemix":
        ks, c, units, n = a[2], a[6], a[8], a[9]
        return 2.0 * units * ks * n * n * c
    return 0.0


if __name__ == "__main__":
    if "--trace" in sys.argv:
        mb.trace(predictor, SHAPE, sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    say("STGCN predictor at (B, T, N, C) = (%d, %d, %d, %d -> 1), rows = %d, %s" % (B, T, N, C, B * T * N, torch.cuda.get_device_name(0)))
    mh, x, w, _ = mb.ab_predictor(predictor, SHAPE, verdicts=False)
    say("  sum of the launches above: %.1f us per pass" % mb.per_kernel(mh, x, w, flops_of, what="the new launches of one"))
    del mh, x, w
    torch.cuda.empty_cache()
    mb.ab_step(step_predictor, SHAPE, "STGCN", "stgcn_backend", verdicts=False)
    mb.write_out("stgcn_hip_ab.txt")
