#!/usr/bin/env python
"""The downstream STGODE predictor at the shapes of its confs — (B, T, N, C) = (64, 12, 170, 64) (PEMS08) and (64, 12, 266, 64) (NYC_TAXI, two
output channels), n_layers = 3: 12 blocks of BN_nodes(relu(step(relu(X)))) and the max over the six branches: the HIP backend (csrc/stgode.hip)
against the torch backend of the same module — the reference's own operations through PyTorch-ROCm — on the same GPU, in the same call.
usage (GPU box, repo root):
    python tools/mb_stgode.py                     per shape: predictor forward + backward and forward under no_grad, the two backends alternating,
                                                  device events, rounds after warm-up; the peak memory of a forward + backward of each backend;
                                                  the launches of the HIP pass summed by entry with the flops / bytes of their shapes; the
                                                  heads, kept in torch, timed alone; the EvalTrainer loop body at the first shape;
                                                  [--out FILE] (default profiles/stgode_hip_ab.txt)
    python tools/mb_stgode.py --trace torch|hip   30 forward + backward passes of one backend at the first shape and nothing else"""
import sys

import torch

import mb_downstream as mb
import mb_stsgcn as ss
from mb_downstream import dev, say
from gptst_amd import graph
from gptst_amd.config import make_args, predictor_args
from gptst_amd.enhance import xavier_downstream_

from gptst_amd.predictors import STGODE

SHAPES = [("PEMS08", (64, 12, 170, 64)), ("NYC_TAXI", (64, 12, 266, 64))]


def graphs(n):
    """two sensor-like graphs in the reference's normalisation 0.4 (I + D^-1/2 A D^-1/2); the semantic one symmetric, as the DTW graph is"""
    s = graph.synthetic_adjacency(n, 2)
    d = graph.synthetic_adjacency(n, 5)
    return graph.stgode_normalized_adj(s), graph.stgode_normalized_adj(((d + d.T) > 0).astype("float32"))


def make_predictor(ds):
    def predictor(backend):
        p = predictor_args(ds, "STGODE")
        p.A_sp_wave, p.A_se_wave = graphs(p.num_nodes)
        torch.manual_seed(0)
        m = STGODE(p, dev, 64, make_args(ds).output_dim, backend=backend)
        return xavier_downstream_(m).train()                         # the confs' xavier = True: without it the branches of a graph tie exactly
    return predictor


def flops_of(name, a):
    """useful floating-point operations of one launch from its arguments (the entry's argument order, include/gptst_hip.h)"""
    if name == "gptst_stgode_step":
        c, b, t, n = a[16], a[17], a[18], a[19]
        return 2.0 * b * t * n * c * (n + c + t)
    if name == "gptst_stgode_wgrad":
        return 2.0 * a[5] * a[2] * a[2]
    if name == "gptst_stgode_reduce":
        c, b, t, n = a[5], a[6], a[7], a[8]
        return 2.0 * b * n * c * t * (t + 1)
    if name == "gptst_stgode_bn_stats":
        return 4.0 * a[3] * a[4] * a[5] * a[6]
    if name == "gptst_stgode_bn_apply":
        return 3.0 * a[16] * a[17] * a[18] * a[19]
    if name == "gptst_stgode_bn_bwd":
        return 6.0 * a[13] * a[14] * a[15] * a[16]
    raise KeyError(name)


if __name__ == "__main__":
    if "--trace" in sys.argv:
        mb.trace(make_predictor("PEMS08"), SHAPES[0][1], sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    ss.flops_of = flops_of                                           # by_entry looks it up in its module
    for i, (ds, shape) in enumerate(SHAPES):
        B, T, N, C = shape
        predictor = make_predictor(ds)
        say("STGODE predictor (%s conf) at (B, T, N, C) = (%d, %d, %d, %d), n_layers = %d: 12 blocks, %s"
            % (ds, B, T, N, C, predictor_args(ds, "STGODE").n_layers, torch.cuda.get_device_name(0)))
        mh, x, w, pass_ms = mb.ab_predictor(predictor, shape, warm=3, reps=5)
        total = ss.by_entry(mh, x, w)
        say("  sum of the launches above: %.1f us per pass = %.1f%% of the %.3f ms pass" % (total, total / 10 / pass_ms, pass_ms))
        ss.heads(mh, shape, T, pass_ms)
        del mh, x, w
        torch.cuda.empty_cache()
        ss.peak_memory(predictor, shape)
        if i == 0:
            mb.ab_step(lambda backend, args: predictor(backend), shape, "STGODE", "stgode_backend", warm=3, steps=10)
        say()
    mb.write_out("stgode_hip_ab.txt")
