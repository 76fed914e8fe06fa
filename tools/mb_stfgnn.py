#!/usr/bin/env python
"""The downstream STFGNN predictor at the shapes of its confs — (B, T, N, C) = (64, 12, 170, 64), three layers of [64, 64, 64] (PEMS08), and
(64, 12, 266, 64), one layer (NYC_TAXI, two output channels): the HIP backend (csrc/stfgnn.hip, the window kernels of csrc/stsgcn.hip on groups
of 4N rows, the gated tap GEMM of csrc/mtgnn.hip, the tap GEMM of csrc/stgcn.hip for the first embedding) against the torch backend of the same
module, on the same GPU, in the same call.
usage (GPU box, repo root):
    python tools/mb_stfgnn.py                     per shape: predictor forward + backward and forward under no_grad, the two backends alternating,
                                                  device events, rounds after warm-up; the peak memory of a forward + backward of each backend;
                                                  the launches of the HIP pass with the flops / bytes of their shapes — each launch for the one-layer
                                                  shape, summed by entry for the three-layer one; the heads, kept in torch, timed alone; the
                                                  EvalTrainer loop body at the first shape; [--out FILE] (default profiles/stfgnn_hip_ab.txt)
    python tools/mb_stfgnn.py --trace torch|hip   30 forward + backward passes of one backend at the first shape and nothing else"""
import sys

import torch

import mb_downstream as mb
import mb_stsgcn as ss
from mb_downstream import dev, say
from gptst_amd import graph, ops
from gptst_amd.config import predictor_args

from gptst_amd.predictors import STFGNN

SHAPES = [("PEMS08", (64, 12, 170, 64)), ("NYC_TAXI", (64, 12, 266, 64))]


def fusion(n):
    """a fusion graph of two sensor-like graphs with rows normalised to sum 1 (raw 0/1 graphs grow the activations layer by layer); the
    temporal one symmetric with a unit diagonal, as graph.dtw_graph gives it"""
    s = ss.row_normalised(n)
    d = graph.synthetic_adjacency(n, 5)
    d = ((d + d.T) > 0).astype("float32")
    d = d / d.sum(1, keepdims=True)
    d[range(n), range(n)] = 1.0
    return graph.stfgnn_fusion_graph(s, d)


def make_predictor(ds):
    def predictor(backend):
        p = predictor_args(ds, "STFGNN")
        p.adj = fusion(p.num_nodes)
        torch.manual_seed(0)
        m = STFGNN(p, dev, 64, backend=backend)
        with torch.no_grad():                                        # position embeddings of the size they have after training
            for k, q in m.named_parameters():
                if k.endswith("_embedding"):
                    q.normal_(0, 0.3)
        return m.train()
    return predictor


_stsgcn_flops_of = ss.flops_of


def flops_of(name, a):
    """useful floating-point operations of one launch from its arguments (the entry's argument order, include/gptst_hip.h)"""
    if name == "gptst_stfgnn_mix":
        c, mode, b, t, n = a[5], a[6], a[7], a[8], a[9]
        w = t - 3
        units = b * (t - 2 + w) if mode == ops.MIX_F2E else b * t * 2 if mode == ops.MIX_E2F else b * w * (3 if mode == ops.MIX_E2E else 1)
        return 2.0 * units * n * n * c
    if name == "gptst_mtgnn_tapgemm":
        ci, ntap, co, gated, b, tdst, n = a[2], a[4], a[14], a[17], a[18], a[20], a[21]
        return 2.0 * b * tdst * n * ntap * ci * co * (2 if gated else 1)
    if name == "gptst_mtgnn_wgrad":
        cw, ci, ntap, b, tdst, n = a[1], a[4], a[6], a[11], a[13], a[14]
        return 2.0 * b * tdst * n * cw * ntap * ci
    return _stsgcn_flops_of(name, a)


if __name__ == "__main__":
    if "--trace" in sys.argv:
        mb.trace(make_predictor("PEMS08"), SHAPES[0][1], sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    ss.flops_of = flops_of                                           # by_entry looks it up in its module
    for i, (ds, shape) in enumerate(SHAPES):
        B, T, N, C = shape
        predictor = make_predictor(ds)
        layers = len(predictor_args(ds, "STFGNN").hidden_dims)
        say("STFGNN predictor (%s conf) at (B, T, N, C) = (%d, %d, %d, %d), %d layer(s) of [64, 64, 64], %s" % (ds, B, T, N, C, layers, torch.cuda.get_device_name(0)))
        mh, x, w, pass_ms = mb.ab_predictor(predictor, shape, warm=3, reps=5)
        if layers == 1:
            total = mb.per_kernel(mh, x, w, flops_of, passes=5)
        else:
            total = ss.by_entry(mh, x, w)
        say("  sum of the launches above: %.1f us per pass = %.1f%% of the %.3f ms pass" % (total, total / 10 / pass_ms, pass_ms))
        ss.heads(mh, shape, T - 3 * layers, pass_ms)
        del mh, x, w
        torch.cuda.empty_cache()
        ss.peak_memory(predictor, shape)
        if i == 0:
            mb.ab_step(lambda backend, args: predictor(backend), shape, "STFGNN", "stfgnn_backend", warm=3, steps=10)
        say()
    mb.write_out("stfgnn_hip_ab.txt")
