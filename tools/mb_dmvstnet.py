#!/usr/bin/env python
"""The downstream DMVSTNET predictor at the shapes of its two confs — (B, T, N, C) = (64, 12, 266, 64) (NYC_TAXI) and (64, 12, 250, 64)
(NYC_BIKE): hidden_dim 64, so a one-layer LSTM of width 128 over B N rows and 12 steps: the HIP backend (csrc/dmvstnet.hip: the semantic
view as a per-node thin projection; csrc/stmgcn.hip: the LSTM in one launch forward and one backward; the hoisted kernels of
csrc/stgcn.hip) against the torch backend of the same module — ``nn.LSTM``, MIOpen's through PyTorch-ROCm — on the same GPU, in the same
call.  The two LSTM matrices are multiplied by 3 first, as in the tests.
usage (GPU box, repo root):
    python tools/mb_dmvstnet.py                  per shape: predictor forward + backward and forward under no_grad, torch and HIP alternating
                                                 (device events, 7 rounds of 5 passes after warm-up); the launches of the HIP pass summed by
                                                 entry; the HIP backend with one and with two row tiles per LSTM workgroup, alternating; the
                                                 peak memory of a forward + backward of each backend;  [--out FILE] (default
                                                 profiles/dmvstnet_hip_ab.txt)"""
import torch

import mb_downstream as mb
import mb_msdr as md
import mb_stsgcn as ss
from mb_downstream import dev, say
from gptst_amd import graph
from gptst_amd.config import predictor_args
from gptst_amd.predictors import DMVSTNET, dmvstnet_hip as DH

SHAPES = [("NYC_TAXI", (64, 12, 266, 64)), ("NYC_BIKE", (64, 12, 250, 64))]


def make_predictor(ds, C):
    def predictor(backend):
        p = predictor_args(ds, "DMVSTNET")
        p.adj_mx = torch.tensor(graph.synthetic_adjacency(p.num_nodes, 2))
        torch.manual_seed(0)
        m = DMVSTNET(p, dev, C, 2, backend=backend)
        with torch.no_grad():
            for w in m.lstm.parameters():
                if w.dim() == 2:
                    w.mul_(3.0)
        return m.train()
    return predictor


def one_against_two_tiles(m, x, w, reps=5):
    """the HIP backend with the LSTM's row tiles per workgroup forced to 1 and to 2 (dmvstnet_hip.row_tiles picks 1 at H = 128)"""
    def fwd():
        with torch.no_grad():
            m(x)
    tb, tf = {1: [], 2: []}, {1: [], 2: []}
    try:
        for t in tb:
            DH.TILES = t
            for _ in range(3):
                mb.fb(m, x, w)
        for _ in range(7):
            for t in tb:
                DH.TILES = t
                tb[t].append(mb.events(lambda: mb.fb(m, x, w), reps))
                tf[t].append(mb.events(fwd, reps))
    finally:
        DH.TILES = 0
    say("the HIP backend with 1 and with 2 row tiles per LSTM workgroup, 7 alternating rounds of %d passes, ms median (min - max):" % reps)
    for t in tb:
        say("  %d tile%s  forward + backward %s   forward only (no_grad) %s" % (t, " " if t == 1 else "s", mb.med(tb[t]), mb.med(tf[t])))


if __name__ == "__main__":
    for ds, shape in SHAPES:
        B, T, N, C = shape
        predictor = make_predictor(ds, C)
        pa = predictor_args(ds, "DMVSTNET")
        say("DMVSTNET predictor (%s conf) at (B, T, N, C) = (%d, %d, %d, %d): hidden_dim %d, a one-layer LSTM of width %d over %d rows and %d steps, %s"
            % (ds, B, T, N, C, pa.hidden_dim, 2 * pa.hidden_dim, B * N, T, torch.cuda.get_device_name(0)))
        mh, x, w, pass_ms = mb.ab_predictor(predictor, shape, warm=3, reps=5)
        total = md.by_entry(mh, x, w)
        say("  sum of the launches above: %.1f us per pass = %.1f%% of the %.3f ms pass" % (total, total / 10 / pass_ms, pass_ms))
        one_against_two_tiles(mh, x, w)
        del mh, x, w
        torch.cuda.empty_cache()
        ss.peak_memory(predictor, shape)
        say()
    mb.write_out("dmvstnet_hip_ab.txt")
