#!/usr/bin/env python
"""The downstream ST-MGCN predictor at the shapes of its two confs — (B, T, N, C) = (64, 12, 266, 64) (NYC_TAXI) and (64, 12, 250, 128)
(NYC_BIKE, whose encoder is 128 wide): two branches of a three-layer LSTM of width 64 over B N rows and 12 steps: the HIP backend
(csrc/stmgcn.hip: one launch per branch forward, one backward, and the hoisted kernels of csrc/stgcn.hip) against the torch backend of the
same module — ``nn.LSTM``, MIOpen's through PyTorch-ROCm — on the same GPU, in the same call.  The 2-D LSTM weights are multiplied by 3 first,
as in the tests.
usage (GPU box, repo root):
    python tools/mb_stmgcn.py                    per shape: predictor forward + backward and forward under no_grad, the two backends alternating,
                                                 device events, 7 rounds of 5 passes after warm-up; the launches of the HIP pass summed by entry;
                                                 the peak memory of a forward + backward of each backend;  [--out FILE] (default
                                                 profiles/stmgcn_hip_ab.txt)
    python tools/mb_stmgcn.py --trace torch|hip  30 forward + backward passes of one backend at the first shape and nothing else"""
import sys

import torch

import mb_downstream as mb
import mb_msdr as md
import mb_stsgcn as ss
from mb_downstream import dev, say
from gptst_amd import graph
from gptst_amd.config import predictor_args

from gptst_amd.predictors import STMGCN

SHAPES = [("NYC_TAXI", (64, 12, 266, 64)), ("NYC_BIKE", (64, 12, 250, 128))]


def make_predictor(ds, C):
    def predictor(backend):
        p = predictor_args(ds, "STMGCN")
        A = graph.synthetic_adjacency(p.n_nodes, 2)
        series = torch.randn(400, p.n_nodes, generator=torch.Generator().manual_seed(1)).numpy()
        p.dis_graph, p.pcc_graph = graph.stmgcn_supports(A), graph.stmgcn_supports(graph.stmgcn_correlation(series))
        torch.manual_seed(0)
        m = STMGCN(p, dev, C, 2, backend=backend)
        with torch.no_grad():
            for r in m.rnn_list:
                for w in r.lstm.parameters():
                    if w.dim() == 2:
                        w.mul_(3.0)
        return m.train()
    return predictor


if __name__ == "__main__":
    if "--trace" in sys.argv:
        mb.trace(make_predictor(SHAPES[0][0], SHAPES[0][1][3]), SHAPES[0][1], sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    for ds, shape in SHAPES:
        B, T, N, C = shape
        predictor = make_predictor(ds, C)
        pa = predictor_args(ds, "STMGCN")
        say("STMGCN predictor (%s conf) at (B, T, N, C) = (%d, %d, %d, %d): 2 branches, %d LSTM layers of width %d over %d rows and %d steps, %s"
            % (ds, B, T, N, C, pa.lstm_num_layers, pa.lstm_hidden_dim, B * N, T, torch.cuda.get_device_name(0)))
        mh, x, w, pass_ms = mb.ab_predictor(predictor, shape, warm=3, reps=5)
        total = md.by_entry(mh, x, w)
        say("  sum of the launches above: %.1f us per pass = %.1f%% of the %.3f ms pass" % (total, total / 10 / pass_ms, pass_ms))
        del mh, x, w
        torch.cuda.empty_cache()
        ss.peak_memory(predictor, shape)
        say()
    mb.write_out("stmgcn_hip_ab.txt")
