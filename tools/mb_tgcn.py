#!/usr/bin/env python
"""The downstream TGCN predictor at the TGCN conf's PEMS08 shape (B, T, N, C) = (64, 12, 170, 64 -> 12 x 1, rnn_units 100): the HIP backend
(csrc/tgcn.hip + the hoisted kernels of csrc/stgcn.hip) against the torch backend of the same module, on the same GPU, in the same call.
usage (GPU box, repo root):
    python tools/mb_tgcn.py                       predictor forward + backward and forward under no_grad, the two backends alternating, device events,
                                                  7 rounds after warm-up; each launch of the HIP pass with the flops / bytes of its shapes; the
                                                  EvalTrainer loop body, frozen and fine-tuned; [--out FILE] (default profiles/tgcn_hip_ab.txt)
    python tools/mb_tgcn.py --trace torch|hip     30 forward + backward passes of one backend and nothing else (for tools/prof.sh)"""
import sys
from types import SimpleNamespace

import torch

import mb_downstream as mb
from mb_downstream import dev, events, med, say
from gptst_amd import graph, ops
from gptst_amd.predictors import TGCN

B, T, N, C = SHAPE = 64, 12, 170, 64
HID = 100


def ap():
    return SimpleNamespace(num_nodes=N, input_window=T, output_window=T, rnn_units=HID, output_dim=1, G=graph.tgcn_graph(graph.synthetic_adjacency(N, 2)))


def predictor(backend):
    torch.manual_seed(0)
    return TGCN(ap(), dev, C, backend=backend).to(dev).train()


def step_predictor(backend, args):
    torch.manual_seed(0)
    return TGCN(ap(), dev, args.hidden_dim, backend=backend)


def ab_tiles():
    """the four step launches alone at this shape with 1 and with 2 node tiles per workgroup (what the library picks from B and N: 2 here)"""
    Hp, Np, S, rows = 16 * ((HID + 15) // 16), 16 * ((N + 15) // 16), B * N, B * T * N
    r = lambda *s: torch.randn(*s, device=dev)          # noqa: E731
    Lp = torch.zeros(Np, Np, device=dev)
    Lp[:N, :N] = graph.tgcn_graph(graph.synthetic_adjacency(N, 2)).to(dev)
    h, q, u, c, dh, part, out = r(S, Hp), r(S, Hp), torch.sigmoid(r(S, Hp)), torch.tanh(r(S, Hp)), r(S, Hp), r(S, Hp), r(S, Hp)
    g0, g1, d0, d1, W2, W1, W2t = r(rows, 2 * Hp), r(rows, Hp), r(rows, 2 * Hp), r(rows, Hp), r(2 * Hp, Hp) / 10, r(Hp, Hp) / 10, r(Hp, 2 * Hp) / 10
    Z = r(rows, C + Hp)
    runs = {"fwd_gates": lambda k: ops.tgcn_fwd_gates(Lp, W2, h, g0, 3, out, q, B, T, N, r=part, z=Z, zoff=C, tiles=k),
            "fwd_state": lambda k: ops.tgcn_fwd_state(Lp, W1, q, g1, 3, u, h, out, B, T, N, c=part, z=Z, zoff=C, tiles=k),
            "bwd_cand": lambda k: ops.tgcn_bwd_cand(Lp, W1, dh, u, c, u, h, 3, d1, d0, part, B, T, N, tiles=k),
            "bwd_state": lambda k: ops.tgcn_bwd_state(Lp, W2t, d0, part, 3, out, B, T, N, tiles=k)}
    say("the step launches alone, 1 against 2 node tiles per workgroup, device events, 5 alternating rounds of 50 launches, us median (min - max):")
    for name, fn in runs.items():
        res = {1: [], 2: []}
        for k in (1, 2):
            for _ in range(10):
                fn(k)
        for _ in range(5):
            for k in (1, 2):
                res[k].append(events(lambda: fn(k), 50) * 1e3)
        say("  %-10s tiles 1: %s   tiles 2: %s" % (name, med(res[1]), med(res[2])))


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
    # the step launches: mix 2 B N N K + GEMM 2 B N K NO
    pos = {"gptst_tgcn_fwd_gates": (11, 13, 14, 1, 2), "gptst_tgcn_fwd_state": (12, 14, 15, 1, 1), "gptst_tgcn_bwd_cand": (11, 13, 14, 1, 1),
           "gptst_tgcn_bwd_state": (6, 8, 9, 2, 1)}
    if name in pos:
        ib, inn, ih, k, no = pos[name]
        b, n, hp = a[ib], a[inn], a[ih]
        return 2.0 * b * n * (k * hp) * (n + no * hp)
    return 0.0


if __name__ == "__main__":
    if "--trace" in sys.argv:
        mb.trace(predictor, SHAPE, sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    say("TGCN predictor at (B, T, N, C) = (%d, %d, %d, %d -> %d x 1), rnn_units %d, rows = %d, %s" % (B, T, N, C, T, HID, B * T * N, torch.cuda.get_device_name(0)))
    mh, x, w, _ = mb.ab_predictor(predictor, SHAPE)
    say("  sum of the launches above: %.1f us per pass" % mb.per_kernel(mh, x, w, flops_of))
    ab_tiles()
    del mh, x, w
    torch.cuda.empty_cache()
    mb.ab_step(step_predictor, SHAPE, "TGCN", "tgcn_backend")
    mb.write_out("tgcn_hip_ab.txt")
