#!/usr/bin/env python
"""The downstream CCRNN predictor at the shapes of its two confs — (B, T, N, C) = (64, 12, 266, 64) (NYC_TAXI, one RNN layer) and
(64, 12, 250, 128) (NYC_BIKE, two RNN layers, whose encoder is 128 wide): a graph-GRU encoder and decoder of width 25 over 12 + 12 steps on a
learned graph, k_hop 3: the HIP backend (csrc/ccrnn.hip: two launches per cell step in each direction, and the hoisted kernels of
csrc/stgcn.hip and csrc/mtgnn.hip) against the torch backend of the same module on the same GPU, in the same call.  The graph-conv weights
are multiplied by 2 first, as in the tests.  No targets are passed: a teacher-forced step runs the same launches.
usage (GPU box, repo root):
    python tools/mb_ccrnn.py                    per shape: predictor forward + backward and forward under no_grad, the two backends alternating,
                                                device events, 7 rounds of 5 passes after warm-up; the launches of the HIP pass summed by entry;
                                                the peak memory of a forward + backward of each backend;  [--out FILE] (default
                                                profiles/ccrnn_hip_ab.txt)
    python tools/mb_ccrnn.py --trace torch|hip  30 forward + backward passes of one backend at the first shape and nothing else
    python tools/mb_ccrnn.py --slab             the four step launches alone at (B, N, Hp, k) = (64, 266, 32, 3): the decoder's slab as built
                                                ([h | input padded to 16], K = 192) against a slab of 32 columns (K = 128: what packing the
                                                input behind column 25 would cost at best), the fed-back input against a given one, and the
                                                backward's addmm_;  device events, 7 rounds of 50 launches, us median (min - max);  appended
                                                to the file after --out (default profiles/ccrnn_hip_ab.txt)"""
import sys

import torch

import mb_downstream as mb
import mb_msdr as md
import mb_stsgcn as ss
from mb_downstream import dev, say
from gptst_amd import graph
from gptst_amd.config import predictor_args

from gptst_amd.predictors import CCRNN

SHAPES = [("NYC_TAXI", (64, 12, 266, 64)), ("NYC_BIKE", (64, 12, 250, 128))]


def make_predictor(ds, C):
    def predictor(backend):
        p = predictor_args(ds, "CCRNN")
        series = torch.rand(400, p.num_nodes, 2, generator=torch.Generator().manual_seed(1)).numpy()
        p.support = torch.tensor(graph.ccrnn_support(series, p.hidden_size_data, p.normalized_category, 0), dtype=torch.float32)
        torch.manual_seed(0)
        m = CCRNN(p, dev, C, 2, backend=backend)
        with torch.no_grad():
            for k, w in m.named_parameters():
                if k.endswith("out.weight") and "graphconv" in k:
                    w.mul_(2.0)
        return m.train()
    return predictor


def slab_ab(B=64, N=266, Hp=32, k=3, T=12, t=5, reps=50):
    import os
    import statistics
    from gptst_amd import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)                       # noqa: E731
    Np, S, rows, M = 16 * ((N + 15) // 16), B * N, B * T * N, k + 1
    P = torch.zeros(k, Np, Np, device=dev)
    P[:, :N, :N] = rn(k, N, N) / N ** 0.5
    h, q, u, r, c, dh = rn(S, Hp), rn(S, Hp), torch.rand(S, Hp, device=dev), torch.rand(S, Hp, device=dev), torch.tanh(rn(S, Hp)), rn(S, Hp)
    o = lambda *s: torch.empty(*s, device=dev)                                 # noqa: E731
    dp1, dp0 = o(rows, Hp), rn(rows, 2 * Hp)
    cases = {}
    for Cp in (16, 0):
        Ks = Hp + Cp
        W0, W1, W1T, W0T = rn(2 * Hp, M * Ks), rn(Hp, M * Ks), rn(Ks, M * Hp), rn(Ks, M * 2 * Hp)
        inp, dinp = (rn(S, Cp), o(S, Cp)) if Cp else (None, None)
        z, tag = o(rows, M * Ks), "K = %d" % (M * Ks)
        cases["fwd gates, given input, " + tag] = lambda W0=W0, inp=inp, z=z: ops.ccrnn_fwd_gates(P, W0, h, rn_b0, t, o_u, o_q, B, T, N, inp=inp, r=o_r, z=z)
        cases["fwd state, " + tag] = lambda W1=W1, inp=inp, z=z: ops.ccrnn_fwd_state(P, W1, q, rn_b1, t, u, h, o_h, B, T, N, inp=inp, c=o_c, z=z)
        cases["bwd cand,  " + tag.replace("K", "NO = %d, K" % Ks).replace(str(M * Ks), str(M * Hp))] = \
            lambda W1T=W1T, dinp=dinp: ops.ccrnn_bwd_cand(P, W1T, dh, u, c, r, h, t, dp1, o_dp0, o_part, B, T, N, dh2=q, dinp=dinp)
        cases["bwd state, " + tag.replace("K", "NO = %d, K" % Ks).replace(str(M * Ks), str(M * 2 * Hp))] = \
            lambda W0T=W0T, dinp=dinp: ops.ccrnn_bwd_state(P, W0T, dp0, dh, t, o_h, B, T, N, dinp=dinp)
        if Cp:
            fb, io = (rn(S, Hp), rn(Cp, Hp), rn(Cp)), o(S, Cp)
            cases["fwd gates, fed-back input, " + tag] = lambda W0=W0, z=z, fb=fb, io=io: ops.ccrnn_fwd_gates(P, W0, h, rn_b0, t, o_u, o_q, B, T, N, fb=fb,
                                                                                                          inp_out=io, r=o_r, z=z)
            Wout, dtop, dz = rn(Cp, Hp), rn(S, Hp), torch.zeros(S, Cp, device=dev)
            cases["the backward's addmm_ (B N, 16) x (16, Hp)"] = lambda dz=dz, Wout=Wout, dtop=dtop: dtop.addmm_(dz, Wout)
    rn_b0, rn_b1, o_u, o_q, o_r, o_h, o_c, o_dp0, o_part = rn(2 * Hp), rn(Hp), o(S, Hp), o(S, Hp), o(S, Hp), o(S, Hp), o(S, Hp), o(rows, 2 * Hp), o(S, Hp)
    for f in cases.values():
        for _ in range(5):
            f()
    res = {k_: [] for k_ in cases}
    for _ in range(7):
        for k_, f in cases.items():
            res[k_].append(mb.events(f, reps) * 1e3)
    say("CCRNN step launches alone at (B, N, Hp, k) = (%d, %d, %d, %d), %s: device events, 7 alternating rounds of %d launches, us median (min - max)"
        % (B, N, Hp, k, torch.cuda.get_device_name(0), reps))
    for k_, v in res.items():
        say("  %-48s %8.2f (%.2f - %.2f)" % (k_, statistics.median(v), min(v), max(v)))
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(mb.ROOT, "profiles", "ccrnn_hip_ab.txt")
    open(out, "a").write("\n".join(mb.LINES) + "\n")


if __name__ == "__main__":
    if "--slab" in sys.argv:
        slab_ab()
        sys.exit(0)
    if "--trace" in sys.argv:
        mb.trace(make_predictor(SHAPES[0][0], SHAPES[0][1][3]), SHAPES[0][1], sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    for ds, shape in SHAPES:
        B, T, N, C = shape
        predictor = make_predictor(ds, C)
        pa = predictor_args(ds, "CCRNN")
        say("CCRNN predictor (%s conf) at (B, T, N, C) = (%d, %d, %d, %d): %d RNN layer(s) of width %d, k_hop %d, %d + %d steps, %s"
            % (ds, B, T, N, C, pa.n_rnn_layers, pa.hidden_size, pa.k_hop, T, pa.num_predict, torch.cuda.get_device_name(0)))
        mh, x, w, pass_ms = mb.ab_predictor(predictor, shape, warm=3, reps=5)
        total = md.by_entry(mh, x, w)
        say("  sum of the launches above: %.1f us per pass = %.1f%% of the %.3f ms pass" % (total, total / 10 / pass_ms, pass_ms))
        del mh, x, w
        torch.cuda.empty_cache()
        ss.peak_memory(predictor, shape)
        say()
    mb.write_out("ccrnn_hip_ab.txt")
