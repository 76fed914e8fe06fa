#!/usr/bin/env python
"""The downstream TGCN predictor at the TGCN conf's PEMS08 shape (B, T, N, C) = (64, 12, 170, 64 -> 12 x 1, rnn_units 100): the HIP backend
(csrc/tgcn.hip + the hoisted kernels of csrc/stgcn.hip) against the torch backend of the same module, on the same GPU, in the same call.
usage (GPU box, repo root):
    python tools/mb_tgcn.py                       predictor forward + backward and forward under no_grad, the two backends alternating, device events,
                                                  7 rounds after warm-up; each launch of the HIP pass with the flops / bytes of its shapes; the
                                                  EvalTrainer loop body, frozen and fine-tuned; [--out FILE] (default profiles/tgcn_hip_ab.txt)
    python tools/mb_tgcn.py --trace torch|hip     30 forward + backward passes of one backend and nothing else (for tools/prof.sh)"""
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gptst_amd import graph, ops, synth          # noqa: E402
from gptst_amd.config import make_args           # noqa: E402
from gptst_amd.predictors import TGCN            # noqa: E402

dev = torch.device("cuda:0")
B, T, N, C, HID = 64, 12, 170, 64, 100
PEAK_TFLOPS, PEAK_TBS = 157.3, 8.0               # fp32 MFMA, HBM3E
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def ap():
    return SimpleNamespace(num_nodes=N, input_window=T, output_window=T, rnn_units=HID, output_dim=1, G=graph.tgcn_graph(graph.synthetic_adjacency(N, 2)))


def predictor(backend):
    torch.manual_seed(0)
    return TGCN(ap(), dev, C, backend=backend).to(dev).train()


def fb(m, x, w):
    for p in m.parameters():
        p.grad = None
    (m(x) * w).sum().backward()


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def med(v):
    return "%.3f (%.3f - %.3f)" % (statistics.median(v), min(v), max(v))


def trace(backend):
    m = predictor(backend)
    x, w = torch.randn(B, T, N, C, device=dev, requires_grad=True), torch.randn(B, T, N, 1, device=dev)
    for _ in range(30):
        fb(m, x, w)
    torch.cuda.synchronize()


def ab_predictor():
    ms = {k: predictor(k) for k in ("torch", "hip")}
    ms["hip"].load_state_dict(ms["torch"].state_dict(), strict=True)
    x, w = torch.randn(B, T, N, C, device=dev, requires_grad=True), torch.randn(B, T, N, 1, device=dev)
    y = {k: m(x).detach() for k, m in ms.items()}
    say("outputs of the two backends at this shape: max |diff| %.2e of max |y| %.2e" % (float((y["hip"] - y["torch"]).abs().max()), float(y["torch"].abs().max())))
    assert ms["hip"].backend_used == "hip"
    for m in ms.values():
        for _ in range(5):
            fb(m, x, w)

    def fwd(m):
        with torch.no_grad():
            m(x)
    tf, tb = {k: [] for k in ms}, {k: [] for k in ms}
    for _ in range(7):
        for k, m in ms.items():
            tb[k].append(events(lambda: fb(m, x, w), 20))
            tf[k].append(events(lambda: fwd(m), 20))
    say("predictor, device events, 7 alternating rounds of 20 passes, ms median (min - max):")
    for k in ms:
        say("  %-5s forward + backward %s   forward only (no_grad) %s" % (k, med(tb[k]), med(tf[k])))
    say("  forward + backward: %s;  forward only: %s" % (verdict(tb), verdict(tf)))
    return ms["hip"], x, w


def verdict(res):
    """faster only where the one's slowest round lies below the other's fastest"""
    h, t = res["hip"], res["torch"]
    return "hip faster" if max(h) < min(t) else ("hip slower" if min(h) > max(t) else "no difference outside the spread")


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


def ab_step():
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    from oracle import gptst_oracle as O
    import logging
    say("EvalTrainer loop body (zero_grad, forward, masked MAE, backward, clip, Adam), host clock around 20 steps ending in a synchronise,")
    say("5 alternating rounds after 5 warm-up steps, ms per step median (min - max):")
    for finetune in (False, True):
        runs = {}
        for backend in ("torch", "hip"):
            args = make_args("PEMS08", mode="eval", num_nodes=N, scaler_zeros=synth.scaler_zeros(), log_dir="/tmp", debug=True, model="TGCN_test",
                             tgcn_backend=backend, batch_size=B)
            torch.manual_seed(0)
            model = EnhanceFrontEnd(args, predictor=TGCN(ap(), dev, args.hidden_dim, backend=backend), finetune_encoder=finetune).to(dev)
            model.load_pretrained_model(O.init_state_dict(args, 11))
            tr = EvalTrainer(model, args, None, None, None, synth.SCALER_MEAN, synth.SCALER_STD)
            tr.logger.setLevel(logging.WARNING)
            runs[backend] = (model, tr)
        src = synth.make_batch(B, T, N, 1, interval=5, seed=21).to(dev)
        tgt = synth.make_batch(B, T, N, 1, interval=5, seed=22, start_slot=12).to(dev)

        def step(model, tr):
            tr.opt.zero_grad()
            loss = tr._loss(model(src, tgt)[0], tgt)
            loss.backward()
            torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.requires_grad], tr.args.max_grad_norm)
            tr.opt.step()
        res = {k: [] for k in runs}
        for k, (model, tr) in runs.items():
            model.train()
            for _ in range(5):
                step(model, tr)
        torch.cuda.synchronize()
        for _ in range(5):
            for k, (model, tr) in runs.items():
                t0 = time.perf_counter()
                for _ in range(20):
                    step(model, tr)
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) * 1e3 / 20)
        for k in runs:
            assert runs[k][0].predictor.backend_used == k
            say("  %-10s %-5s %s" % ("fine-tuned" if finetune else "frozen", k, med(res[k])))
        say("  %-10s %s" % ("", verdict(res)))
        del runs
        torch.cuda.empty_cache()


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


def per_kernel(m, x, w):
    ops.TIMER = []
    for _ in range(10):
        fb(m, x, w)
    torch.cuda.synchronize()
    acc, order = {}, []
    for name, tag, e0, e1, nbytes in ops.TIMER:
        if (name, tag) not in acc:
            order.append((name, tag))
        acc.setdefault((name, tag), []).append((e0.elapsed_time(e1) * 1e3, nbytes))
    ops.TIMER = None
    say("the launches of one HIP forward + backward (device events around each launch, 10 passes; us = median of a launch, n = launches per pass;")
    say("bound = max(flops / %.1f TFLOP/s, bytes / %.1f TB/s), bytes = every operand once):" % (PEAK_TFLOPS, PEAK_TBS))
    say("  %-26s %-22s %2s %9s %9s %9s %9s %7s  %s" % ("entry", "shape", "n", "us", "GFLOP", "MB", "bound us", "share", "bound by"))
    total = 0.0
    for key in order:
        v = acc[key]
        us = statistics.median(t for t, _ in v)
        n = len(v) // 10
        fl, by = flops_of(key[0], ops.LAST_CALL[key]), v[0][1]
        tf, tb = fl / PEAK_TFLOPS / 1e6, by / PEAK_TBS / 1e6
        bound = max(tf, tb)
        total += us * n
        say("  %-26s %-22s %2d %9.1f %9.2f %9.1f %9.1f %6.1f%%  %s" % (key[0][6:], key[1], n, us, fl / 1e9, by / 1e6, bound, 100 * bound / us,
                                                                    "MFMA" if tf >= tb else "HBM"))
    say("  sum of the launches above: %.1f us per pass" % total)


if __name__ == "__main__":
    if "--trace" in sys.argv:
        trace(sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    say("TGCN predictor at (B, T, N, C) = (%d, %d, %d, %d -> %d x 1), rnn_units %d, rows = %d, %s" % (B, T, N, C, T, HID, B * T * N, torch.cuda.get_device_name(0)))
    mh, x, w = ab_predictor()
    per_kernel(mh, x, w)
    ab_tiles()
    del mh, x, w
    torch.cuda.empty_cache()
    ab_step()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "tgcn_hip_ab.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(LINES) + "\n")
