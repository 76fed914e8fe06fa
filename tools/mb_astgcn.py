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
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gptst_amd import graph, ops, synth                          # noqa: E402
from gptst_amd.config import make_args, predictor_args           # noqa: E402
from gptst_amd.enhance import xavier_downstream_                 # noqa: E402
from gptst_amd.predictors import ASTGCN, astgcn_hip              # noqa: E402

dev = torch.device("cuda:0")
B, T, N, C = 64, 12, 170, 64
PEAK_TFLOPS, PEAK_TBS = 157.3, 8.0               # fp32 MFMA, HBM3E
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


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


def verdict(res):
    """faster only where the one's slowest round lies below the other's fastest"""
    h, t = res["hip"], res["torch"]
    return "hip faster" if max(h) < min(t) else ("hip slower" if min(h) > max(t) else "no difference outside the spread")


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
        for _ in range(3):
            fb(m, x, w)

    def fwd(m):
        with torch.no_grad():
            m(x)
    tf, tb = {k: [] for k in ms}, {k: [] for k in ms}
    for _ in range(7):
        for k, m in ms.items():
            tb[k].append(events(lambda: fb(m, x, w), 5))
            tf[k].append(events(lambda: fwd(m), 5))
    say("predictor, device events, 7 alternating rounds of 5 passes, ms median (min - max):")
    for k in ms:
        say("  %-5s forward + backward %s   forward only (no_grad) %s" % (k, med(tb[k]), med(tf[k])))
    say("  forward + backward: %s;  forward only: %s" % (verdict(tb), verdict(tf)))
    return ms["hip"], x, w, statistics.median(tb["hip"])


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
    ops.TIMER = []
    for _ in range(5):
        fb(m, x, w)
    torch.cuda.synchronize()
    acc, order = {}, []
    for name, tag, e0, e1, nbytes in ops.TIMER:
        if (name, tag) not in acc:
            order.append((name, tag))
        acc.setdefault((name, tag), []).append((e0.elapsed_time(e1) * 1e3, nbytes))
    ops.TIMER = None
    say("the launches of one HIP forward + backward (device events around each launch, 5 passes; us = median of a launch, n = launches per pass;")
    say("bound = max(flops / %.1f TFLOP/s, bytes / %.1f TB/s), bytes = every operand once):" % (PEAK_TFLOPS, PEAK_TBS))
    say("  %-26s %-22s %2s %9s %9s %9s %9s %7s  %s" % ("entry", "shape", "n", "us", "GFLOP", "MB", "bound us", "share", "bound by"))
    total = 0.0
    for key in order:
        v = acc[key]
        us = statistics.median(t for t, _ in v)
        n = len(v) // 5
        fl, by = flops_of(key[0], ops.LAST_CALL[key]), v[0][1]
        tf, tb = fl / PEAK_TFLOPS / 1e6, by / PEAK_TBS / 1e6
        bound = max(tf, tb)
        total += us * n
        say("  %-26s %-22s %2d %9.1f %9.2f %9.1f %9.1f %6.1f%%  %s" % (key[0][6:], key[1], n, us, fl / 1e9, by / 1e6, bound, 100 * bound / us,
                                                                    "MFMA" if tf >= tb else "HBM"))
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


def ab_step():
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    from oracle import gptst_oracle as O
    import logging
    say("EvalTrainer loop body (zero_grad, forward, masked MAE, backward, clip, Adam), host clock around 10 steps ending in a synchronise,")
    say("5 alternating rounds after 3 warm-up steps, ms per step median (min - max):")
    for finetune in (False, True):
        runs = {}
        for backend in ("torch", "hip"):
            args = make_args("PEMS08", mode="eval", num_nodes=N, scaler_zeros=synth.scaler_zeros(), log_dir="/tmp", debug=True, model="ASTGCN_test",
                             astgcn_backend=backend, batch_size=B)
            model = EnhanceFrontEnd(args, predictor=predictor(backend), finetune_encoder=finetune).to(dev)
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
            for _ in range(3):
                step(model, tr)
        torch.cuda.synchronize()
        for _ in range(5):
            for k, (model, tr) in runs.items():
                t0 = time.perf_counter()
                for _ in range(10):
                    step(model, tr)
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) * 1e3 / 10)
        for k in runs:
            assert runs[k][0].predictor.backend_used == k
            say("  %-10s %-5s %s" % ("fine-tuned" if finetune else "frozen", k, med(res[k])))
        say("  %-10s %s" % ("", verdict(res)))
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if "--trace" in sys.argv:
        trace(sys.argv[sys.argv.index("--trace") + 1])
        sys.exit(0)
    say("ASTGCN predictor at (B, T, N, C) = (%d, %d, %d, %d -> %d x 1), 2 blocks, K 3, rows = %d, %s" % (B, T, N, C, T, B * T * N, torch.cuda.get_device_name(0)))
    mh, x, w, pass_ms = ab_predictor()
    per_kernel(mh, x, w, pass_ms)
    del mh, x, w
    torch.cuda.empty_cache()
    ab_step()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "astgcn_hip_ab.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(LINES) + "\n")
