"""What the micro-benchmarks of the four downstream predictors share (mb_stgcn.py, mb_tgcn.py, mb_mtgnn.py, mb_astgcn.py): the HIP backend
against the torch backend of the same module, on the same GPU, in the same call, the two alternating.  A tool hands over what is its own:
``predictor(backend)`` -> its module in train mode on the device (the class and its args factory), its shape (B, T, N, C), the model name and
the name of its ``*_backend`` option, its ``flops_of`` table."""
import contextlib
import logging
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gptst_amd import ops, synth                 # noqa: E402
from gptst_amd.config import make_args           # noqa: E402

dev = torch.device("cuda:0")
PEAK_TFLOPS, PEAK_TBS = 157.3, 8.0               # fp32 MFMA, HBM3E
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def write_out(default_name):
    """what ``say`` said -> the file after --out, or profiles/<default_name>"""
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", default_name)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(LINES) + "\n")


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


def inputs(shape):
    B, T, N, C = shape
    return torch.randn(B, T, N, C, device=dev, requires_grad=True), torch.randn(B, T, N, 1, device=dev)


def trace(predictor, shape, backend):
    """30 forward + backward passes of one backend and nothing else"""
    m = predictor(backend)
    x, w = inputs(shape)
    for _ in range(30):
        fb(m, x, w)
    torch.cuda.synchronize()


def ab_predictor(predictor, shape, warm=5, reps=20, verdicts=True, compared=contextlib.nullcontext, compared_note="", mode_note=""):
    """the two backends with one state, alternating: -> (the HIP module, x, w, its median forward + backward ms).  ``compared(ms)``: a context
    the outputs are compared in"""
    ms = {k: predictor(k) for k in ("torch", "hip")}
    ms["hip"].load_state_dict(ms["torch"].state_dict(), strict=True)
    x, w = inputs(shape)
    with compared(ms):
        y = {k: m(x).detach() for k, m in ms.items()}
    say("outputs of the two backends at this shape%s: max |diff| %.2e of max |y| %.2e"
        % (compared_note, float((y["hip"] - y["torch"]).abs().max()), float(y["torch"].abs().max())))
    assert ms["hip"].backend_used == "hip"
    for m in ms.values():
        for _ in range(warm):
            fb(m, x, w)

    def fwd(m):
        with torch.no_grad():
            m(x)
    tf, tb = {k: [] for k in ms}, {k: [] for k in ms}
    for _ in range(7):
        for k, m in ms.items():
            tb[k].append(events(lambda: fb(m, x, w), reps))
            tf[k].append(events(lambda: fwd(m), reps))
    say("predictor, %sdevice events, 7 alternating rounds of %d passes, ms median (min - max):" % (mode_note, reps))
    for k in ms:
        say("  %-5s forward + backward %s   forward only (no_grad) %s" % (k, med(tb[k]), med(tf[k])))
    if verdicts:
        say("  forward + backward: %s;  forward only: %s" % (verdict(tb), verdict(tf)))
    return ms["hip"], x, w, statistics.median(tb["hip"])


def ab_step(step_predictor, shape, model_name, option, warm=5, steps=20, verdicts=True):
    """the EvalTrainer loop body on either backend, frozen and fine-tuned encoder.  ``step_predictor(backend, args)`` -> the predictor"""
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    from oracle import gptst_oracle as O
    B, T, N, _ = shape
    say("EvalTrainer loop body (zero_grad, forward, masked MAE, backward, clip, Adam), host clock around %d steps ending in a synchronise," % steps)
    say("5 alternating rounds after %d warm-up steps, ms per step median (min - max):" % warm)
    for finetune in (False, True):
        runs = {}
        for backend in ("torch", "hip"):
            args = make_args("PEMS08", mode="eval", num_nodes=N, scaler_zeros=synth.scaler_zeros(), log_dir="/tmp", debug=True, model=model_name + "_test",
                             batch_size=B, **{option: backend})
            model = EnhanceFrontEnd(args, predictor=step_predictor(backend, args), finetune_encoder=finetune).to(dev)
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
            for _ in range(warm):
                step(model, tr)
        torch.cuda.synchronize()
        for _ in range(5):
            for k, (model, tr) in runs.items():
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(model, tr)
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) * 1e3 / steps)
        for k in runs:
            assert runs[k][0].predictor.backend_used == k
            say("  %-10s %-5s %s" % ("fine-tuned" if finetune else "frozen", k, med(res[k])))
        if verdicts:
            say("  %-10s %s" % ("", verdict(res)))
        del runs
        torch.cuda.empty_cache()


def kernel_row(fmt, entry, shape, n, us, fl, by):
    """one launch against its bound = max(flops / peak, bytes / peak)"""
    tf, tb = fl / PEAK_TFLOPS / 1e6, by / PEAK_TBS / 1e6
    bound = max(tf, tb)
    say(fmt % (entry[6:], shape, n, us, fl / 1e9, by / 1e6, bound, 100 * bound / us, "MFMA" if tf >= tb else "HBM"))


def per_kernel(m, x, w, flops_of, passes=10, what="the launches of one HIP"):
    """every (entry, tag) of the HIP pass alone, from ops.TIMER: -> the sum of their medians, us per pass"""
    ops.TIMER = []
    for _ in range(passes):
        fb(m, x, w)
    torch.cuda.synchronize()
    acc, order = {}, []
    for name, tag, e0, e1, nbytes in ops.TIMER:
        if (name, tag) not in acc:
            order.append((name, tag))
        acc.setdefault((name, tag), []).append((e0.elapsed_time(e1) * 1e3, nbytes))
    ops.TIMER = None
    say("%s forward + backward (device events around each launch, %d passes; us = median of a launch, n = launches per pass;" % (what, passes))
    say("bound = max(flops / %.1f TFLOP/s, bytes / %.1f TB/s), bytes = every operand once):" % (PEAK_TFLOPS, PEAK_TBS))
    say("  %-26s %-22s %2s %9s %9s %9s %9s %7s  %s" % ("entry", "shape", "n", "us", "GFLOP", "MB", "bound us", "share", "bound by"))
    total = 0.0
    for key in order:
        v = acc[key]
        us = statistics.median(t for t, _ in v)
        n = len(v) // passes
        total += us * n
        kernel_row("  %-26s %-22s %2d %9.1f %9.2f %9.1f %9.1f %6.1f%%  %s", key[0], key[1], n, us, flops_of(key[0], ops.LAST_CALL[key]), v[0][1])
    return total
