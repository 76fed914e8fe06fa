#!/usr/bin/env python
"""Two builds of the library against each other on the two recurrences (csrc/tgcn.hip, csrc/msdr.hip), their processes alternating on one GPU:
the protocol of profiles/downstream_rowgemm_ab.txt.  The library is chosen with GPTST_LIB; the timing is the tools' own (mb_downstream.ab_predictor,
mb_tgcn.ab_tiles, device events around each launch through ops.TIMER).
usage (GPU box, repo root):
    GPTST_LIB=... python tools/ab_recurrence.py --measure OUT.json [tgcn] [msdr] [tiles]     one process: the lines below (default: these three) ->
                                                                        {line: [median, min, max]}
    GPTST_LIB=... python tools/ab_recurrence.py --measure OUT.json stsgcn stfgnn             the same for the two window predictors (csrc/stsgcn.hip,
                                                                        csrc/stfgnn.hip, win_mix_dev.h) at mb_stsgcn.py's / mb_stfgnn.py's two shapes
                                                                        each; in-pass: the median launch of the mix entry, per mode
    python tools/ab_recurrence.py --table parent=A.json,B.json,C.json refactor=D.json,E.json,F.json       (no GPU) -> the table, on stdout
Lines of a process: the TGCN predictor (mb_tgcn.py's shape) and the MSDR predictor (mb_msdr.py's two shapes), HIP backend, forward + backward and
forward under no_grad, ms; per pass the median launch of each step entry inside 10 forward + backward passes ("in-pass"), us; the four TGCN step
launches alone with 1 and 2 node tiles per workgroup, us.  Table: per tree the median of its processes' medians, then the smallest and largest
round of any of its processes; the yardstick is the first tree's own spread."""
import json
import re
import statistics
import sys

NUM = r"([0-9.]+) \(([0-9.]+) - ([0-9.]+)\)"


def measure(out_path, parts):
    import torch
    import mb_downstream as mb
    import mb_msdr
    import mb_stfgnn
    import mb_stsgcn
    import mb_tgcn
    from gptst_amd import ops
    res = {}

    def recurrence(name, tag):
        return name if "_tgcn_" in name or "_msdr_" in name else None

    def mix_by_mode(name, tag):                              # tag "m<mode> c<width> T<frames>": one line per mode, the layers' launches together
        return name + " " + tag.split()[0] if name.endswith("_mix") else None

    def predictor_lines(label, predictor, shape, inpass=recurrence, **kw):
        m, x, w, _ = mb.ab_predictor(predictor, shape, verdicts=False, **kw)
        hip = next(s for s in reversed(mb.LINES) if s.startswith("  hip "))
        v = [float(g) for g in re.search("forward \\+ backward " + NUM + " +forward only \\(no_grad\\) " + NUM, hip).groups()]
        res[label + " predictor forward + backward, ms"], res[label + " predictor forward only (no_grad), ms"] = v[:3], v[3:]
        per = {}
        for _ in range(10):                                  # in-pass: per pass, the median launch of each step entry
            ops.TIMER = []
            mb.fb(m, x, w)
            torch.cuda.synchronize()
            acc = {}
            for name, tag, e0, e1, _n in ops.TIMER:
                key = inpass(name, tag)
                if key is not None:
                    acc.setdefault(key, []).append(e0.elapsed_time(e1) * 1e3)
            ops.TIMER = None
            for name, t in acc.items():
                per.setdefault((name, len(t)), []).append(statistics.median(t))
        for (name, n), t in per.items():
            res["%s in-pass %s (n %d), us" % (label, name[6:], n)] = [statistics.median(t), min(t), max(t)]
        del m, x, w
        torch.cuda.empty_cache()

    if "tgcn" in parts:
        predictor_lines("tgcn", mb_tgcn.predictor, mb_tgcn.SHAPE)
    for ds, shape in mb_msdr.SHAPES if "msdr" in parts else ():
        predictor_lines("msdr %s" % ds, mb_msdr.make_predictor(ds), shape, warm=3, reps=5)
    for part, tool in (("stsgcn", mb_stsgcn), ("stfgnn", mb_stfgnn)):
        for ds, shape in tool.SHAPES if part in parts else ():
            predictor_lines("%s %s" % (part, ds), tool.make_predictor(ds), shape, inpass=mix_by_mode, warm=3, reps=5)
    if "tiles" in parts:
        mb_tgcn.ab_tiles()
    for s in mb.LINES:
        g = re.match(r"  (\w+) +tiles 1: " + NUM + " +tiles 2: " + NUM, s)
        if g:
            v = [float(t) for t in g.groups()[1:]]
            res["tgcn %s alone, tiles 1, us" % g.group(1)], res["tgcn %s alone, tiles 2, us" % g.group(1)] = v[:3], v[3:]
    json.dump(res, open(out_path, "w"), indent=0)


def table(specs):
    trees = []
    for spec in specs:
        name, files = spec.split("=")
        trees.append((name, [json.load(open(f)) for f in files.split(",")]))
    fold = lambda runs, k: (statistics.median(r[k][0] for r in runs), min(r[k][1] for r in runs), max(r[k][2] for r in runs))      # noqa: E731
    (pn, pr), (bn, br) = trees
    print("%-58s %-34s %-34s %s" % ("line (HIP backend)", pn + ": median (min - max)", bn + ": median (min - max)", bn + " median in " + pn + "'s spread"))
    above = 0
    for k in pr[0]:
        p, b = fold(pr, k), fold(br, k)
        verdict = "NO: above it" if b[0] > p[2] else ("below it" if b[0] < p[1] else "yes")
        above += b[0] > p[2]
        print("%-58s %-34s %-34s %s" % (k, "%.3f (%.3f - %.3f)" % p, "%.3f (%.3f - %.3f)" % b, verdict))
    print("%d lines, %d above the %s's spread" % (len(pr[0]), above, pn))


if __name__ == "__main__":
    if sys.argv[1] == "--measure":
        measure(sys.argv[2], sys.argv[3:] or ["tgcn", "msdr", "tiles"])
    else:
        table(sys.argv[2:])
