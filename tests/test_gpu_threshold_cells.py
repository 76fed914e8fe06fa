"""GPU: the loss and metric kernels against fp32 torch on cells AT the threshold.  Every kept count here is exact, and the yardstick is the
reference's fp32 two-step inverse transform (tests/threshold_util.py::inverse32) — not fp64, which sides with a fused multiply-add on exactly
these cells.  Labels are synth.make_batch with a tenth of the flow cells set to the stored raw zero; tests/test_threshold_cells_cpu.py shows
that each input below holds enough of them under the mask for a kernel on the fused form to miss its count by at least 1 % of the cells.

The MAE tail has two bodies, tail_mfma_body<0, C> (csrc/kl_guest.h) and tail_kernel<0, C> (csrc/tails.hip).  Which one gptst_tail_mae launches
is decided by a library switch, for C = 64 and C = 128 alike — gptst_tune(15, .) of include/gptst_hip_testing.h, MFMA unless told otherwise —
never by the shape, and the MAE tail never travels as a guest of another launch (only the KL head does).  ops exposes no name for the choice,
so the tests set the switch themselves, run every case on both bodies, and put the default back."""
import contextlib

import numpy as np
import pytest
import torch

import step_grad_util as U
import threshold_util as TU
from oracle import metrics_oracle as MO
from test_gpu_kernels import close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAIL_BODIES = {"mfma": 1, "valu": 0}            # gptst_tune(15, value): tail_mfma_kernel (the default) | tail_kernel
COUNT_COLS_T, COUNT_COLS_TN = (0, 3), (0,)      # n1, n2 of the per-horizon table; K of the per-node one
SUM_TOL = 1e-9      # fp64 accumulation in another order: n u with n <= 1e6 terms, u = 1.1e-16, under a margin of ten — relative to the sum of |terms|


@contextlib.contextmanager
def tail_body(which):
    from gptst_amd import _C
    _C.lib().call("gptst_tune", 15, TAIL_BODIES[which])
    try:
        yield
    finally:
        _C.lib().call("gptst_tune", 15, TAIL_BODIES["mfma"])


def _thr_id(t):
    return "mae_%s-mape_%s" % t


# ---- a. gptst_metrics_accum ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_vis", [True, False], ids=["vis", "novis"])
@pytest.mark.parametrize("thr", TU.THRESHOLDS, ids=_thr_id)
@pytest.mark.parametrize("shape", TU.METRIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metrics_accum_matches_fp32_torch(shape, thr, with_vis, parity):
    from gptst_amd import ops
    mae_t, mape_t = thr
    _, T, N, D = shape
    d = TU.metric_inputs(shape, with_vis)
    sums_t, sums_tn = ops.metrics_new(T, N, DEV)
    for b, out, src, vis in d["calls"]:                                         # two calls accumulate
        ops.metrics_accum(out.to(DEV), src.to(DEV), d["lda"], None if vis is None else vis.to(DEV), TU.SIGMA, TU.MU, mae_t, mape_t,
                          b, T, N, D, sums_t, sums_tn)
    args = (d["out"], d["src"], d["lda"], d["vis"], TU.SIGMA, TU.MU, mae_t, mape_t, T, N, D)
    (rt, rn), (at, an) = TU.metric_sums(*args), TU.metric_sums(*args, absolute=True)
    gt, gn = sums_t.cpu(), sums_tn.cpu()
    masked_plant = int((d["plant"] & ((d["vis"] == 0) if with_vis else torch.ones_like(d["plant"]))).sum())
    for k, what in ((0, "n1"), (3, "n2")):
        diff = float((gt[:, k] - rt[:, k]).sum())
        print("metrics", shape, thr, "vis" if with_vis else "novis", what, "device %d, rule %d, excess %d (planted masked cells: %d)"
              % (float(gt[:, k].sum()), float(rt[:, k].sum()), diff, masked_plant))
        parity("count_excess_" + what, abs(diff))
    assert float(rt[:, 0].min()) > 0 and float(rt[:, 3].min()) > 0              # the reference keeps cells on every horizon
    for k in COUNT_COLS_T:
        assert torch.equal(gt[:, k], rt[:, k]), ("count column %d" % k, (gt[:, k] - rt[:, k]).tolist())
    for k in COUNT_COLS_TN:
        assert torch.equal(gn[..., k], rn[..., k]), "K"
    for name, g, r, a, cols in (("t", gt, rt, at, (1, 2, 4)), ("tn", gn, rn, an, (1, 2, 3, 4, 5))):
        for k in cols:
            e = float(((g[..., k] - r[..., k]).abs() / a[..., k].clamp_min(1e-300)).max())
            parity("sum_%s%d" % (name, k), e)
            assert e <= SUM_TOL, ("sums_%s column %d" % (name, k), e)
    got = ops.metrics_report(sums_t, sums_tn)
    p, y = TU.metric_py(*args[:2], args[3], TU.SIGMA, TU.MU, D)
    want = MO.test_report(p, y, mae_t, mape_t)
    ok = ~torch.isnan(want)
    parity("report_rel", float(((got - want).abs() / want.abs())[ok].max()))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4)            # MAE, RMSE, MAPE, CORR rows; fp32 means against double sums


# ---- b. gptst_mae_fwd / gptst_mae_bwd -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,thresh", TU.LOSS_CASES)
def test_mae_fwd_bwd_keep_set_is_fp32_torch(base, thresh, parity):
    from gptst_amd import ops
    out, src, vis, plant = TU.loss_inputs(base)
    B, T, N = TU.LOSS_SHAPE
    rows = B * T * N
    r = TU.loss_ref(out, src[..., :base], vis, TU.SIGMA, TU.MU, thresh)
    assert r["count"] > 0
    stats = torch.zeros(8, device=DEV)
    o, s, m = out.to(DEV).contiguous(), src.to(DEV).contiguous(), vis.to(DEV).contiguous()
    ops.mae_fwd(o, s, base + 2, m, TU.SIGMA, TU.MU, thresh, rows, base, stats)
    st = stats.cpu()
    masked_plant = plant & (vis == 0)
    print("mae_fwd base %d thresh %g: kept device %d, rule %d, excess %d (planted masked cells: %d)"
          % (base, thresh, float(st[1]), r["count"], float(st[1]) - r["count"], int(masked_plant.sum())))
    parity("count_excess", abs(float(st[1]) - r["count"]))
    assert float(st[1]) == float(r["count"])
    e = abs(float(st[0]) - r["total"]) / r["total"]
    parity("sum_abs_err", e)
    assert e < 1e-4
    dO = ops.mae_bwd(o, s, base + 2, m, TU.SIGMA, TU.MU, thresh, rows, base, stats).cpu()
    assert bool((dO[~r["keep"]] == 0).all()), "gradient on %d cells the reference drops" % int((dO[~r["keep"]] != 0).sum())
    assert bool((dO[masked_plant] == 0).all())
    close(dO, r["a"] / r["count"], what="mae bwd")


# ---- c. gptst_tail_mae, both bodies -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", list(TAIL_BODIES))
@pytest.mark.parametrize("J,C,rows", TU.TAIL_CASES)
def test_tail_mae_keep_set_is_fp32_torch(J, C, rows, body, parity):
    from gptst_amd import _C, ops
    dec, W, b, src, vis, plant = TU.tail_inputs(J, C, rows)
    r = TU.tail_ref(dec, W, b, src, vis, J, TU.SIGMA, TU.MU, TU.TAIL_THRESH)
    assert r["count"] > 0
    stats, sws = torch.zeros(8, device=DEV), ops.tail_sws(rows, DEV)
    with tail_body(body):
        out, dd, part = ops.tail_mae(dec.to(DEV), W.to(DEV), b.to(DEV), src.to(DEV), J + 2, vis.to(DEV), TU.SIGMA, TU.MU, TU.TAIL_THRESH, sws)
    ops.stats_fold(sws, stats)
    st = stats.cpu()
    masked_plant = plant & (vis.view(rows, J) == 0)
    print("tail_mae %s J %d C %d rows %d: kept device %d, rule %d, excess %d (planted masked cells: %d)"
          % (body, J, C, rows, float(st[1]), r["count"], float(st[1]) - r["count"], int(masked_plant.sum())))
    parity("count_excess", abs(float(st[1]) - r["count"]))
    close(out, r["out"], what="tail out")
    assert float(st[1]) == float(r["count"])
    e = abs(float(st[0]) - r["total"]) / r["total"]
    parity("sum_abs_err", e)
    assert e < 1e-4
    dd = dd.cpu()
    dropped_rows = ~r["keep"].any(1)
    assert bool((dd[dropped_rows] == 0).all()), "data gradient on rows whose every cell the reference drops"
    close(dd, r["d_dec"], what="tail d_dec")
    gwb = part.sum(0).cpu()
    close(gwb[:J * C].view(J, C), r["gW"], what="tail gW")
    close(gwb[J * C:], r["gb"], what="tail gb")
    assert _C.lib().value("gptst_tail_parts", rows) == part.shape[0]


def test_tail_bodies_differ_and_default_is_mfma():
    """the switch really selects another kernel: on one input the two bodies sum in another order (the data gradient differs in its last bits
    somewhere), and what ops.tail_mae launches untouched is the MFMA body, bit for bit"""
    from gptst_amd import ops
    J, C, rows = 2, 64, 1000
    dec, W, b, src, vis, _ = TU.tail_inputs(J, C, rows)
    a = [t.to(DEV) for t in (dec, W, b, src)]

    def run():
        sws = ops.tail_sws(rows, DEV)
        return ops.tail_mae(a[0], a[1], a[2], a[3], J + 2, vis.to(DEV), TU.SIGMA, TU.MU, TU.TAIL_THRESH, sws) + (sws,)
    plain = run()
    with tail_body("mfma"):
        mfma = run()
    with tail_body("valu"):
        valu = run()
    assert all(torch.equal(x, y) for x, y in zip(plain, mfma))
    assert not all(torch.equal(x, y) for x, y in zip(mfma, valu))
    assert torch.equal(mfma[3][:, 1].sum(), valu[3][:, 1].sum())               # and still keep the same cells


# ---- d. one fused step --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", list(TAIL_BODIES))
@pytest.mark.parametrize("name", TU.STEP_CASES)
def test_fused_step_keeps_the_fp32_torch_cells(name, body, parity):
    """the step's stats[1] is the fp32 torch count of the planted batch — step_grad_util.kept_count on the device's own mask, and the fp32 oracle's
    own count — and its MAE loss is the fp32 oracle's.  fp64 is not consulted: it keeps the planted cells.  Each case runs with the step's
    gptst_tail_mae launch on the MFMA body (the product's) and on the VALU body."""
    args, B, epoch, sd, src, inj, plant = TU.step_inputs(name)
    _, l32, m32, kept32 = U.oracle_grads(args, sd, src, epoch, inj, torch.float32)
    with tail_body(body):
        got, stats, mask, names, st = U.one_step(args, B, epoch, sd_seed=U.SD_SEED, inject=inj, src=src)
        lh = st.losses()
    assert "gptst_tail_mae" in names and "gptst_mae_fwd" not in names, sorted(set(names))      # the loss went through the tail
    vis = mask.cpu().reshape(m32.shape)
    assert torch.equal(vis, m32), (name, "the device's mask differs from the fp32 oracle's")
    kept = U.kept_count(args, src, vis)
    stats = stats.cpu()
    masked_plant = int((plant & (vis == 0)).sum())
    print("step %s %s: kept device %d, fp32 rule %d, fp32 oracle %d, excess %d (planted masked cells: %d)"
          % (name, body, float(stats[1]), kept, kept32, float(stats[1]) - kept, masked_plant))
    parity("count_excess", abs(float(stats[1]) - kept))
    assert kept > 0 and masked_plant > 0
    assert float(stats[1]) == float(kept) == float(kept32), (name, float(stats[1]), kept, kept32)
    e = abs(lh[1] - l32[1]) / abs(l32[1])
    parity("loss_mae", e)
    assert e < 1e-4, (name, lh[1], l32[1])
