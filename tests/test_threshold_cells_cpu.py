"""CPU: the reference side of tests/test_gpu_threshold_cells.py stands on its own feet.  The rule (two rounded fp32 steps) and one fused
multiply-add part ways on a stored raw zero; every input the GPU file feeds holds enough such cells under the mask that a kernel on the fused
form cannot pass its exact counts; metric_sums reproduces the metric oracle on the golden cases through the host-side report; the loss helpers
are oracle.gptst_oracle.mae_loss term by term; and the metric oracle's own fp32 std is exactly 0 at the constant-truth nodes."""
import os

import numpy as np
import pytest
import torch

import step_grad_util as U
import threshold_util as TU
from gptst_amd import ops, synth
from oracle import gptst_oracle as O
from oracle import metrics_oracle as MO

FX = np.load(os.path.join(os.path.dirname(__file__), "golden", "metrics.npz"))


def test_rules_part_ways_on_a_stored_zero():
    assert (synth.SCALER_MEAN, synth.SCALER_STD) == (230.0, 146.0)
    z = torch.tensor([TU.stored_zero()])
    assert abs(float(z) + 1.57534242) < 1e-7
    assert float(TU.inverse32(z)) == 0.0                      # the rule drops the cell at threshold 0
    f = float(TU.inverse_fused(z))
    assert f > 0.0 and abs(f - 7.153e-6) < 1e-8, f            # one rounding keeps it — and so does fp64 itself
    assert float(z.double() * 146.0 + 230.0) > 0.0
    # everywhere the two forms differ by the rounding of the product and no more (half an ulp of x sigma, and the final rounding of each):
    # it is the comparison against the threshold that tells them apart
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    a, b = TU.inverse32(x), TU.inverse_fused(x)
    assert bool(((a - b).abs().double() <= 2.0 ** -24 * ((x.double() * 146.0).abs() + 2 * b.abs().double())).all())


def _excess(label, vis, thresh=0.0):
    """(cells, kept under the rule, kept by the fused form) with M = 1 - vis (vis None: every cell is masked)"""
    vis = torch.zeros_like(label) if vis is None else vis
    r = TU.loss_ref(torch.zeros_like(label), label, vis, TU.SIGMA, TU.MU, thresh)
    return label.numel(), r["count"], TU.fused_count(label, vis, TU.SIGMA, TU.MU, thresh)


def _check_plant(what, label, vis, plant):
    cells, rule, fused = _excess(label, vis)
    masked_plant = int((plant & ((vis.reshape(plant.shape) == 0) if vis is not None else torch.ones_like(plant))).sum())
    print(what, "cells %d, kept: rule %d, fused %d, planted masked %d" % (cells, rule, fused, masked_plant))
    assert rule > 0, what                                     # the reference itself keeps cells: its loss is no 0/0
    assert fused - rule == masked_plant, (what, fused, rule, masked_plant)      # the excess IS the planted masked cells
    assert fused - rule >= max(1, -(-cells // 100)), (what, fused, rule, cells)


@pytest.mark.parametrize("shape", TU.METRIC_SHAPES)
@pytest.mark.parametrize("with_vis", [True, False])
def test_metric_inputs_separate_the_rules(shape, with_vis):
    d = TU.metric_inputs(shape, with_vis)
    D = shape[3]
    _check_plant("metrics %s vis=%s" % (shape, with_vis), d["src"][..., :D].contiguous(), d["vis"], d["plant"])
    assert sum(c[0] for c in d["calls"]) == d["src"].shape[0] and all(c[0] >= 1 for c in d["calls"])      # no launch on zero rows
    for b, out, src, vis in d["calls"]:
        assert b == shape[0] or shape[0] >= 2
        assert out.shape == (b * shape[1] * shape[2], D) and src.shape == (b,) + shape[1:3] + (d["lda"],)


@pytest.mark.parametrize("base", [1, 2])
def test_loss_inputs_separate_the_rules(base):
    out, src, vis, plant = TU.loss_inputs(base)
    _check_plant("loss base %d" % base, src[..., :base].contiguous(), vis, plant)
    for b, thresh in TU.LOSS_CASES:
        if b == base:
            assert TU.loss_ref(out, src[..., :base], vis, TU.SIGMA, TU.MU, thresh)["count"] > 0


@pytest.mark.parametrize("J,C,rows", TU.TAIL_CASES)
def test_tail_inputs_separate_the_rules(J, C, rows):
    dec, W, b, src, vis, plant = TU.tail_inputs(J, C, rows)
    _check_plant("tail J %d C %d rows %d" % (J, C, rows), src[:, :J].contiguous(), vis.view(rows, J), plant)


@pytest.mark.parametrize("name", TU.STEP_CASES)
def test_step_inputs_separate_the_rules(name):
    args, B, epoch, sd, src, inj, plant = TU.step_inputs(name)
    base = args.input_base_dim
    assert args.mape_thresh == 0.0
    with torch.no_grad():
        outs, aux = O.forward_pretrain(sd, args, src, epoch, materialize_5d=False, **inj)
    vis = aux["final_mask"].to(torch.float32)
    _check_plant("step " + name, src[..., :base].contiguous(), vis, plant)
    assert U.kept_count(args, src, vis) == _excess(src[..., :base].contiguous(), vis)[1]      # step_grad_util's count is the rule
    if epoch > args.change_epoch:
        # the adaptive mask hangs on the guide classifier's labels: no fp32 classifier flips one at this margin (tests/test_gpu_step_grads.py)
        assert U.label_margin(args, sd, src) > 1e-4


@pytest.mark.parametrize("name", ["pems", "nyc", "thr"])
def test_metric_sums_reproduce_the_oracle_rows(name):
    a, b = FX[name + ".thr"]
    mae_t, mape_t = (None if np.isnan(a) else float(a)), float(b)
    y_pred, y_true = torch.from_numpy(FX[name + ".pred"]), torch.from_numpy(FX[name + ".true"])
    B, T, N, D = y_true.shape
    st, sn = TU.metric_sums(y_pred.reshape(-1, D), y_true, D, None, 1.0, 0.0, mae_t, mape_t, T, N, D)      # identity scaler, as the fixtures are
    assert st.dtype == sn.dtype == torch.float64 and st.shape == (T, 5) and sn.shape == (T, N, 6)
    got = ops.metrics_report(st, sn)
    want = MO.test_report(y_pred, y_true, mae_t, mape_t)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-6)
    np.testing.assert_allclose(got.numpy(), FX[name + ".rows"], rtol=1e-6)


@pytest.mark.parametrize("base,thresh", TU.LOSS_CASES)
def test_loss_helpers_are_the_oracle_loss(base, thresh):
    out, src, vis, _ = TU.loss_inputs(base)
    o = out.clone().requires_grad_()
    loss = O.mae_loss(o, src[..., :base], (1 - vis).long(), TU.MU, TU.SIGMA, thresh)
    loss.backward()
    loss = float(loss.detach())
    r = TU.loss_ref(out, src[..., :base], vis, TU.SIGMA, TU.MU, thresh)
    assert abs(r["total"] / r["count"] - loss) < 1e-6 * loss        # fp32 mean against the fp64 sum of the same terms
    assert torch.equal((r["a"] / r["count"]).float() != 0, o.grad != 0)
    assert float(((r["a"] / r["count"]) - o.grad.double()).abs().max()) < 1e-6 * float(o.grad.abs().max())


@pytest.mark.parametrize("shape", TU.METRIC_SHAPES)
@pytest.mark.parametrize("with_vis", [True, False])
def test_oracle_std_is_exactly_zero_at_constant_truth(shape, with_vis):
    """What the CORR column of the GPU test leans on: at a node whose truth is constant (mu where every cell is visible, 0.0 where every cell is a
    masked stored zero) the metric oracle's fp32 `true.std` is EXACTLY 0, so the oracle skips that node as ops.metrics_report does — and it is
    nonzero at every other node.  Held on every row that has more than one sample per node (the per-horizon rows of the 513-node shape have
    two).  On the all-horizon row of the two larger batches the constant nodes are the two built ones and no other; per horizon, and at 513 nodes
    with six cells each, chance adds nodes whose few cells are all visible — constant truth all the same, found here from the truth itself."""
    d = TU.metric_inputs(shape, with_vis)
    B, T, N, D = shape
    _, y = TU.metric_py(d["out"], d["src"], d["vis"], TU.SIGMA, TU.MU, D)
    built = {TU.NODE_PLANTED} | ({TU.NODE_VISIBLE} if with_vis else set())
    for row in list(range(T)) + [None]:
        yt = y[:, row] if row is not None else y
        per_node = yt.transpose(-1, -2).reshape(-1, N)                                   # (samples, N)
        assert per_node.shape[0] > 1
        const = (per_node == per_node[0]).all(0)
        ts = (yt.transpose(1, 2).unsqueeze(1) if yt.dim() == 3 else yt.transpose(2, 3)).std(dim=(0, 1, 2))      # as metrics_oracle.corr
        assert torch.equal(ts == 0, const), (shape, with_vis, row)
        assert all(bool(const[n]) for n in built)
        if row is None and y[:, :, 0].numel() >= 48:
            assert set(const.nonzero().flatten().tolist()) == built, (shape, with_vis)
    if with_vis:
        assert bool((y[:, :, TU.NODE_VISIBLE] == TU.MU).all()) and bool((y[:, :, TU.NODE_PLANTED] == 0.0).all())
