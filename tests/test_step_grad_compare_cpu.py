"""CPU: the comparator of the fused step's gradient checks (tests/step_grad_util.py::compare) is proven before it is trusted.  The fp32 oracle's
gradients, dressed as PretrainStep.g (path A multiplied by the kept count), pass against the fp64 oracle; four defects of the kind the GPU file
is there to catch each fail: a tensor scaled by 1 + 1e-3, a transposed square weight, the KL segment scaled by 1.1, a kept count off by one."""
import pytest
import torch

import step_grad_util as U
from oracle import gptst_oracle as O

SMALLEST = ["small_rand", "small_ada"]
SCALED = "decoder.STHCN_decode.hyperTem2.weights_pool"
SQUARE = "encoder.STHCN_encode.cap1.ln_p.weight"


def _dressed(name):
    """(fp32 oracle gradients as the step stores them, stats_out, fp64 gradients, fp32 gradients, layout)"""
    c = U.CASES[name]
    args = U.case_args(name)
    sd = O.init_state_dict(args, U.SD_SEED)
    src = U.make_src(args, c["B"])
    inj = U.noise_inject(args, c["B"], c["epoch"])
    g64, _, m64, kept = U.oracle_grads(args, sd, src, c["epoch"], inj, torch.float64)
    g32, _, m32, kept32 = U.oracle_grads(args, sd, src, c["epoch"], inj, torch.float32)
    assert torch.equal(m32, m64) and kept32 == kept == U.kept_count(args, src, m64)
    layout = U.layout_of(args)
    offs, nA, nB = layout
    got = {}
    for k, g in g32.items():
        if g is None:
            got[k] = torch.zeros_like(sd[k])
        else:
            got[k] = g * kept if offs[k] < nA else g.clone()
    stats = torch.zeros(8)
    stats[1] = kept
    return got, stats, g64, g32, layout, c["epoch"] > args.change_epoch


def _run(got, stats, g64, g32, layout):
    seen = {}
    allowed = U.compare(got, stats, g64, lambda: g32, seen.__setitem__, layout)
    return allowed, seen


@pytest.mark.parametrize("name", SMALLEST)
def test_fp32_oracle_dressed_as_the_step_passes(name):
    got, stats, g64, g32, layout, kl = _dressed(name)
    allowed, seen = _run(got, stats, g64, g32, layout)
    assert allowed == {}                                         # nothing needed the fp32-oracle allowance at these cases
    trained = [k for k, g in g64.items() if g is not None]
    assert sorted(seen) == sorted("grad:" + k for k in trained)  # every trained tensor was measured and recorded
    assert max(seen.values()) < U.GRAD_TOL
    offs, nA, nB = layout
    assert any(nA <= offs[k] < nA + nB for k in trained) == kl   # the KL path has oracle gradients in the adaptive phase only


@pytest.mark.parametrize("name", SMALLEST)
def test_perturbed_copies_fail(name):
    got, stats, g64, g32, layout, kl = _dressed(name)
    offs, nA, nB = layout

    def fails(g, s, key):
        with pytest.raises(AssertionError) as ei:
            _run(g, s, g64, g32, layout)
        assert key in str(ei.value), (key, str(ei.value)[:300])

    # 1. one tensor scaled by 1 + 1e-3
    g = dict(got); g[SCALED] = got[SCALED] * (1 + 1e-3)
    fails(g, stats, SCALED)
    # 2. one transposed square weight
    assert got[SQUARE].shape[0] == got[SQUARE].shape[1]
    g = dict(got); g[SQUARE] = got[SQUARE].t().contiguous()
    fails(g, stats, SQUARE)
    # 3. the KL segment scaled by 1.1 (random phase: it has no gradient, so anything but zero there fails)
    klkeys = [k for k in got if nA <= offs[k] < nA + nB]
    assert klkeys
    g = dict(got)
    for k in klkeys:
        g[k] = got[k] * 1.1 if kl else got[k] + 1e-12
    fails(g, stats, "encoder.MLP_RL.ln3.weight")
    # 4. a kept count that is off by one
    s = stats.clone(); s[1] += 1
    fails(got, s, SCALED)
    s = stats.clone(); s[1] -= 1
    fails(got, s, SCALED)


def test_seeds_of_the_adaptive_cases():
    """the conditions the GPU file's mask handling rests on, for the seeds of the case table: the fp32 oracle's adaptive mask already equals
    the fp64 one, and the cases that must be compared on their free-running mask have a top-2 label margin far beyond fp32 rounding"""
    from test_gpu_step_grads import MARGIN, MUST_RUN_FREE
    seen = set()
    for name, c in U.CASES.items():
        args = U.case_args(name)
        key = (c["ds"], tuple(sorted(c["over"].items())), c["B"], c["epoch"])
        if c["epoch"] <= args.change_epoch or key in seen:
            continue
        seen.add(key)
        sd = O.init_state_dict(args, U.SD_SEED)
        src = U.make_src(args, c["B"])
        inj = U.noise_inject(args, c["B"], c["epoch"])
        masks = []
        with torch.no_grad():
            for dt in (torch.float32, torch.float64):
                cast = lambda v: v.to(dt) if torch.is_tensor(v) and v.dtype.is_floating_point else v      # noqa: E731
                sdd = {k: cast(v) for k, v in sd.items()}
                prob = O.guide_probability(sdd, cast(src), args.input_base_dim)
                label = torch.sort(prob, dim=-1, descending=True)[1][..., 0]
                ada, rnd = O.adaptive_counts(label.numel(), args.mask_ratio, c["epoch"], args.change_epoch, args.epochs, args.ada_mask_ratio)
                masks.append(O.adaptive_mask(label, inj["list_c"], cast(inj["noise_a"]), cast(inj["noise_r"]), ada, rnd, args.ada_type)[2])
            top2 = torch.topk(prob, 2, dim=-1)[0]
        assert torch.equal(masks[0], masks[1]), name
        if name in MUST_RUN_FREE:
            assert float((top2[..., 0] - top2[..., 1]).min()) > MARGIN, name
    assert all(U.CASES[n]["epoch"] > U.case_args(n).change_epoch for n in MUST_RUN_FREE) and MUST_RUN_FREE
