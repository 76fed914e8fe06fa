"""Downstream ST-WA predictor against golden vectors generated from the reference implementation (tests/golden/make_golden_stwa.py:
reference model/ST_WA/ST_WA.py, attention.py, args.py): the 215-key parameter tree in the reference's order, the seeded initialisation, the
output and every gradient (in float64 and in float32, with the generators' last Linears x 3: stwa_util.perturb_), the noise and its order
of draws, the cuts that read no data, the argument set, the backend switch and Run.py's dispatch."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stwa_util as su
from downstream_util import TOL as TOL32
from gptst_amd import config
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import STWA
from golden_util import load

G = load("stwa_small.npz")
TOL = 1e-5                 # largest absolute error over the reference tensor's largest magnitude (both sides float64: rounding leaves 1e-12)
CASES = {"A": dict(N=20, B=2, lag=12, out=1), "B": dict(N=13, B=3, lag=8, out=2)}
C = 64
# the whole-model inputs of test_gpu_stwa_hip.py: (B, lag, N, C, out), and the four shipped configurations at B = 1
GPU_CASES = [(2, 12, 20, 16, 1), (3, 8, 37, 16, 2), (1, 12, 170, 16, 1), (2, 5, 16, 32, 1)]
SHIPPED = [("PEMS08", 170, 1), ("METR_LA", 207, 1), ("NYC_BIKE", 250, 2), ("NYC_TAXI", 266, 2)]


def _ap(c, **kw):
    return su.model_args(CASES[c]["N"], lag=CASES[c]["lag"], out=CASES[c]["out"], **kw)


def _state(c):
    keys = [str(k) for k in G[c + ".init.keys"]]
    return {k: torch.tensor(G["%s.sd.%s" % (c, k)] if "%s.sd.%s" % (c, k) in G else G["%s.init.%s" % (c, k)]) for k in keys}


def _noise(c, dtype=torch.float32):
    return torch.tensor(G[c + ".eps_d"]).to(dtype), [torch.tensor(G[c + ".eps_l%d" % i]).to(dtype) for i in range(3)]


def _golden_model(c, backend="torch"):
    m = STWA(_ap(c), "cpu", C, backend=backend)
    m.load_state_dict(_state(c), strict=True)
    return m


@pytest.mark.parametrize("c", ["A", "B"])
def test_state_dict_is_the_reference_tree_and_seeded_construction_equals_it(c):
    torch.manual_seed(int(G["seed"]))
    m = STWA(_ap(c), "cpu", C)
    keys = [str(k) for k in G[c + ".init.keys"]]
    assert len(keys) == 215 and list(m.state_dict()) == keys and len(list(m.parameters())) == 215 and not list(m.named_buffers())
    sd = m.state_dict()
    for k in keys:
        assert torch.equal(sd[k], torch.tensor(G["%s.init.%s" % (c, k)])), k         # bit for bit
    one = STWA(_ap(c), "cpu", 1)
    assert len(one.state_dict()) == 213 and "eval_dimin.weight" not in one.state_dict()
    moved = [k for k in keys if "%s.sd.%s" % (c, k) in G]
    assert len(moved) == 48 and all(".4." in k and "generator" in k for k in moved)          # 3 layers x 4 generators x 2 Linears x 2


@pytest.mark.parametrize("c", ["A", "B"])
@pytest.mark.parametrize("dtype,tol", [(torch.float64, TOL), (torch.float32, TOL32)])
def test_reference_state_loads_strictly_and_torch_backend_reproduces_the_vectors(c, dtype, tol):
    """The identically zero gradients, measured on the CPU at these two inputs: fp32 torch leaves at most 9.5e-9 of the model's largest
    gradient on them (fp64 1e-17), so the bound 1e-6 keeps 100 x over the measurement."""
    m = _golden_model(c).to(dtype).train()
    y, dx, g = su.run(m, torch.tensor(G[c + ".x"]).to(dtype), torch.tensor(G[c + ".w"]).to(dtype), _noise(c, dtype))
    k_ = CASES[c]
    assert m.backend_used == "torch" and tuple(y.shape) == (k_["B"], 12, k_["N"], k_["out"])
    assert su.err(y, G[c + ".y"]) < tol and su.err(dx, G[c + ".dx"]) < tol
    gmax = max(float(np.abs(G["%s.grad.%s" % (c, k)]).max()) for k in g)
    seen = 0
    for k, v in g.items():
        ref = G["%s.grad.%s" % (c, k)]
        if su.degenerate(k):
            assert float(v.abs().max()) <= su.ZERO * gmax and float(np.abs(ref).max()) <= su.ZERO * gmax, k
        else:
            assert float(np.abs(ref).max()) > 0 and su.err(v, ref) < tol, (k, su.err(v, ref))
            seen += 1
    assert seen == 194 and len(g) == 215


@pytest.mark.parametrize("c", ["A", "B"])
def test_noise_none_draws_in_the_reference_order(c):
    m = _golden_model(c).train()
    x = torch.tensor(G[c + ".x"]).float()
    torch.manual_seed(int(G[c + ".noise_seed"]))
    y = m(x)                                                               # the reference's forward under this seed drew the recorded noise
    assert torch.equal(y, m(x, noise=_noise(c)))
    torch.manual_seed(int(G[c + ".noise_seed"]))
    eps_d, eps_l = m.draw_noise(x)
    assert torch.equal(eps_d, _noise(c)[0]) and all(torch.equal(a, b) for a, b in zip(eps_l, _noise(c)[1]))
    assert m.draw_noise(x.double())[0].dtype == torch.float64


def test_eval_mode_is_stochastic_too():
    m = _golden_model("A").eval()
    x = torch.tensor(G["A.x"]).float()
    with torch.no_grad():
        assert not torch.equal(m(x), m(x))
        assert torch.equal(m(x, noise=_noise("A")), m(x, noise=_noise("A")))


def test_cuts_past_the_end_of_the_input_read_no_data():
    """lag 12, first layer: cut_size 6, so cuts 0 and 1 hold all 12 steps and cuts 2 .. 11 slice past the end.  With the memory held fixed
    (the same z_data) the first layer's output depends on x in cuts 0, 1 directly and in later cuts only through the carried out_{i-1}."""
    m = _golden_model("A").double().eval()
    layer = m.layers[0]
    x = torch.tensor(G["A.x"]).double()
    nz = _noise("A", torch.float64)
    with torch.no_grad():
        z = m.z_data(x, nz[0])
        h = m.start_fc(x)
        h2 = h.clone()
        h2[:, 6:] += 1.0                                                   # cut 1's rows only
        a, b = layer(h, z, nz[1][0]), layer(h2, z, nz[1][0])
        assert tuple(a.shape) == (2, 12, 20, 16) and torch.equal(a[:, 0], b[:, 0]) and not torch.equal(a[:, 1], b[:, 1])
        # a 14-step input: cut 2 now reads steps 12, 13; cuts 0 and 1 are what they were
        c14 = layer(torch.cat([h, h[:, :2] + 0.5], dim=1), z, nz[1][0])
        assert torch.equal(c14[:, :2], a[:, :2]) and not torch.equal(c14[:, 2], a[:, 2])
        # cut i >= 2 is a function of out_{i-1} and the parameters alone: restart the chain from the carried value
        prox = layer.proxies[:, 4:6] + a[:, 1:2]
        zz = z + layer.mu + nz[1][0] * torch.exp(0.5 * layer.logvar)
        tp = [g(zz) for g in layer.temporal_parameter_generators]
        sp = [g(zz) for g in layer.spatial_parameter_generators]
        o = layer.spatial_att(layer.temporal_att(prox, prox, tp), sp)
        assert su.err((layer.aggregator(o) * o).sum(1), a[:, 2]) < 1e-12


@pytest.mark.parametrize("ds,n,seed,out", [("PEMS08", 170, 11, 1), ("METR_LA", 207, 0, 1), ("NYC_BIKE", 250, 0, 2), ("NYC_TAXI", 266, 12, 2)])
def test_confs_parse_to_the_reference_values(ds, n, seed, out):
    pa = predictor_args(ds, "STWA")
    assert (pa.num_nodes, pa.lag, pa.horizon) == (n, 12, 12) == (make_args(ds).num_nodes, 12, 12)
    assert (pa.channels, pa.memory_size, pa.out_dim, pa.dynamic) == (16, 16, out, "True") and pa.in_dim == out
    assert (pa.seed, pa.seed_mode, pa.xavier, pa.loss_func, pa.batch_size) == (seed, True, False, "mask_mae", 64)
    assert os.path.isfile(os.path.join(os.path.dirname(config.CONF_DIR), "ST-WA", ds + ".conf"))
    assert predictor_args(ds, "STWA", ["--dynamic", "False"]).dynamic == "False"           # a string: truthy, as in the reference
    m = STWA(SimpleNamespace(**vars(predictor_args(ds, "STWA", ["--dynamic", "False"]))), "cpu", 64)
    assert len(m.state_dict()) == 215 and tuple(m.layers[0].proxies.shape) == (1, 24, n, 16)


def test_an_empty_dynamic_raises_and_gwn_is_still_refused():
    with pytest.raises(ValueError):
        STWA(su.model_args(8, dynamic=""), "cpu", 4)
    with pytest.raises(ValueError):
        STWA(su.model_args(8, C=12), "cpu", 4)                             # not a multiple of the 8 heads
    with pytest.raises(ValueError) as e:
        predictor_args("PEMS08", "GWN")
    assert "STWA" in str(e.value)


def test_backend_switch_and_defaults():
    assert config.FINETUNE_DEFAULTS["stwa_backend"] == "torch" and make_args("PEMS08").stwa_backend == "torch"
    base = ["-dataset", "PEMS08", "-mode", "eval", "-model", "STWA"]
    assert config.parse_args("cpu", base).stwa_backend == "torch"
    assert config.parse_args("cpu", base + ["-stwa_backend", "hip"]).stwa_backend == "hip"
    with pytest.raises(SystemExit):
        config.parse_args("cpu", base + ["-stwa_backend", "triton"])
    with pytest.raises(ValueError):
        STWA(_ap("A"), "cpu", C, backend="triton")


def test_run_py_dispatches_stwa():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpt-st_amd", "Run.py")
    spec = importlib.util.spec_from_file_location("gptst_run_for_stwa_test", path)
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    assert "STWA" in run.EVAL_MODELS and "GWN" not in run.EVAL_MODELS
    src = open(path).read()
    assert 'str(args.model) == "STWA"' in src and "args.stwa_backend" in src


def _gpu_input(B, lag, N, Cc, out, seed=su.SEED):
    """the model, input, weight and noise of one whole-model GPU case, all float32 on the CPU (test_gpu_stwa_hip.py builds the same)"""
    torch.manual_seed(seed)
    m = su.perturb_(STWA(su.model_args(N, lag=lag, C=Cc, out=out), "cpu", 64)).train()
    g = torch.Generator().manual_seed(seed + 1)
    x, w = torch.randn(B, lag, N, 64, generator=g), torch.randn(B, 12, N, out, generator=g)
    return m, x, w, su.noise(B, N, 16, seed + 2)


@pytest.mark.parametrize("B,lag,N,Cc,out", GPU_CASES + [(1, 12, n, 16, o) for _, n, o in SHIPPED])
def test_every_gpu_input_is_sharp_and_within_fp32_reach(B, lag, N, Cc, out):
    """The conditions of stwa_util on the torch module alone, at every whole-model input the GPU tests use.  Measured here: sharpness
    2.8 - 9.4 x 1 / N, fp32 against fp64 at most 7.5e-6, degenerate gradients at most 2.3e-8 of the model's largest (bound 1e-6: 40 x)."""
    m, x, w, nz = _gpu_input(B, lag, N, Cc, out)
    sharp, e, zero, _ = su.conditions(m, x, w, nz)
    print("sharpness x N %.2f  fp32 vs fp64 %.2e  degenerate %.2e" % (sharp, e, zero))
    assert sharp >= su.SHARP and e <= su.FP32 and zero <= su.ZERO / 10
