"""Downstream MSDR predictor against golden vectors generated from the reference implementation (tests/golden/make_golden_msdr.py: reference
model/MSDR/gmsdr_model.py, gmsdr_cell.py, args.py): the argument set with the reference's ``filter_type`` quirk, the 42-key parameter tree
in the reference's order after its first forward, the seeded initialisation, the output and every gradient (in float64, with W, b and R
moved off zero: msdr_util.perturb_), the supports, the backend switch and Run.py's dispatch."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import msdr_util as gu
from gptst_amd import config, graph
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import MSDR
from golden_util import load

G = load("msdr_small.npz")
TOL = 1e-5                 # largest absolute error over the reference tensor's largest magnitude (both sides float64: rounding leaves 1e-12)
N, B, T, C, D = 20, 2, 12, 64, 64
CELL = ["nodevec1", "nodevec2", "W", "b", "R", "gconv_weight_(384, 64)", "gconv_biases_64", "attlinear.weight", "attlinear.bias"]
CELL_SHAPES = [(N, 10), (10, N), (D, D), (N, D), (4, N, D), (384, D), (D,), (1, N * D), (1,)]


def _ap(**kw):
    return gu.model_args(N, graph.msdr_supports(G["A"], kw.pop("filter_type", "2000")), **kw)


def _err(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((got.detach().double().reshape(ref.shape) - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _golden_model(backend="torch"):
    m = MSDR(_ap(), "cpu", C, backend=backend)
    m.load_state_dict({k[3:]: torch.tensor(G[k]) for k in G.files if k.startswith("sd.")}, strict=True)
    return m


@pytest.mark.parametrize("ds,n,seed,d,out", [("PEMS08", 170, 12, 64, 1), ("METR_LA", 207, 0, 64, 1), ("NYC_BIKE", 250, 12, 128, 2),
                                            ("NYC_TAXI", 266, 12, 64, 2)])
def test_confs_parse_to_the_reference_values(ds, n, seed, d, out):
    pa = predictor_args(ds, "MSDR")
    assert pa.filter_type == "2000" and pa.cl_decay_steps == 2000          # the reference's default: the conf's dual_random_walk is never read
    assert (pa.num_nodes, pa.seq_len, pa.horizon) == (n, 12, 12) == (make_args(ds).num_nodes, 12, 12)
    assert (pa.max_diffusion_step, pa.num_rnn_layers, pa.output_dim, pa.rnn_units, pa.pre_k, pa.pre_v) == (1, 2, out, d, 4, 1)
    assert (pa.use_curriculum_learning, pa.construct_type, pa.l2lambda) == (True, "connectivity", 0) and not hasattr(pa, "input_dim")
    assert (pa.seed, pa.seed_mode, pa.xavier, pa.loss_func, pa.batch_size) == (seed, True, False, "mask_mae", 64)
    over = predictor_args(ds, "MSDR", ["--filter_type", "dual_random_walk", "--pre_k", "3"])
    assert over.filter_type == "dual_random_walk" and over.pre_k == 3 and over.cl_decay_steps == 2000 and over.num_nodes == n
    m = MSDR(SimpleNamespace(**vars(pa), supports=torch.eye(n)[None]), "cpu", 64)
    assert len(m.state_dict()) == 42 and "encoder_model.gmsdr_layers.0.gconv_weight_(%d, %d)" % (6 * d, d) in m.state_dict()


def test_gwn_is_still_refused_and_the_message_names_the_built_predictors():
    with pytest.raises(ValueError) as e:
        predictor_args("PEMS08", "GWN")
    assert all(name in str(e.value) for name in ("STSGCN", "STFGNN", "STGODE", "MSDR"))


def test_state_dict_is_the_reference_tree_after_its_first_forward():
    m = MSDR(_ap(), "cpu", C)
    keys = [str(k) for k in G["init.keys"]]
    want = (["encoder_model.mlp.weight", "encoder_model.mlp.bias"] + ["encoder_model.gmsdr_layers.%d.%s" % (l, k) for l in (0, 1) for k in CELL]
            + ["decoder_model.projection_layer.weight", "decoder_model.projection_layer.bias"]
            + ["decoder_model.gmsdr_layers.%d.%s" % (l, k) for l in (0, 1) for k in CELL] + ["out.weight", "out.bias"])
    assert len(keys) == 42 and keys == want and list(m.state_dict()) == keys
    sd = m.state_dict()
    for k in keys:
        assert tuple(sd[k].shape) == tuple(G["init." + k].shape), k
    for l in (0, 1):
        for k, shape in zip(CELL, CELL_SHAPES):
            assert tuple(sd["decoder_model.gmsdr_layers.%d.%s" % (l, k)].shape) == shape
    assert len(list(m.parameters())) == 42 and "supports" not in "".join(keys)             # nodevec1 / nodevec2 are parameters, the supports no key
    assert [k for k, _ in m.named_buffers()] == [p + ".gmsdr_layers.%d.supports" % l for p in ("encoder_model", "decoder_model") for l in (0, 1)]


def test_seeded_construction_equals_the_reference_after_one_forward():
    torch.manual_seed(int(G["seed"]))
    sd = MSDR(_ap(), "cpu", C).state_dict()
    for k in sd:
        assert torch.equal(sd[k], torch.tensor(G["init." + k])), k         # bit for bit, the four xavier draws the first forward makes included
    c = "decoder_model.gmsdr_layers.1."
    assert not bool(sd[c + "W"].any()) and not bool(sd[c + "R"].any()) and torch.equal(sd[c + "gconv_biases_64"], torch.ones(64))


def test_reference_state_loads_strictly_and_torch_backend_reproduces_the_vectors():
    m = _golden_model().double().train()
    x = torch.tensor(G["x"]).requires_grad_(True)
    y = m(x)
    assert m.backend_used == "torch" and tuple(y.shape) == (B, T, N, 1)
    (y * torch.tensor(G["w"])).sum().backward()
    assert _err(y, G["y"]) < TOL and _err(x.grad, G["dx"]) < TOL
    seen = 0
    for k, p in m.named_parameters():
        if k.startswith("out."):
            assert p.grad is None                                          # the dead head
            continue
        ref = G["grad." + k]
        if k.endswith("attlinear.bias"):                                   # identically zero (a constant added to every logit of a softmax)
            wmax = float(np.abs(G["grad." + k[:-4] + "weight"]).max())
            assert float(p.grad.abs().max()) <= 1e-6 * wmax and float(np.abs(ref).max()) <= 1e-6 * wmax, k
        else:
            assert float(np.abs(ref).max()) > 0 and _err(p.grad, ref) < TOL, k
        seen += 1
    assert seen == 40


@pytest.mark.parametrize("ft,nsup", [("2000", 1), ("dual_random_walk", 2), ("random_walk", 1), ("laplacian", 1)])
def test_supports_match_the_reference(ft, nsup):
    s = graph.msdr_supports(G["A"], ft)
    assert s.dtype == torch.float32 and tuple(s.shape) == (nsup, N, N)
    assert torch.allclose(s[0], s[0].t(), atol=1e-6) == (ft in ("2000", "laplacian"))      # Laplacians of max(A, A^T); the walks keep A's direction
    assert _err(s, G["sup." + ft]) < (1e-5 if ft == "laplacian" else 1e-6)                  # laplacian: dense eigenvalues against ARPACK's
    if ft == "2000":
        assert _err(s, G["sup.cell"]) < 1e-6                               # what the reference's cell builds for the default it resolves to
        assert torch.equal(graph.msdr_supports(G["A"], "anything else"), s)


def test_torch_backend_serves_the_other_branches():
    torch.manual_seed(0)
    for kw in (dict(filter_type="dual_random_walk"), dict(pre_v=2), dict(mds=2), dict(filter_type="dual_random_walk", mds=2, pre_v=2, K=3)):
        m = gu.perturb_(MSDR(_ap(T=3, horizon=2, **kw), "cpu", 16)).train()
        nsup = 2 if kw.get("filter_type") else 1
        assert m.cells()[0].theta.shape == (64 * (1 + kw.get("pre_v", 1)) * ((nsup + 1) * kw.get("mds", 1) + 1), 64)
        y = m(torch.randn(2, 3, N, 16))
        y.sum().backward()
        assert tuple(y.shape) == (2, 2, N, 1) and bool(torch.isfinite(y).all()) and float(m.cells()[0].theta.grad.abs().max()) > 0
    with pytest.raises(ValueError):
        MSDR(_ap(T=3, horizon=4), "cpu", 16)


def test_backend_switch_and_defaults():
    assert config.FINETUNE_DEFAULTS["msdr_backend"] == "torch" and make_args("PEMS08").msdr_backend == "torch"
    base = ["-dataset", "PEMS08", "-mode", "eval", "-model", "MSDR"]
    assert config.parse_args("cpu", base).msdr_backend == "torch"
    assert config.parse_args("cpu", base + ["-msdr_backend", "hip"]).msdr_backend == "hip"
    with pytest.raises(SystemExit):
        config.parse_args("cpu", base + ["-msdr_backend", "triton"])
    with pytest.raises(ValueError):
        MSDR(_ap(), "cpu", C, backend="triton")


def test_hip_backend_on_a_cpu_input_takes_the_torch_path_bit_equally():
    a, b = _golden_model("hip").train(), _golden_model("torch").train()
    x = torch.tensor(G["x"]).float()
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = a(xa), b(xb)
    assert (a.backend, a.backend_used, b.backend_used) == ("hip", "torch", "torch") and torch.equal(ya, yb)
    ya.square().sum().backward()
    yb.square().sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert (p.grad is None and q.grad is None) or torch.equal(p.grad, q.grad), k


def test_run_py_dispatches_msdr():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpt-st_amd", "Run.py")
    spec = importlib.util.spec_from_file_location("gptst_run_for_msdr_test", path)
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    assert "MSDR" in run.EVAL_MODELS and "GWN" not in run.EVAL_MODELS
    src = open(path).read()
    assert 'str(args.model) == "MSDR"' in src and "graph.msdr_supports(A, pargs.filter_type)" in src and "args.msdr_backend" in src
