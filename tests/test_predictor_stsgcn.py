"""Downstream STSGCN predictor against golden vectors generated from the reference implementation (tests/golden/make_golden_stsgcn.py:
reference model/STSGCN/STSGCN.py, lib/metrics.py): the parameter tree, the seeded initialisation, the output and every gradient for the
``individual`` and ``sharing`` layers and two output channels, the graph, the huber loss and its selection, the argument set."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stsgcn_util as su
from gptst_amd import config, graph
from gptst_amd.config import make_args, predictor_args
from gptst_amd.eval_trainer import EvalTrainer, masked_huber, masked_mae
from gptst_amd.predictors import STSGCN
from gptst_amd.predictors.stsgcn import window_adjacency
from golden_util import load

G = load("stsgcn_small.npz")
TOL = 1e-4                 # the project's: largest absolute error over the reference tensor's largest magnitude
VARIANTS = {"ind": ("individual", 1, 54), "sha": ("sharing", 1, 30), "do2": ("individual", 2, 54)}


def _ap(module_type="individual", **kw):
    return su.model_args(20, G["A"], T=6, P=3, module_type=module_type, **kw)


def _sd(prefix):
    return {k[len(prefix):]: torch.tensor(G[k]) for k in G.files if k.startswith(prefix)}


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_state_dict_is_the_reference_tree_in_its_order(tag):
    module_type, dim_out, n = VARIANTS[tag]
    m = STSGCN(_ap(module_type), "cpu", 64, dim_out)
    want = _sd(tag + ".sd.")
    assert len(want) == n and list(m.state_dict()) == list(want)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in want.items()}
    assert "outputs.0.ouput_layer.weight" in want and ("stsgcl_layers.1.layer.gcms.1.layers.2.layer.bias" in want) == (module_type == "individual")
    assert sorted(k for k, _ in m.named_buffers()) == ["a_hat", "adj"] and not {"adj", "a_hat"} & set(m.state_dict())
    assert all(p.device.type == "cpu" for p in m.parameters())
    m.load_state_dict(want, strict=True)


@pytest.mark.parametrize("ds,dim_out,n", [("PEMS08", 1, 226), ("NYC_TAXI", 2, 112)])
def test_full_configurations_have_the_reference_entry_counts(ds, dim_out, n):
    pa = predictor_args(ds, "STSGCN")
    m = STSGCN(SimpleNamespace(**vars(pa), A=su.adjacency(pa.num_nodes)), "cpu", 64, dim_out)
    assert len(m.state_dict()) == n


def test_seeded_construction_draws_what_the_reference_draws():
    torch.manual_seed(int(G["seed"]))
    m = STSGCN(_ap(), "cpu", 64, 1)
    want = _sd("init.")
    sd = m.state_dict()
    assert len(want) == 54 and list(sd) == list(want)
    for k, v in want.items():
        assert torch.equal(sd[k], v), k
    assert not bool(sd["stsgcl_layers.0.layer.position_embedding.temporal_emb"].any())


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_torch_backend_reproduces_the_reference_vectors(tag):
    module_type, dim_out, n = VARIANTS[tag]
    m = STSGCN(_ap(module_type), "cpu", 64, dim_out)
    m.load_state_dict(_sd(tag + ".sd."), strict=True)
    x = torch.tensor(G[tag + ".x"], requires_grad=True)
    y = m(x)
    assert m.backend_used == "torch" and y.shape == (3, 3, 20, dim_out)
    (y * torch.tensor(G[tag + ".w"])).sum().backward()
    got, want = {"y": y.detach(), "dx": x.grad}, {"y": G[tag + ".y"], "dx": G[tag + ".dx"]}
    for k, p in m.named_parameters():
        got[k], want[k] = p.grad, G[tag + ".grad." + k]
    assert len(want) == n + 2 and all(np.abs(v).max() > 0 for v in want.values())
    errs = {k: float((got[k] - torch.tensor(want[k])).abs().max() / np.abs(want[k]).max()) for k in want}
    print("worst: %s" % max(errs.items(), key=lambda kv: kv[1])[0], {k: "%.2e" % v for k, v in errs.items() if v > 0.1 * TOL})
    assert all(v <= TOL for v in errs.values()), {k: v for k, v in errs.items() if v > TOL}


def test_two_output_channels_keep_the_reference_order():
    """the last axis of (B, P, N, 2) is the output layer's two rows of head p"""
    m = STSGCN(_ap(), "cpu", 64, 2)
    m.load_state_dict(_sd("do2.sd."), strict=True)
    x = torch.tensor(G["do2.x"])
    h = torch.relu(m.first_layer_embedding(x))
    for lay in m.stsgcl_layers:
        h = lay(h, m.adj)
    o = m.outputs[2]
    flat = h.transpose(1, 2).reshape(3, 20, -1)
    one = o.ouput_layer(o.hidden_layer(flat)).detach()                              # (B, N, 2)
    y = m(x).detach()
    assert y.shape == (3, 3, 20, 2) and float((y[:, 2] - one).abs().max()) < 1e-5
    assert float((y[..., 0] - y[..., 1]).abs().max()) > 1e-3


def test_stsgcn_graph_rebuilds_construct_adj_exactly():
    A = G["A"]
    assert not np.array_equal(A, A.T) and np.all(np.diag(A) == 0) and np.allclose(A.sum(1), 1, atol=1e-6)
    a_hat = graph.stsgcn_graph(A)
    assert a_hat.dtype == torch.float32 and a_hat.shape == (20, 20) and bool((a_hat.diagonal() == 1).all())
    off = ~torch.eye(20, dtype=torch.bool)
    assert torch.equal(a_hat[off], torch.tensor(A)[off])
    assert torch.equal(window_adjacency(a_hat).double(), torch.tensor(G["adj3"]))
    # the block rule on a random source equals the dense product
    S = torch.randn(2, 3, 20, 5, dtype=torch.float64)
    dense = (torch.tensor(G["adj3"]) @ S.reshape(2, 60, 5)).reshape(2, 3, 20, 5)
    assert float((su.mix_expanded(a_hat.double(), S) - dense).abs().max()) < 1e-12
    assert float((su.mix_middle(a_hat.double(), S) - dense[:, 1]).abs().max()) < 1e-12


def test_masked_huber_reproduces_the_reference_values():
    p, t, th = torch.tensor(G["huber.pred"]), torch.tensor(G["huber.true"]), float(G["huber.thresh"])
    assert abs(float(masked_huber(p, t, 0.0, 1.0, th)) - float(G["huber.loss"])) <= 1e-12 * float(G["huber.loss"])
    assert abs(float(masked_huber(p, t, 0.0, 1.0, th, delta=2.0)) - float(G["huber.loss_delta2"])) <= 1e-12 * float(G["huber.loss_delta2"])
    assert abs(float(masked_huber(p, t, 0.0, 1.0, -1.0)) - float(G["huber.loss_nomask"])) <= 1e-12 * float(G["huber.loss_nomask"])
    assert float(G["huber.loss"]) != float(G["huber.loss_nomask"]) != float(G["huber.loss_delta2"])
    # de-normalisation first: the threshold and delta act on real values
    mean, std = 1.5, 2.0
    assert abs(float(masked_huber((p - mean) / std, (t - mean) / std, mean, std, th)) - float(G["huber.loss"])) <= 1e-9


def test_eval_trainer_picks_the_loss_by_name(tmp_path):
    tr = EvalTrainer.__new__(EvalTrainer)
    tr.mean, tr.std = 0.0, 1.0
    p, t = torch.tensor(G["huber.pred"]).view(1, 1, 200, 1), torch.tensor(G["huber.true"]).view(1, 1, 200, 1)
    for name, f in (("mask_mae", masked_mae), ("mask_huber", masked_huber)):
        tr.args = SimpleNamespace(loss_func=name, output_dim=1, mape_thresh=0.001)
        assert float(tr._loss(p, t)) == float(f(p, t, 0.0, 1.0, 0.001))
    assert float(masked_mae(p, t, 0.0, 1.0, 0.001)) != float(masked_huber(p, t, 0.0, 1.0, 0.001))
    tr.args = SimpleNamespace(loss_func="mse", output_dim=1, mape_thresh=0.001)
    with pytest.raises(ValueError):
        tr._loss(p, t)


@pytest.mark.parametrize("ds,nodes,layers,seed", [("PEMS08", 170, 4, 12), ("METR_LA", 207, 4, 0), ("NYC_BIKE", 250, 1, 0), ("NYC_TAXI", 266, 1, 12)])
def test_predictor_args_restate_the_conf(ds, nodes, layers, seed):
    pa = predictor_args(ds, "STSGCN")
    assert (pa.num_nodes, pa.input_window, pa.output_window, pa.seed) == (nodes, 12, 12, seed)
    assert pa.filter_list == [[64, 64, 64]] * layers and (pa.module_type, pa.activation) == ("individual", "GLU")
    assert (pa.first_layer_embedding_size, pa.steps, pa.rho, pa.feature_dim) == (64, 3, 1, 64)
    assert (pa.use_mask, pa.xavier, pa.temporal_emb, pa.spatial_emb, pa.seed_mode) == (False, False, True, True, True)
    assert pa.loss_func == "mask_huber" and pa.batch_size == 64
    over = predictor_args(ds, "STSGCN", ["--module_type", "sharing", "--filter_list", "[[32, 32]]"])
    assert over.module_type == "sharing" and over.filter_list == [[32, 32]] and over.num_nodes == nodes
    with pytest.raises(ValueError) as e:
        predictor_args(ds, "GWN")
    assert "STSGCN" in str(e.value)


def test_backend_option_parses():
    assert config.FINETUNE_DEFAULTS["stsgcn_backend"] == "torch" and make_args("PEMS08").stsgcn_backend == "torch"
    base = ["-dataset", "PEMS08", "-mode", "eval", "-model", "STSGCN"]
    assert config.parse_args("cpu", base).stsgcn_backend == "torch"
    assert config.parse_args("cpu", base + ["-stsgcn_backend", "hip"]).stsgcn_backend == "hip"
    with pytest.raises(SystemExit):
        config.parse_args("cpu", base + ["-stsgcn_backend", "triton"])
    with pytest.raises(ValueError):
        STSGCN(_ap(), "cpu", 64, 1, backend="triton")


def test_use_mask_is_refused_and_relu_runs():
    with pytest.raises(NotImplementedError):
        STSGCN(_ap(use_mask=True), "cpu", 64, 1)
    m = STSGCN(_ap(activation="relu"), "cpu", 64, 1)
    assert m.stsgcl_layers[0].layer.gcms[0].layers[0].layer.weight.shape == (16, 16)
    y = m(torch.randn(2, 6, 20, 64))
    assert y.shape == (2, 3, 20, 1) and bool(torch.isfinite(y).all())
