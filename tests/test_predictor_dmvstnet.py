"""Downstream DMVSTNET predictor against golden vectors generated from the reference implementation (tests/golden/make_golden_dmvstnet.py:
reference model/DMVSTNET_demand/DMVSTNET.py, args.py): the argument set of the two demand confs and the refusal of every other dataset, the
22-key parameter tree in the reference's order, the seeded initialisation, the output and every gradient (in float64, off the
initialisation: dmvstnet_util.perturb_), the two sub-modules nothing reads, the raw adjacency, the backend switch and Run.py's dispatch."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dmvstnet_util as gu
from gptst_amd import config, graph
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import DMVSTNET
from golden_util import load

G = load("dmvstnet_small.npz")
TOL = 1e-5                 # largest absolute error over the reference tensor's largest magnitude (both sides float64: the bound of test_predictor_stmgcn.py)
B, T, N, C, OUT, HID, TOPO = 2, 12, 20, 64, 2, 32, 16
H = HID * OUT
LIN = lambda n: [n + ".weight", n + ".bias"]                                    # noqa: E731
KEYS = (["node_embeddings", "w"] + LIN("Lin_in_spa") + LIN("Lin_in_tem") + LIN("Lin_in_sen") + LIN("Local_GNN1.lin") + LIN("Local_GNN2.lin")
        + LIN("Local_GNN3.lin") + LIN("Lin_spa") + ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0"] + LIN("output"))
SHAPES = ([(N, TOPO), (TOPO, HID, HID)] + [(HID, C), (HID,)] * 3 + [(HID, HID), (HID,)] * 4 + [(4 * H, H), (4 * H, H), (4 * H,), (4 * H,)]
          + [(OUT, H + HID), (OUT,)])
RUN_PY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpt-st_amd", "Run.py")


def _ap(**kw):
    return gu.model_args(N, G["A"], **{"T": T, "hidden": HID, "topo": TOPO, **kw})


def _err(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((got.detach().double().reshape(ref.shape) - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _golden_model(backend="torch"):
    m = DMVSTNET(_ap(), "cpu", C, OUT, backend=backend)
    m.load_state_dict({k[3:]: torch.tensor(G[k]) for k in G.files if k.startswith("sd.")}, strict=True)
    return m


def _run_py():
    spec = importlib.util.spec_from_file_location("gptst_run_for_dmvstnet_test", RUN_PY)
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


@pytest.mark.parametrize("ds,n", [("NYC_TAXI", 266), ("NYC_BIKE", 250)])
def test_confs_parse_to_the_reference_values(ds, n):
    pa = predictor_args(ds, "DMVSTNET")
    assert (pa.input_window, pa.output_window, pa.num_nodes) == (12, 12, n) and make_args(ds).num_nodes == n
    assert (pa.hidden_dim, pa.topo_embedded_dim) == (64, 16)
    assert (pa.seed, pa.seed_mode, pa.xavier, pa.loss_func, pa.batch_size) == (12, True, False, "mask_mae", 64)
    over = predictor_args(ds, "DMVSTNET", ["--hidden_dim", "32", "--topo_embedded_dim", "8"])
    assert over.hidden_dim == 32 and over.topo_embedded_dim == 8 and over.num_nodes == n
    assert config._PRED_DIRS["DMVSTNET"] == "DMVSTNET_demand" and config.DMVSTNET_DATASETS == ("NYC_TAXI", "NYC_BIKE")
    # exactly the keys the reference's args.py reads: none of the nine its conf carries and never parses
    assert [k for _, k, *_ in config._DMVSTNET_KEYS] == ["input_window", "output_window", "num_nodes", "hidden_dim", "topo_embedded_dim", "seed",
                                                         "seed_mode", "xavier", "loss_func"]
    for dead in ("cnn_hidden_dim_first", "local_image_size", "num_feature", "seq_len", "kernel_size", "feature_len", "conv_len", "toponet_len",
                 "spatial_out_dim"):
        assert not hasattr(pa, dead), dead


@pytest.mark.parametrize("ds", ["PEMS08", "METR_LA"])
def test_other_datasets_are_refused_with_the_references_message(ds):
    with pytest.raises(ValueError, match="Demand prediction baseline. Please select NYC_TAXI or NYC_BIKE dataset!"):
        predictor_args(ds, "DMVSTNET")


def test_gwn_is_still_refused_and_the_message_names_the_built_predictors():
    with pytest.raises(ValueError) as e:
        predictor_args("PEMS08", "GWN")
    assert all(name in str(e.value) for name in ("STGCN", "TGCN", "MTGNN", "ASTGCN", "STSGCN", "STFGNN", "STGODE", "MSDR", "STWA", "STMGCN",
                                                 "CCRNN", "DMVSTNET"))
    run = _run_py()
    assert "DMVSTNET" in run.EVAL_MODELS and "GWN" not in run.EVAL_MODELS


def test_state_dict_is_the_reference_tree():
    m = DMVSTNET(_ap(), "cpu", C, OUT)
    keys = [str(k) for k in G["init.keys"]]
    assert len(keys) == 22 and keys == KEYS and list(m.state_dict()) == keys
    sd = m.state_dict()
    for k, shape in zip(keys, SHAPES):
        assert tuple(sd[k].shape) == tuple(G["init." + k].shape) == shape, k
    assert len(list(m.parameters())) == 22
    assert [k for k, _ in m.named_buffers()] == ["adj_mx"] and "adj_mx" not in sd       # the adjacency: a buffer, no key
    assert tuple(m(torch.zeros(1, T, N, C)).shape) == (1, T, N, OUT)
    long = DMVSTNET(SimpleNamespace(**{**vars(_ap()), "output_window": 3}), "cpu", C, OUT)      # output_window is read by nothing
    assert tuple(long(torch.zeros(1, T, N, C)).shape) == (1, T, N, OUT)


def test_seeded_construction_equals_the_reference():
    torch.manual_seed(int(G["seed"]))
    sd = DMVSTNET(_ap(), "cpu", C, OUT).state_dict()
    for k in sd:
        assert torch.equal(sd[k], torch.tensor(G["init." + k])), k


def test_reference_state_loads_strictly_and_torch_backend_reproduces_the_vectors():
    m = _golden_model().double().train()
    x = torch.tensor(G["x"]).requires_grad_(True)
    y = m(x)
    assert m.backend_used == "torch" and tuple(y.shape) == (B, T, N, OUT)
    (y * torch.tensor(G["w"])).sum().backward()
    assert _err(y, G["y"]) < TOL and _err(x.grad, G["dx"]) < TOL
    assert [str(k) for k in G["nograd.keys"]] == gu.NO_GRAD_KEYS
    seen = 0
    for k, p in m.named_parameters():
        if k in gu.NO_GRAD_KEYS:
            assert p.grad is None and ("grad." + k) not in G, k
            continue
        ref = G["grad." + k]
        assert float(np.abs(ref).max()) > 0 and _err(p.grad, ref) < TOL, k
        seen += 1
    assert seen == 18
    assert _err(m.lstm.bias_ih_l0.grad, m.lstm.bias_hh_l0.grad) < 1e-12          # they only ever appear as their sum


def test_the_two_unread_gnns_take_no_gradient_and_adam_leaves_them():
    m = _golden_model().train()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    m(torch.tensor(G["x"]).float()).square().sum().backward()
    for k, p in m.named_parameters():
        assert (p.grad is None) == (k in gu.NO_GRAD_KEYS), k
    opt.step()
    after = m.state_dict()
    for k in before:
        assert torch.equal(after[k], before[k]) == (k in gu.NO_GRAD_KEYS), k


@pytest.mark.parametrize("dim_out", [1, 3])
def test_dim_out_other_than_two_is_refused(dim_out):
    with pytest.raises(ValueError, match="dim_out must be 2"):
        DMVSTNET(_ap(), "cpu", C, dim_out)


def test_adjacency_is_read_as_it_is(tmp_path):
    A = G["A"]
    np.savetxt(tmp_path / "NYC_TAXI.csv", A, delimiter=",")
    got = graph.dmvstnet_adjacency(str(tmp_path / "NYC_TAXI.csv"), N)
    assert got.dtype == np.float32 and got.shape == (N, N) and np.abs(got - A).max() < 1e-7 and not got[N - 1].any()      # no normalisation
    np.savetxt(tmp_path / "bad.csv", A[:, :3], delimiter=",")
    with pytest.raises(ValueError):
        graph.dmvstnet_adjacency(str(tmp_path / "bad.csv"), N)
    with pytest.raises(ValueError):
        graph.dmvstnet_adjacency(str(tmp_path / "NYC_TAXI.csv"), N + 1)
    with pytest.raises(ValueError):
        DMVSTNET(gu.model_args(N + 1, A), "cpu", C, OUT)


def test_backend_switch_and_defaults():
    assert config.FINETUNE_DEFAULTS["dmvstnet_backend"] == "torch" and make_args("NYC_TAXI").dmvstnet_backend == "torch"
    base = ["-dataset", "NYC_TAXI", "-mode", "eval", "-model", "DMVSTNET"]
    assert config.parse_args("cpu", base).dmvstnet_backend == "torch"
    assert config.parse_args("cpu", base + ["-dmvstnet_backend", "hip"]).dmvstnet_backend == "hip"
    with pytest.raises(SystemExit):
        config.parse_args("cpu", base + ["-dmvstnet_backend", "triton"])
    with pytest.raises(ValueError):
        DMVSTNET(_ap(), "cpu", C, OUT, backend="triton")
    assert DMVSTNET(_ap(), "cpu", C, OUT).backend == "torch"


def test_run_py_dispatches_dmvstnet(tmp_path, capsys):
    run = _run_py()
    src = open(RUN_PY).read()
    assert 'str(args.model) == "DMVSTNET"' in src and "dmvstnet_adjacency(args, csv_path, A)" in src and "args.dmvstnet_backend" in src
    A = G["A"]
    np.savetxt(tmp_path / "NYC_TAXI.csv", A, delimiter=",")
    args = SimpleNamespace(dataset="NYC_TAXI", num_nodes=N)
    got = run.dmvstnet_adjacency(args, str(tmp_path / "NYC_TAXI.csv"), np.eye(N, dtype=np.float32))
    assert got.dtype == torch.float32 and _err(got, A) < 1e-7 and capsys.readouterr().out == ""
    # the file absent: the adjacency at hand, and one line that says so
    got = run.dmvstnet_adjacency(args, str(tmp_path / "absent.csv"), np.eye(N, k=1, dtype=np.float32))
    said = capsys.readouterr().out
    assert torch.equal(got, torch.tensor(np.eye(N, k=1, dtype=np.float32))) and said.count("\n") == 1 and "absent.csv" in said
