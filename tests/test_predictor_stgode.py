"""Downstream STGODE predictor against golden vectors generated from the reference implementation (tests/golden/make_golden_stgode.py:
reference model/STGODE/STGODE.py, odegcn.py, args.py, with one Euler step standing in for torchdiffeq): the parameter tree with its dead
convolutions, the seeded initialisation, the output and every gradient for one and two output channels (in float64: relu and max decide),
the batch-norm buffers, the eval-mode output, the ties of the default initialisation, the two graphs, the argument set."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stgode_util as gu
from gptst_amd import config, graph
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import STGODE
from golden_util import check, load

G = load("stgode_small.npz")
TOL = 1e-4                 # the project's: largest absolute error over the reference tensor's largest magnitude
VARIANTS = {"do1": 1, "do2": 2}
NKEYS, NPARAMS, NDEAD = 316, 232, 144      # 12 blocks x (2 x 8 conv keys + 5 ode + 5 bn) + 4; 12 x (2 x 6 + 5 + 2) + 4; 12 x 12
N, T, P = 20, 5, 3


def _ap(**kw):
    return gu.model_args(N, T=T, P=P, g=(torch.tensor(G["A_sp"]), torch.tensor(G["A_se"])), **kw)


def _err(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((got.detach().double().reshape(ref.shape) - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _variant(tag):
    m = STGODE(_ap(), "cpu", 64, VARIANTS[tag])
    live = {k[len(tag) + 4:]: torch.tensor(G[k]) for k in G.files if k.startswith(tag + ".sd.")}
    missing, unexpected = m.load_state_dict(live, strict=False)
    assert not unexpected and all(gu.is_dead(k) for k in missing) and len(missing) + len(live) == NKEYS
    return m.double()


def test_state_dict_is_the_reference_tree_in_its_order():
    m = STGODE(_ap(), "cpu", 64, 1)
    keys = [str(k) for k in G["init.keys"]]
    assert len(keys) == NKEYS and list(m.state_dict()) == keys
    assert keys[:4] == ["sp_blocks.0.0.temporal1.conv.weight", "sp_blocks.0.0.temporal1.conv.bias", "sp_blocks.0.0.temporal1.network.0.0.weight",
                        "sp_blocks.0.0.temporal1.network.0.0.bias"]
    assert keys[8:13] == ["sp_blocks.0.0.odeg.odeblock.odefunc." + s for s in ("alpha", "w", "d", "w2", "d2")]
    assert keys[-4:] == ["pred.0.weight", "pred.0.bias", "pred.2.weight", "pred.2.bias"]
    assert len(list(m.parameters())) == NPARAMS
    assert sorted(k for k, _ in m.named_buffers() if "batch_norm" not in k) == ["A_se", "A_sp"] and not {"A_sp", "A_se"} & set(m.state_dict())
    assert m.sp_blocks[0][0].temporal1.conv is m.sp_blocks[0][0].temporal1.network[2][0]              # the alias the reference's attribute leaves


def test_seeded_construction_draws_what_the_reference_draws():
    torch.manual_seed(int(G["seed"]))
    sd = STGODE(_ap(), "cpu", 64, 1).state_dict()
    for k in sd:
        check(G, "init." + k, sd[k], rtol=1e-13, atol=0)                   # bit for bit (1e-13 lets the compact form's fp64 sums be added in another order)
    assert torch.equal(sd["se_blocks.2.1.odeg.odeblock.odefunc.w"], torch.eye(64)) and float(sd["sp_blocks.1.0.odeg.odeblock.odefunc.alpha"][3]) == pytest.approx(0.8)


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_torch_backend_reproduces_the_reference_vectors(tag):
    m = _variant(tag).train()
    x = torch.tensor(G[tag + ".x"]).requires_grad_(True)
    y = m(x)
    assert m.backend_used == "torch" and tuple(y.shape) == (2, P, N, VARIANTS[tag])
    (y * torch.tensor(G[tag + ".w"])).sum().backward()
    assert _err(y, G[tag + ".y"]) < TOL and _err(x.grad, G[tag + ".dx"]) < TOL
    nograd = {str(k) for k in G[tag + ".nograd"]}
    assert len(nograd) == NDEAD and all(gu.is_dead(k) for k in nograd)
    seen = 0
    for k, p in m.named_parameters():
        if k in nograd:
            assert p.grad is None, k                                       # the convolutions never ran
        else:
            assert _err(p.grad, G[tag + ".grad." + k]) < TOL, k
            seen += 1
    assert seen == NPARAMS - NDEAD
    sd = m.state_dict()
    for k in G.files:
        if k.startswith(tag + ".run."):
            key = k[len(tag) + 5:]
            if key.endswith("num_batches_tracked"):
                assert int(sd[key]) == int(G[k]) == 1
            else:
                assert _err(sd[key], G[k]) < TOL, key
    m.eval()
    with torch.no_grad():
        assert _err(m(x), G[tag + ".y_eval"]) < TOL


def test_default_initialisation_ties_go_to_the_first_branch_of_each_graph():
    torch.manual_seed(5)
    m = STGODE(_ap(), "cpu", 64, 1).double().train()
    x = torch.randn(2, T, N, 64, dtype=torch.float64)
    res = gu.model_manual(m, x)
    for i in (1, 2):
        assert torch.equal(res["outs"][i], res["outs"][0]) and torch.equal(res["outs"][3 + i], res["outs"][3])     # bit-identical within a graph
    assert set(res["which"].unique().tolist()) <= {0, 3} and {0, 3} <= set(res["which"].unique().tolist())
    m(x).sum().backward()
    zero = [k for k, p in m.named_parameters() if p.grad is not None and "odefunc" in k and not bool(p.grad.any())]
    losers = [k for k, _ in m.named_parameters() if "odefunc" in k and k.split(".")[1] != "0"]
    assert sorted(zero) == sorted(losers) and len(losers) == 40              # 4 losing branches x 2 blocks x 5
    nz = [k for k, p in m.named_parameters() if p.grad is not None and not bool(p.grad.any())]
    assert len(nz) == 56                                                     # with the batch-norm affine of the losers: 4 x 2 x 7


def test_graphs_match_the_reference():
    cfg = [float(v) for v in G["small.cfg"]]
    sp, dtw = graph.stgode_adjacencies(G["small.sp_dist"], G["small.dtw_dist"], sigma1=cfg[0], sigma2=cfg[1], thres1=cfg[2], thres2=cfg[3])
    np.testing.assert_allclose(sp, G["small.sp_matrix"], rtol=1e-12, atol=0)
    assert np.array_equal(dtw, G["small.dtw_matrix"]) and 0 < dtw.sum() < dtw.size and 0 < (sp > 0).sum() < sp.size
    a, b = graph.stgode_graphs(G["small.sp_dist"], G["small.dtw_dist"], *cfg)
    assert torch.equal(a, torch.tensor(G["small.A_sp"])) and torch.equal(b, torch.tensor(G["small.A_se"]))
    assert torch.equal(graph.stgode_normalized_adj(G["floor.A"]), torch.tensor(G["floor.norm"]))            # a node of degree 0: the floor 1e-4
    pa = predictor_args("PEMS08", "STGODE")
    a8, b8 = graph.stgode_graphs(G["pems08.sp_dist"], G["pems08.dtw_dist"], pa.sigma1, pa.sigma2, pa.thres1, pa.thres2)
    assert _err(a8, G["pems08.A_sp"]) < 1e-6 and _err(b8, G["pems08.A_se"]) < 1e-6 and a8.shape == (170, 170)


def test_spatial_distance_rule_and_exact_dtw():
    A = np.array([[0, 1.0], [0.25, 0]])
    np.testing.assert_allclose(graph.stgode_spatial_distance(A), [[1000, 0], [750, 1000]])
    rng = np.random.RandomState(3)
    series = rng.rand(3 * 8, 4)                                              # three days of 8 slots, 4 nodes
    d = graph.stgode_dtw_distances(series, day_slots=8)
    prof = series.reshape(3, 8, 4).mean(0)

    def dtw(a, b):                                                           # the textbook recurrence, unconstrained
        D = np.full((len(a) + 1, len(b) + 1), np.inf)
        D[0, 0] = 0
        for i in range(1, len(a) + 1):
            for j in range(1, len(b) + 1):
                D[i, j] = abs(a[i - 1] - b[j - 1]) + min(D[i - 1, j], D[i, j - 1], D[i - 1, j - 1])
        return D[-1, -1]
    want = np.array([[dtw(prof[:, i], prof[:, j]) for j in range(4)] for i in range(4)])
    np.testing.assert_allclose(d, want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("ds,n,seed", [("PEMS08", 170, 12), ("METR_LA", 207, 0), ("NYC_BIKE", 250, 12), ("NYC_TAXI", 266, 12)])
def test_confs_parse_to_the_reference_values(ds, n, seed):
    pa = predictor_args(ds, "STGODE")
    assert (pa.num_nodes, pa.num_timesteps_input, pa.num_timesteps_output) == (n, 12, 12) == (make_args(ds).num_nodes, 12, 12)
    assert (pa.sigma1, pa.sigma2, pa.thres1, pa.thres2) == (0.1, 10.0, 0.6, 0.5)
    assert (pa.in_channels, pa.out_channels, pa.n_layers) == (64, [64, 32, 64], 3)
    assert (pa.seed, pa.seed_mode, pa.xavier, pa.loss_func) == (seed, False, True, "mask_huber")
    m = STGODE(SimpleNamespace(**vars(pa), A_sp_wave=torch.eye(n), A_se_wave=torch.eye(n)), "cpu", 64, 1)
    assert len(m.state_dict()) == NKEYS and all(b.identity_form() for seq, _ in m.branches() for b in seq)


def test_backend_switch_and_defaults():
    assert config.FINETUNE_DEFAULTS["stgode_backend"] == "torch" and make_args("PEMS08").stgode_backend == "torch"
    with pytest.raises(ValueError):
        STGODE(_ap(), "cpu", 64, 1, backend="triton")
    with pytest.raises(ValueError) as e:
        predictor_args("PEMS08", "GWN")
    assert "STSGCN" in str(e.value) and "STFGNN" in str(e.value) and "STGODE" in str(e.value)


def test_other_input_width_runs_the_convolutions():
    torch.manual_seed(0)
    m = STGODE(_ap(), "cpu", 2, 1).train()                                 # -mode ori sizes: temporal1 of the first blocks has a downsample
    assert not m.sp_blocks[0][0].identity_form() and m.sp_blocks[0][1].identity_form()
    m(torch.randn(2, T, N, 2)).sum().backward()
    assert m.sp_blocks[0][0].temporal1.network[0][0].weight.grad is not None and m.sp_blocks[0][1].temporal1.conv.weight.grad is None
