"""Downstream MTGNN predictor against golden vectors generated from the reference implementation (tests/golden/make_golden_mtgnn.py:
reference model/MTGNN/MTGNN.py): the seeded initialisation, the parameter tree, the eval-mode output and every gradient, one training-mode
pass whose dropout masks come from the seeded random stream, and the predictor's argument set."""
import types

import numpy as np
import pytest
import torch

from gptst_amd.config import predictor_args
from gptst_amd.predictors import MTGNN
from golden_util import load

G = load("mtgnn_small.npz")
CFG = dict(num_nodes=20, input_window=12, output_window=12, output_dim=2, gcn_true=True, buildA_true=True, gcn_depth=2, dropout=0.3,
           subgraph_size=8, node_dim=40, dilation_exponential=1, conv_channels=16, residual_channels=16, skip_channels=16, end_channels=32,
           layers=3, propalpha=0.05, tanhalpha=3, layer_norm_affline=True, use_curriculum_learning=True, task_level=0)
DIM_IN = 16
TOL = 1e-5                                                                 # of the fixture tensor's largest magnitude (the TGCN CPU test's bound)


def _model(**kw):
    return MTGNN(types.SimpleNamespace(adj_mx=G["A"], **{**CFG, **kw}), "cpu", DIM_IN, kw.get("output_dim", CFG["output_dim"]))


def _sd(prefix="sd."):
    return {k[len(prefix):]: torch.tensor(G[k]) for k in G.files if k.startswith(prefix)}


def _against(m, tag):
    x = torch.tensor(G["x"], requires_grad=True)
    y = m(x)
    assert m.backend_used == "torch" and y.shape == (2, 12, 20, 2)
    (y * torch.tensor(G["w"])).sum().backward()
    got, want = {"y": y.detach(), "dx": x.grad}, {"y": G[tag + "y"], "dx": G[tag + "dx"]}
    for k, p in m.named_parameters():
        assert (p.grad is None) == k.startswith("residual_convs."), k     # built, in the state dict, and used by nothing with gcn_true
        if p.grad is not None:
            got[k], want[k] = p.grad, G[tag + "grad." + k]
    assert len(want) == 2 + 94 - 6
    errs = {k: float((got[k] - torch.tensor(want[k])).abs().max() / np.abs(want[k]).max()) for k in want}
    print(tag, "worst", max(errs, key=errs.get), "%.2e" % max(errs.values()))
    assert all(v < TOL for v in errs.values()), {k: v for k, v in errs.items() if v >= TOL}


def test_seeded_initialisation_equals_the_reference():
    torch.manual_seed(int(G["seed"]))
    m = _model()
    want = _sd("init.")
    assert len(want) == 94 and list(m.state_dict()) == list(want)         # the reference's keys in the reference's order
    for k, v in m.state_dict().items():
        assert torch.equal(v, want[k]), k
    assert "idx" not in want and "predefined_A" not in want
    assert torch.equal(m.predefined_A, torch.tensor(G["A"]) - torch.eye(20)) and torch.equal(m.idx, torch.arange(20))


def test_parameter_tree_loads_strictly_both_ways():
    torch.manual_seed(0)
    m, m2 = _model(), _model()
    m.load_state_dict(_sd(), strict=True)                                  # the reference's own state dict
    m2.load_state_dict(m.state_dict(), strict=True)
    assert {k: tuple(v.shape) for k, v in m2.state_dict().items()} == {k: tuple(v.shape) for k, v in _sd().items()}
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), _sd().values()))


def test_eval_mode_reproduces_the_reference_vectors():
    m = _model().eval()
    m.load_state_dict(_sd(), strict=True)
    _against(m, "")


def test_training_mode_draws_the_reference_dropout_masks():
    """dropout 0.3 on the padded input and on every layer's gated output, drawn in the reference's order from the seeded stream"""
    m = _model().train()
    m.load_state_dict(_sd(), strict=True)
    torch.manual_seed(int(G["train_seed"]))
    _against(m, "train.")
    assert float(np.abs(G["train.y"] - G["y"]).max()) > 1e-2              # the masks were active


def test_injected_masks_replace_the_random_stream():
    m = _model().train()
    m.load_state_dict(_sd(), strict=True)
    seen = []

    def keep(tag, like):
        seen.append((tag, tuple(like.shape)))
        return None
    m._keep = keep
    y = m(torch.tensor(G["x"]))
    assert seen == [("in", (2, 16, 20, 20)), ("l0", (2, 16, 20, 14)), ("l1", (2, 16, 20, 8)), ("l2", (2, 16, 20, 2))]
    assert float((y.detach() - torch.tensor(G["y"])).abs().max()) < TOL * float(np.abs(G["y"]).max())      # no mask: the eval-mode output
    m._keep = lambda tag, like: torch.zeros_like(like) if tag == "in" else None
    y0 = m(torch.tensor(G["x"]))
    assert float((y0 - y).abs().max()) > 1e-3                              # skip0 sees the dropped-out input


def test_double_copy_and_output_dim_one():
    """the top-k mask takes the dtype of the adjacency, so a .double() copy runs; output_dim 1 gives T = 19 -> 13 -> 7 -> 1"""
    torch.manual_seed(3)
    m = _model(output_dim=1).double().eval()
    assert (m.receptive_field, m.frames) == (19, [19, 13, 7, 1])
    y = m(torch.randn(2, 12, 20, DIM_IN, dtype=torch.float64))
    assert y.shape == (2, 12, 20, 1) and y.dtype == torch.float64
    adp = m.adjacency()
    assert int((adp > 0).sum(1).max()) <= 8 and int((m.gc.dense(m.idx) > 0).sum(1).max()) > 8            # the top-k cuts
    assert _model().frames == [20, 14, 8, 2]
    with pytest.raises(ValueError):
        MTGNN(types.SimpleNamespace(adj_mx=G["A"], **CFG), "cpu", DIM_IN, 2, backend="triton")


@pytest.mark.parametrize("ds,n,out,sub,end,seed", [("PEMS08", 170, 1, 20, 128, 12), ("METR_LA", 207, 1, 20, 128, 0),
                                                   ("NYC_TAXI", 266, 2, 20, 128, 12), ("NYC_BIKE", 250, 2, 40, 64, 12)])
def test_predictor_args(ds, n, out, sub, end, seed):
    p = predictor_args(ds, "MTGNN")
    assert (p.num_nodes, p.input_window, p.output_window, p.output_dim) == (n, 12, 12, out)
    assert (p.gcn_true, p.buildA_true, p.gcn_depth, p.dropout, p.subgraph_size, p.node_dim, p.dilation_exponential) == (True, True, 2, 0.3, sub, 40, 1)
    assert (p.conv_channels, p.residual_channels, p.skip_channels, p.end_channels, p.layers) == (32, 32, 64, end, 3)
    assert (p.propalpha, p.tanhalpha, p.layer_norm_affline, p.use_curriculum_learning, p.task_level) == (0.05, 3, True, True, 0)
    assert (p.seed, p.seed_mode, p.xavier, p.loss_func, p.batch_size, p.epochs) == (seed, False, False, "mask_mae", 64, 100)
    assert predictor_args(ds, "MTGNN", ["--layers", "2"]).layers == 2
    with pytest.raises(ValueError):
        predictor_args(ds, "GWN")
    m = MTGNN(types.SimpleNamespace(adj_mx=None, **vars(p)), "cpu", 64, out)
    assert len(m.state_dict()) == 94 and m.predefined_A is None and m.frames[0] == 18 + out
