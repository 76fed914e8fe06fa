"""Downstream TGCN predictor against golden vectors generated from the reference implementation (tests/golden/make_golden_tgcn.py:
reference model/TGCN/TGCN.py): the normalised graph, the seeded initialisation, the parameter tree, the output and every gradient."""
import types

import numpy as np
import pytest
import torch

from gptst_amd import graph
from gptst_amd.predictors import TGCN
from golden_util import load

G = load("tgcn_small.npz")
KEYS = {"tgcn_model.weights_0": (164, 200), "tgcn_model.weights_1": (164, 100), "tgcn_model.bias_0": (200,), "tgcn_model.bias_1": (100,),
        "output_model.weight": (12, 100), "output_model.bias": (12,)}
TOL = 1e-5


def _ap(output_dim=1):
    return types.SimpleNamespace(num_nodes=G["A"].shape[0], input_window=12, output_window=12, rnn_units=100, output_dim=output_dim,
                                 G=graph.tgcn_graph(G["A"]))


def _sd(prefix="sd."):
    return {k[len(prefix):]: torch.tensor(G[k]) for k in G.files if k.startswith(prefix)}


def test_tgcn_graph_is_the_reference_normalisation():
    A = G["A"]
    assert not np.array_equal(A, A.T)                                  # non-symmetric: the naive D^-1/2 A~ D^-1/2 is the transpose
    assert np.abs(graph.normalized_adjacency(A) - G["L"]).max() < 1e-12
    L = graph.tgcn_graph(A)
    assert L.dtype == torch.float32 and torch.equal(L, torch.tensor(G["L"]).float())
    assert np.abs(graph.normalized_adjacency(A).T - G["L"]).max() > 1e-2


def test_seeded_initialisation_equals_the_reference():
    torch.manual_seed(int(G["seed"]))
    m = TGCN(_ap(), "cpu", 64)
    want = _sd("init.")
    assert list(m.state_dict()) == list(want)
    for k, v in m.state_dict().items():
        assert torch.equal(v, want[k]), k


def test_parameter_tree_loads_strictly_both_ways_between_backends():
    torch.manual_seed(0)
    mt, mh = TGCN(_ap(), "cpu", 64), TGCN(_ap(), "cpu", 64, backend="hip")
    for m in (mt, mh):
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == KEYS
    mh.load_state_dict(_sd(), strict=True)                             # the reference's own state dict
    mt.load_state_dict(mh.state_dict(), strict=True)
    mh.load_state_dict(mt.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(mt.state_dict().values(), mh.state_dict().values()))


def test_torch_backend_reproduces_the_reference_vectors():
    m = TGCN(_ap(), "cpu", 64)
    m.load_state_dict(_sd(), strict=True)
    x = torch.tensor(G["x"], requires_grad=True)
    y = m(x)
    assert m.backend_used == "torch" and y.shape == (2, 12, 20, 1)
    (y * torch.tensor(G["w"])).sum().backward()
    got = {"y": y.detach(), "dx": x.grad}
    want = {"y": G["y"], "dx": G["dx"]}
    for k, p in m.named_parameters():
        got[k], want[k] = p.grad, G["grad." + k]
    assert set(want) == {"y", "dx"} | set(KEYS)
    errs = {k: float((got[k] - torch.tensor(want[k])).abs().max() / np.abs(want[k]).max()) for k in want}
    print({k: "%.2e" % v for k, v in errs.items()})
    assert all(v < TOL for v in errs.values()), errs


def test_two_output_channels_keep_the_reference_view():
    """(B, N, W * output_dim) viewed as (B, N, W, output_dim) and permuted to (B, W, N, output_dim)   (TGCN.py:172-174)"""
    torch.manual_seed(1)
    m = TGCN(_ap(2), "cpu", 64)
    x = torch.randn(1, 12, 20, 64)
    y = m(x)
    h = x.new_zeros(1, 20, 100)
    for t in range(12):
        h = m.tgcn_model(x[:, t], h)
    flat = m.output_model(h)                                           # (1, 20, 24)
    assert y.shape == (1, 12, 20, 2) and torch.equal(y[0, 3, 7], flat[0, 7, 6:8])
    with pytest.raises(ValueError):
        TGCN(_ap(), "cpu", 64, backend="triton")
