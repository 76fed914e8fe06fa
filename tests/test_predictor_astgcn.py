"""Downstream ASTGCN predictor against golden vectors generated from the reference implementation (tests/golden/make_golden_astgcn.py:
reference model/ASTGCN/ASTGCN.py): the parameter tree, the seeded initialisation, the output and every gradient, the graph."""
import numpy as np
import pytest
import torch

import astgcn_util as au
from gptst_amd import graph
from gptst_amd.predictors import ASTGCN
from golden_util import load

G = load("astgcn_small.npz")
TOL = 1e-4                 # the project's: largest absolute error over the reference tensor's largest magnitude


def _ap(**kw):
    return au.model_args(G["A"].shape[0], torch.tensor(G["cheb"]).float(), **kw)


def _sd(prefix="sd."):
    return {k[len(prefix):]: torch.tensor(G[k]) for k in G.files if k.startswith(prefix)}


def test_state_dict_is_the_reference_tree_in_its_order():
    m = ASTGCN(_ap(), "cpu", 64, 1)
    want = _sd()
    assert len(want) == 40 and list(m.state_dict()) == list(want)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in want.items()}
    assert [k for k, _ in m.named_buffers()] == ["cheb"] and "cheb" not in m.state_dict()
    m.load_state_dict(want, strict=True)


def test_seeded_construction_draws_what_the_reference_draws():
    torch.manual_seed(int(G["seed"]))
    m = ASTGCN(_ap(), "cpu", 64, 1)
    want = _sd("init.")
    assert len(want) == 14                                             # per block: two convolutions and the LayerNorm; then final_conv
    sd = m.state_dict()
    for k, v in want.items():
        assert torch.equal(sd[k], v), k


def test_torch_backend_reproduces_the_reference_vectors():
    m = ASTGCN(_ap(), "cpu", 64, 1)
    m.load_state_dict(_sd(), strict=True)
    x = torch.tensor(G["x"], requires_grad=True)
    zs = []
    with au.recorded_sigmoids(zs):
        y = m(x)
    assert m.backend_used == "torch" and y.shape == (3, 12, 20, 1)
    (y * torch.tensor(G["w"])).sum().backward()
    got, want = {"y": y.detach(), "dx": x.grad}, {"y": G["y"], "dx": G["dx"]}
    for k, p in m.named_parameters():
        got[k], want[k] = p.grad, G["grad." + k]
    assert len(want) == 42
    au.assert_condition(zs, {k: want[k] for k in want if k not in ("y", "dx")})
    errs = {k: float((got[k] - torch.tensor(want[k])).abs().max() / np.abs(want[k]).max()) for k in want}
    print({k: "%.2e" % v for k, v in errs.items()})
    assert all(v <= TOL for v in errs.values()), errs


def test_astgcn_graph_against_the_reference_polynomials():
    """The reference takes lambda_max from ARPACK, graph.scaled_laplacian from the dense eigenvalues.  The generator measured, on this adjacency,
    a largest difference of 1.276e-06 in the scaled Laplacian and 4.877e-06 in the polynomials (T_2 doubles and squares it); the bound is ten
    times the latter, because ARPACK's stopping point is not ours to reproduce."""
    measured = 4.877e-06
    assert abs(float(G["lambda_diff"]) - measured) < 1e-8
    A = G["A"]
    assert not np.array_equal(A, A.T)
    cheb = graph.astgcn_graph(A, 3)
    assert cheb.dtype == torch.float32 and cheb.shape == (3, 20, 20)
    assert float((cheb.double() - torch.tensor(G["cheb"])).abs().max()) <= 10 * measured
    assert np.abs(graph.scaled_laplacian(A) - G["L"]).max() <= 10 * measured
    assert torch.equal(graph.astgcn_graph(A, 2), cheb[:2])


def test_two_output_channels_keep_the_reference_reshape():
    """(B, P * dim_out, N, 1) reshaped to (B, P, dim_out, N) and transposed to (B, P, N, dim_out)   (ASTGCN.py:309-311)"""
    torch.manual_seed(1)
    m = ASTGCN(_ap(), "cpu", 64, 2)
    au.xavier_pass_(m)
    au.move_score_vectors_(m)
    x = torch.randn(1, 12, 20, 64)
    y = m(x)
    h = x.permute(0, 2, 3, 1)
    for blk in m.BlockList:
        h = blk(h, m.cheb)
    flat = m.final_conv(h.permute(0, 3, 1, 2))                          # (1, 24, 20, 1)
    assert y.shape == (1, 12, 20, 2) and torch.equal(y[0, 3, 7], flat[0, 6:8, 7, 0])
    with pytest.raises(ValueError):
        ASTGCN(_ap(), "cpu", 64, 1, backend="triton")
