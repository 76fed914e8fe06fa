"""``STGCN(..., backend="hip")`` without a GPU: the switch, the fallback on CPU tensors, the shared parameter tree, the command-line option."""
import types

import numpy as np
import pytest
import torch

from gptst_amd import graph
from gptst_amd.config import make_args, parse_args
from gptst_amd.predictors import STGCN
from golden_util import load

G = load("stgcn_small.npz")


def _model(backend, dim_out=1):
    N = G["A"].shape[0]
    ap = types.SimpleNamespace(Ks=3, Kt=3, num_nodes=N, G=graph.stgcn_graph(G["A"]), blocks1=[64, 32, 128], drop_prob=0, outputl_ks=3)
    return STGCN(ap, "cpu", 64, dim_out, backend=backend)


def test_hip_backend_on_cpu_tensors_takes_the_torch_modules_and_matches_the_reference():
    m = _model("hip")
    m.load_state_dict({k[3:]: torch.tensor(G[k]) for k in G.files if k.startswith("sd.")}, strict=True)
    assert m.backend == "hip" and m.backend_used is None
    x = torch.tensor(G["x"], requires_grad=True)
    y = m(x)
    assert m.backend_used == "torch"
    tol = 2e-5
    assert float((y.detach() - torch.tensor(G["y"])).abs().max()) < tol * float(np.abs(G["y"]).max())
    (y * torch.tensor(G["w"])).sum().backward()
    assert float((x.grad - torch.tensor(G["dx"])).abs().max()) < tol * float(np.abs(G["dx"]).max())
    for k, p in m.named_parameters():
        ref = torch.tensor(G["grad." + k])
        assert float((p.grad - ref).abs().max()) <= tol * float(ref.abs().max()) + 1e-7, k


def test_both_backends_share_one_parameter_tree():
    torch.manual_seed(0)
    mh, mt = _model("hip", 2), _model("torch", 2)
    sh, st = mh.state_dict(), mt.state_dict()
    assert list(sh) == list(st) and all(sh[k].shape == st[k].shape for k in sh)
    assert not any(k.endswith("Lk") for k in sh)                       # the graph stays a non-persistent buffer
    mt.load_state_dict(sh, strict=True)
    mh.load_state_dict(st, strict=True)
    x = torch.randn(1, 12, G["A"].shape[0], 64)
    assert torch.equal(mh(x), mt(x)) and mt.backend_used == "torch"
    with pytest.raises(ValueError):
        _model("triton")


def test_stgcn_backend_option():
    base = ["-dataset", "PEMS08", "-mode", "eval", "-model", "STGCN"]
    assert parse_args("cpu", base).stgcn_backend == "torch"
    assert parse_args("cpu", base + ["-stgcn_backend", "hip"]).stgcn_backend == "hip"
    assert make_args("PEMS08", mode="eval").stgcn_backend == "torch"
    with pytest.raises(SystemExit):
        parse_args("cpu", base + ["-stgcn_backend", "eager"])
