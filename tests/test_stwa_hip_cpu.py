"""The ST-WA HIP path's host side, checked without a GPU: the packed factors reproduce the generated weights, the factored cut formulas the
GPU tests hold the kernels to (stwa_util.cut_local / cut_spatial) are the module's Layer, and what the kernels do not serve takes the torch
path bit-equally."""
import pytest
import torch

import stwa_util as su
from gptst_amd.predictors import STWA, stwa_hip
from gptst_amd.predictors.stwa import reparameterize


def _model(N=11, lag=8, C=16, out=1, dim_in=5, backend="torch", dtype=torch.float64):
    torch.manual_seed(su.SEED)
    return su.perturb_(STWA(su.model_args(N, lag=lag, C=C, out=out), "cpu", dim_in, backend=backend)).to(dtype)


@pytest.mark.parametrize("C", [16, 32, 24])
def test_packed_factors_reproduce_the_generated_weights_and_biases(C):
    """fp64: the reference's generated W (B, N, C, C) and bias (B, N, C) against V, u folded by co, cb.  The two differ by rounding only
    (8.9e-16 measured on the reference's LinearCustom); bound 1e-12."""
    m = _model(C=C)
    B, N = 3, m.num_nodes
    nz = su.noise(B, N, 16, dtype=torch.float64)
    z = m.z_data(torch.randn(B, 8, N, 5, dtype=torch.float64), nz[0])
    for layer, eps in zip(m.layers, nz[1]):
        zl = z + reparameterize(layer.mu, layer.logvar, eps)
        V, u, Wl, bl = stwa_hip.pack(layer)
        co, cb = stwa_hip.coefficients(layer, zl)
        assert V.shape == (4, 6, C, C) and u.shape == (4, 6, C) and Wl.shape == (6, C, C) and bl.shape == (6, C) and co.shape == cb.shape == (B, N, 4, 5)
        one = torch.ones(B, N, 1, dtype=torch.float64)
        for g, gen in enumerate(layer.generators()):
            W, bias = gen(zl)
            assert su.err(torch.einsum("bnk,kij->bnij", torch.cat([one, co[:, :, g]], -1), V[g]), W) < 1e-12
            assert su.err(torch.matmul(torch.cat([one, cb[:, :, g]], -1), u[g]), bias) < 1e-12
            x = torch.randn(B, 3, N, C, dtype=torch.float64)
            ref = torch.matmul(x.unsqueeze(-2), W.unsqueeze(1)).squeeze(-2) + bias.unsqueeze(1)
            assert su.err(su.gen_map(x, g, co, cb, V, u), ref) < 1e-12
        assert torch.equal(Wl[4], layer.aggregator[0].weight) and torch.equal(bl[1], layer.temporal_att.projection2.bias)


@pytest.mark.parametrize("lag,C", [(12, 16), (8, 16), (5, 32)])
def test_the_factored_cut_formulas_are_the_modules_layer(lag, C):
    m = _model(lag=lag, C=C)
    B, N = 2, m.num_nodes
    nz = su.noise(B, N, 16, dtype=torch.float64)
    z = m.z_data(torch.randn(B, lag, N, 5, dtype=torch.float64), nz[0])
    h = torch.randn(B, lag, N, C, dtype=torch.float64)
    with torch.no_grad():
        for layer, eps in zip(m.layers, nz[1]):
            zl = z + reparameterize(layer.mu, layer.logvar, eps)
            got = su.layer_by_cuts(h, layer.proxies[0], *stwa_hip.coefficients(layer, zl), *stwa_hip.pack(layer), layer.cuts, layer.cut_size)
            want = layer(h, z, eps)
            assert tuple(want.shape) == (B, layer.cuts, N, C) and su.err(got, want) < 1e-12
            h = want


def test_supported_refuses_what_the_kernels_do_not_serve():
    x = torch.randn(2, 8, 11, 5)
    assert not stwa_hip.supported(_model(dtype=torch.float32, backend="hip"), x)             # a CPU input
    assert not stwa_hip.supported(_model(C=24, dtype=torch.float32, backend="hip"), x)
    assert not stwa_hip.supported(_model(backend="hip"), x.double())                          # fp64
    assert stwa_hip.WIDTHS == (16, 32) and stwa_hip.MAX_CUT == 6


def test_hip_backend_on_a_cpu_input_takes_the_torch_path_bit_equally():
    a, b = _model(backend="hip", dtype=torch.float32).train(), _model(backend="torch", dtype=torch.float32).train()
    x, w, nz = torch.randn(2, 8, 11, 5), torch.randn(2, 12, 11, 1), su.noise(2, 11, 16)
    ya, dxa, ga = su.run(a, x, w, nz)
    yb, dxb, gb = su.run(b, x, w, nz)
    assert (a.backend, a.backend_used, b.backend_used) == ("hip", "torch", "torch")
    assert torch.equal(ya, yb) and torch.equal(dxa, dxb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    torch.manual_seed(3)
    y1 = a(x)
    torch.manual_seed(3)
    assert torch.equal(y1, b(x))                                           # both backends draw the noise the same way
