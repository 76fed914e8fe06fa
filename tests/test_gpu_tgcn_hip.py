"""The TGCN predictor on HIP (``TGCN(..., backend="hip")``, csrc/tgcn.hip, predictors/tgcn_hip.py) on the GPU.  The reference of every comparison
is the torch TGCN module (pinned to the reference implementation's vectors by tests/test_predictor_tgcn.py) or the step's formula, in fp64 on the
CPU; the bound is the project's element-wise one, 1e-4 of the reference tensor's largest magnitude, for every output, dX and parameter gradient.

Step shapes: padded widths Hp 16 (one column tile: three waves skip the mix, K below one k-block), 32, 48, 112 and 128 (two full slabs), each
with one and two row tiles per workgroup forced; the launch's own choice between the two (tiles = 0) is crossed at its boundary, 37 nodes at
B = 128 and 129, where it must be bit-equal to the forced count it names.  Every launch is run twice and must repeat bit for bit."""
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gptst_amd import _C, graph, ops, synth
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import TGCN, tgcn_hip as H
from golden_util import load
from downstream_util import _check, _err
from oracle import gptst_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _g(t):
    return t.float().to(DEV).contiguous()


# ---- 1. the four step launches, each alone -------------------------------------------------------------------------------------------------
# (1, 461, 112): 464 padded nodes, a slab of 126 208 bytes plus the M tile: every one of the four launches asks for more than the 64 KB of dynamic
# LDS a launch gets by default, up to 155 392 bytes (backward state, two tiles), just under the 160 KB a workgroup can have.
# Widths: (1, 16, 16): one column tile, so three of the four waves skip the mix, and K = 16 (32 in the backward state) is less than one
# 64-wide k-block of the GEMM; (3, 37, 48): three column tiles, one wave idle; 112: a second slab pass with a wave idle and a partial k-block;
# (2, 37, 128): two full 64-column slabs, K up to 256
STEP_SHAPES = [(1, 16, 32), (3, 37, 112), (2, 170, 112), (1, 461, 112), (1, 16, 16), (3, 37, 48), (2, 37, 128)]
T2, T1 = 2, 1                # two steps in the seq tensors, the launch works on the second: a wrong (b, t) row offset shows


def test_step_shapes_reach_beyond_64_kb_of_lds():
    v = _C.lib().value
    assert v("gptst_tgcn_lds_bytes", 461, 112, 1) == (464 * 68 + 16 * 228) * 4 > 126208 > 64 * 1024        # (one tile: the plan for B = 1)
    assert all(v("gptst_tgcn_lds_bytes", N, Hp, B) <= 64 * 1024 for B, N, Hp in STEP_SHAPES[:3])
    # the widest rows at a small graph: served, and on the near side of 64 KB whichever tile count is forced (13 056 + 16 640 a tile)
    assert 0 < v("gptst_tgcn_lds_bytes", 37, 128, 2) == (48 * 68 + 16 * 260) * 4 == 29696 <= 64 * 1024 and 29696 + 16 * 260 * 4 <= 64 * 1024
    assert all(0 < v("gptst_tgcn_lds_bytes", N, Hp, B) <= 64 * 1024 for B, N, Hp in STEP_SHAPES[4:])


def _step_inputs(B, N, Hp, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)          # noqa: E731
    Np = 16 * ((N + 15) // 16)
    L = rn(N, N) / N ** 0.5                                                       # non-symmetric: a transposed graph shows
    Lp = torch.zeros(Np, Np, dtype=torch.float64)
    Lp[:N, :N] = L
    return SimpleNamespace(L=L, Lp=_g(Lp), S=B * N, rows=B * T2 * N, rn=rn,
                           seq=lambda x: x.view(B, T2, N, -1)[:, T1].reshape(B * N, -1),       # the (b, T1) rows of a seq tensor
                           mix=lambda x: torch.matmul(L, x.view(B, N, -1)).reshape(B * N, -1))


# each launch at one shape and tile count -> (what it wrote, its errors against the fp64 formula); a repeated launch is bit-equal
def _fwd_gates(B, N, Hp, tiles):
    s = _step_inputs(B, N, Hp, N + Hp)
    W, h, Gx = s.rn(2 * Hp, Hp) / Hp ** 0.5, s.rn(s.S, Hp), s.rn(s.rows, 2 * Hp)
    M = s.mix(h)
    g = torch.sigmoid(M @ W.t() + s.seq(Gx))
    u, q, r = (torch.full((s.S, Hp), 7.0, device=DEV) for _ in range(3))
    z = torch.full((s.rows, 16 + Hp), 7.0, device=DEV)
    ops.tgcn_fwd_gates(s.Lp, _g(W), _g(h), _g(Gx), T1, u, q, B, T2, N, r=r, z=z, zoff=16, tiles=tiles)
    zz = z.view(B, T2, N, -1)
    assert bool((zz[:, 0] == 7).all()) and bool((zz[:, T1, :, :16] == 7).all())            # only its own block of z is written
    errs = {"r": _err(r, g[:, :Hp]), "u": _err(u, g[:, Hp:]), "q": _err(q, g[:, :Hp] * h), "m1": _err(s.seq(z.cpu())[:, 16:], M)}
    u2, q2 = torch.empty_like(u), torch.empty_like(q)
    ops.tgcn_fwd_gates(s.Lp, _g(W), _g(h), _g(Gx), T1, u2, q2, B, T2, N, tiles=tiles)       # nothing kept: the same u and q
    assert torch.equal(u2, u) and torch.equal(q2, q)
    return (u, q, r, z), errs


def _fwd_state(B, N, Hp, tiles):
    s = _step_inputs(B, N, Hp, N + Hp + 1)
    W, h, q, Gx, u = s.rn(Hp, Hp) / Hp ** 0.5, s.rn(s.S, Hp), s.rn(s.S, Hp), s.rn(s.rows, Hp), torch.sigmoid(s.rn(s.S, Hp))
    M = s.mix(q)
    c = torch.tanh(M @ W.t() + s.seq(Gx))
    hn, ck = (torch.full((s.S, Hp), 7.0, device=DEV) for _ in range(2))
    z = torch.full((s.rows, 16 + Hp), 7.0, device=DEV)
    ops.tgcn_fwd_state(s.Lp, _g(W), _g(q), _g(Gx), T1, _g(u), _g(h), hn, B, T2, N, c=ck, z=z, zoff=16, tiles=tiles)
    errs = {"c": _err(ck, c), "h": _err(hn, u * h + (1 - u) * c), "m2": _err(s.seq(z.cpu())[:, 16:], M)}
    hn2 = torch.empty_like(hn)
    ops.tgcn_fwd_state(s.Lp, _g(W), _g(q), _g(Gx), T1, _g(u), _g(h), hn2, B, T2, N, tiles=tiles)
    assert torch.equal(hn2, hn)
    return (hn, ck, z), errs


def _bwd_cand(B, N, Hp, tiles):
    s = _step_inputs(B, N, Hp, N + Hp + 2)
    Wt, dh, h = s.rn(Hp, Hp) / Hp ** 0.5, s.rn(s.S, Hp), s.rn(s.S, Hp)
    u, r, c = torch.sigmoid(s.rn(s.S, Hp)), torch.sigmoid(s.rn(s.S, Hp)), torch.tanh(s.rn(s.S, Hp))
    d1 = dh * (1 - u) * (1 - c * c)
    dq = s.mix(d1) @ Wt.t()                                                      # (the launch is handed L^T; here "L" plays that part)
    d0 = torch.cat([dq * h * r * (1 - r), dh * (h - c) * u * (1 - u)], 1)

    def run():
        dp1, dp0 = torch.full((s.rows, Hp), 7.0, device=DEV), torch.full((s.rows, 2 * Hp), 7.0, device=DEV)
        part = torch.empty(s.S, Hp, device=DEV)
        ops.tgcn_bwd_cand(s.Lp, _g(Wt), _g(dh), _g(u), _g(c), _g(r), _g(h), T1, dp1, dp0, part, B, T2, N, tiles=tiles)
        return dp1, dp0, part
    (dp1, dp0, part), again = run(), run()
    assert all(torch.equal(x, y) for x, y in zip((dp1, dp0, part), again))
    assert bool((dp1.view(B, T2, N, -1)[:, 0] == 7).all()) and bool((dp0.view(B, T2, N, -1)[:, 0] == 7).all())
    return (dp1, dp0, part), {"dpre1": _err(s.seq(dp1.cpu()), d1), "dpre0": _err(s.seq(dp0.cpu()), d0), "dh_part": _err(part, dh * u + dq * r)}


def _bwd_state(B, N, Hp, tiles):
    s = _step_inputs(B, N, Hp, N + Hp + 3)
    Wt, d0, part = s.rn(Hp, 2 * Hp) / Hp ** 0.5, s.rn(s.rows, 2 * Hp), s.rn(s.S, Hp)
    out, out2 = torch.empty(s.S, Hp, device=DEV), torch.empty(s.S, Hp, device=DEV)
    ops.tgcn_bwd_state(s.Lp, _g(Wt), _g(d0), _g(part), T1, out, B, T2, N, tiles=tiles)
    ops.tgcn_bwd_state(s.Lp, _g(Wt), _g(d0), _g(part), T1, out2, B, T2, N, tiles=tiles)
    assert torch.equal(out, out2)
    return (out,), {"dh": _err(out, part + s.mix(s.seq(d0)) @ Wt.t())}


@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("B,N,Hp", STEP_SHAPES)
def test_step_fwd_gates(B, N, Hp, tiles, parity):
    _check(parity, _fwd_gates(B, N, Hp, tiles)[1])


@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("B,N,Hp", STEP_SHAPES)
def test_step_fwd_state(B, N, Hp, tiles, parity):
    _check(parity, _fwd_state(B, N, Hp, tiles)[1])


@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("B,N,Hp", STEP_SHAPES)
def test_step_bwd_cand(B, N, Hp, tiles, parity):
    _check(parity, _bwd_cand(B, N, Hp, tiles)[1])


@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("B,N,Hp", STEP_SHAPES)
def test_step_bwd_state(B, N, Hp, tiles, parity):
    _check(parity, _bwd_state(B, N, Hp, tiles)[1])


@pytest.mark.parametrize("B,rule", [(128, 1), (129, 2)])
def test_the_kernel_s_own_tile_count_at_its_boundary(B, rule, parity):
    """tiles = 0 leaves the rows per workgroup to the launch: two 16-node tiles once B ceil(tiles / 2) exceeds 256.  37 nodes are 3 tiles, so
    B = 128 gives 256 (one tile a workgroup) and B = 129 gives 258 (two).  The LDS entry plans with the same rule: it shows which side was
    taken; and every launch of a step, left to the rule, writes bit for bit what it writes with that tile count forced, within TOL of fp64"""
    N, Hp = 37, 16
    assert _C.lib().value("gptst_tgcn_lds_bytes", N, Hp, B) == (48 * 68 + 16 * rule * (2 * Hp + 4)) * 4
    for launch in (_fwd_gates, _fwd_state, _bwd_cand, _bwd_state):
        own, errs = launch(B, N, Hp, 0)
        forced, _ = launch(B, N, Hp, rule)
        assert all(torch.equal(x, y) for x, y in zip(own, forced)), launch.__name__
        _check(parity, {launch.__name__[1:] + "." + k: v for k, v in errs.items()})


# ---- 2. the whole model --------------------------------------------------------------------------------------------------------------------
def _adj(N, seed=2):
    A = graph.synthetic_adjacency(N, seed)
    assert not np.array_equal(A, A.T)
    return A


def _ap(N, T=12, H=100, out=1, A=None):
    return SimpleNamespace(num_nodes=N, input_window=T, output_window=T, rnn_units=H, output_dim=out, G=graph.tgcn_graph(_adj(N) if A is None else A))


def _run(m, x, w):
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    y = m(xi)
    (y * w).sum().backward()
    return y.detach(), xi.grad, {k: p.grad.clone() for k, p in m.named_parameters()}


def _model_pair(B, T, N, C, Hd, out, seed):
    """the torch module in fp64 on the CPU (default init, gate biases moved off 0), its HIP twin, and a batch with its fp64 results"""
    torch.manual_seed(seed)
    ap = _ap(N, T, Hd, out)
    m64 = TGCN(ap, "cpu", C).double()
    with torch.no_grad():
        m64.tgcn_model.bias_0.normal_(0, 0.3)
        m64.tgcn_model.bias_1.normal_(0, 0.3)
    x64, w64 = torch.randn(B, T, N, C, dtype=torch.float64), torch.randn(B, T, N, out, dtype=torch.float64)
    ref = _run(m64, x64, w64)
    m = TGCN(ap, DEV, C, backend="hip").to(DEV)
    m.load_state_dict({k: v.float() for k, v in m64.state_dict().items()}, strict=True)
    return m, _g(x64), _g(w64), ref


def _errs(got, ref):
    errs = {"y": _err(got[0], ref[0]), "dx": _err(got[1], ref[1])}
    assert set(got[2]) == set(ref[2]) and len(ref[2]) == 6
    for k, g in ref[2].items():
        errs[k] = _err(got[2][k], g)
    return errs


CASES = [(2, 12, 20, 64, 100, 1), (3, 12, 37, 64, 100, 2), (2, 3, 16, 16, 32, 1), (1, 12, 170, 64, 100, 1), (2, 1, 20, 64, 128, 1)]


@pytest.mark.parametrize("B,T,N,C,Hd,out", CASES)
def test_whole_model_against_fp64_torch(B, T, N, C, Hd, out, parity):
    m, x, w, ref = _model_pair(B, T, N, C, Hd, out, 5 + N + Hd)
    m.train()
    got = _run(m, x, w)
    assert m.backend_used == "hip" and got[0].shape == (B, T, N, out)
    _check(parity, _errs(got, ref))


@pytest.mark.parametrize("ds", ["METR_LA", "NYC_BIKE", "NYC_TAXI"])
def test_shipped_tgcn_configuration_against_fp64_torch(ds, parity):
    """the predictor as ``-mode eval -model TGCN`` builds it from conf/TGCN/<dataset>.conf (207, 250 and 266 nodes) over a synthetic graph, one
    batch element of the 64-wide embedding"""
    pa = predictor_args(ds, "TGCN")
    assert (pa.num_nodes, pa.output_dim) == {"METR_LA": (207, 1), "NYC_BIKE": (250, 2), "NYC_TAXI": (266, 2)}[ds]
    m, x, w, ref = _model_pair(1, pa.input_window, pa.num_nodes, 64, pa.rnn_units, pa.output_dim, 5 + pa.num_nodes)
    m.train()
    got = _run(m, x, w)
    assert m.backend_used == "hip" and got[0].shape == (1, pa.output_window, pa.num_nodes, pa.output_dim)
    _check(parity, _errs(got, ref))


def test_lds_limit_depends_on_the_batch(parity):
    """N = 500 with 128 units: 512 padded nodes, a slab of 139 264 bytes.  A batch of 2 is planned with one row tile per workgroup, 155 904 bytes,
    and runs on the kernels; a batch of 17 is planned with two, 172 544 bytes, beyond the 160 KB of a workgroup: ``supported`` says no, and the
    SAME module answers through torch, bit for bit what a torch-backend twin gives"""
    N, Hd, C, T = 500, 128, 64, 3
    v = _C.lib().value
    assert v("gptst_tgcn_lds_bytes", N, Hd, 2) == 155904 <= H.LDS_MAX < v("gptst_tgcn_lds_bytes", N, Hd, 17) == 172544
    m, x, w, ref = _model_pair(2, T, N, C, Hd, 1, 5 + N + Hd)
    m.train()
    assert H.supported(m, x)
    got = _run(m, x, w)
    assert m.backend_used == "hip"
    _check(parity, _errs(got, ref))
    mt = TGCN(_ap(N, T, Hd, 1), DEV, C).to(DEV)
    mt.load_state_dict(m.state_dict(), strict=True)
    x17 = torch.randn(17, T, N, C, device=DEV)
    assert not H.supported(m, x17)
    yh, yt = m(x17), mt(x17)
    assert m.backend_used == "torch" and mt.backend_used == "torch" and yh.shape == (17, T, N, 1) and torch.equal(yh, yt)
    m(x)                                                                          # and the small batch is served by the kernels again
    assert m.backend_used == "hip"


def test_whole_model_against_the_reference_vectors(parity):
    G = load("tgcn_small.npz")
    m = TGCN(_ap(G["A"].shape[0], A=G["A"]), DEV, 64, backend="hip").to(DEV)
    m.load_state_dict({k[3:]: torch.tensor(G[k]) for k in G.files if k.startswith("sd.")}, strict=True)
    m.train()
    got = _run(m, torch.tensor(G["x"], device=DEV), torch.tensor(G["w"], device=DEV))
    assert m.backend_used == "hip"
    ref = (torch.tensor(G["y"]), torch.tensor(G["dx"]), {k: torch.tensor(G["grad." + k]) for k in got[2]})
    _check(parity, _errs(got, ref))


# ---- 3. padding, repeatability, modes ------------------------------------------------------------------------------------------------------
STEP_OPS = ("tgcn_fwd_gates", "tgcn_fwd_state", "tgcn_bwd_cand", "tgcn_bwd_state")
HOISTED = ("stgcn_nodemix", "stgcn_tapgemm", "stgcn_wgrad")


def _spy(monkeypatch):
    """every launch wrapper the backend calls, in order, and what the two forward step launches were handed to keep"""
    seen = {"calls": [], "kept": [], "h": []}

    def wrap(name):
        fn = getattr(ops, name)

        def f(*a, **kw):
            seen["calls"].append(name)
            if name == "tgcn_fwd_gates":
                seen["kept"].append((kw.get("r"), kw.get("z")))
            if name == "tgcn_fwd_state":
                seen["kept"].append((kw.get("c"), kw.get("z")))
                seen["h"].append(a[7])
            return fn(*a, **kw)
        monkeypatch.setattr(ops, name, f)
    for n in STEP_OPS + HOISTED:
        wrap(n)
    return seen


def test_padded_channels_repeatability_and_modes(monkeypatch):
    torch.manual_seed(3)
    B, T, N, Hd = 2, 12, 37, 100
    m = TGCN(_ap(N, T, Hd), DEV, 64, backend="hip").to(DEV)
    with torch.no_grad():
        m.tgcn_model.bias_0.normal_(0, 0.3)
        m.tgcn_model.bias_1.normal_(0, 0.3)
    x, w = torch.randn(B, T, N, 64, device=DEV), torch.randn(B, T, N, 1, device=DEV)
    seen = _spy(monkeypatch)
    m.train()
    y1, dx1, g1 = _run(m, x, w)
    fwd = ["stgcn_nodemix", "stgcn_tapgemm", "stgcn_tapgemm"] + ["tgcn_fwd_gates", "tgcn_fwd_state"] * T
    bwd = ["tgcn_bwd_cand", "tgcn_bwd_state"] * (T - 1) + ["tgcn_bwd_cand"] + ["stgcn_wgrad"] * 2 + ["stgcn_tapgemm"] * 2 + ["stgcn_nodemix"]
    assert m.backend_used == "hip" and seen["calls"] == fwd + bwd, seen["calls"]
    assert len(seen["kept"]) == 2 * T and all(a is not None and z is not None for a, z in seen["kept"])
    # every kept h: (B N, 112) with the 12 padded channels exactly 0, the others not
    assert len(seen["h"]) == T and all(h.shape == (B * N, 112) for h in seen["h"])
    assert all(bool((h[:, Hd:] == 0).all()) and bool((h[:, :Hd] != 0).any()) for h in seen["h"])
    # a second backward of the same batch: bit for bit
    y2, dx2, g2 = _run(m, x, w)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    # no_grad, and eval mode with gradients enabled: the same launches, the same output, nothing handed over to keep
    for mode in ("no_grad", "eval"):
        seen["calls"].clear(), seen["kept"].clear()
        if mode == "no_grad":
            with torch.no_grad():
                y3 = m(x)
        else:
            m.eval()
            y3 = m(x.clone().requires_grad_(True))
        assert torch.equal(y3, y1) and m.backend_used == "hip" and not y3.requires_grad and y3.grad_fn is None
        assert seen["calls"] == fwd and len(seen["kept"]) == 2 * T and all(a is None and z is None for a, z in seen["kept"]), (mode, seen)


def test_frozen_predictor_skips_the_weight_gradients(monkeypatch):
    """parameters that take no gradient: the input's gradient is the same, bit for bit, no weight-gradient kernel is launched and m1, m2 are not kept"""
    torch.manual_seed(3)
    m = TGCN(_ap(20), DEV, 64, backend="hip").to(DEV).train()
    x, w = torch.randn(2, 12, 20, 64, device=DEV), torch.randn(2, 12, 20, 1, device=DEV)
    want = _run(m, x, w)[1]
    for p in m.parameters():
        p.requires_grad_(False)
    seen = _spy(monkeypatch)
    xi = x.clone().requires_grad_(True)
    (m(xi) * w).sum().backward()
    assert m.backend_used == "hip" and "stgcn_wgrad" not in seen["calls"] and torch.equal(xi.grad, want)
    assert all(a is not None and z is None for a, z in seen["kept"])


def test_unsupported_input_takes_the_torch_path():
    torch.manual_seed(4)
    ap = _ap(20)
    mh, mt = TGCN(ap, DEV, 24, backend="hip").to(DEV), TGCN(ap, DEV, 24).to(DEV)
    mt.load_state_dict(mh.state_dict(), strict=True)
    x = torch.randn(2, 12, 20, 24, device=DEV)
    assert not H.supported(mh, x)
    yh, yt = mh(x), mt(x)
    assert mh.backend_used == "torch" and mt.backend_used == "torch" and torch.equal(yh, yt)


# ---- 4. the chain --------------------------------------------------------------------------------------------------------------------------
def _front_end(tmp_path, backend, finetune, sd):
    from gptst_amd.enhance import EnhanceFrontEnd
    from gptst_amd.eval_trainer import EvalTrainer
    N = 20
    args = make_args("PEMS08", mode="eval", num_nodes=N, embed_dim=8, HS=5, HT=6, scaler_zeros=synth.scaler_zeros(), batch_size=8, epochs=3,
                     early_stop=False, log_dir=str(tmp_path), debug=True, model="TGCN_test", tgcn_backend=backend)
    sd = O.init_state_dict(args, 4) if sd is None else sd
    torch.manual_seed(0)
    model = EnhanceFrontEnd(args, predictor=TGCN(_ap(N, out=args.output_dim), DEV, args.hidden_dim, backend=args.tgcn_backend),
                            finetune_encoder=finetune).to(DEV)
    model.load_pretrained_model(sd)
    return args, sd, model, EvalTrainer


@pytest.mark.parametrize("finetune", [False, True])
def test_chain_one_step_agrees_with_the_torch_backend(tmp_path, finetune, parity):
    args, sd, mh, ET = _front_end(tmp_path, "hip", finetune, None)
    _, _, mt, _ = _front_end(tmp_path, "torch", finetune, sd)
    mt.load_state_dict(mh.state_dict(), strict=True)
    src = synth.make_batch(2, 12, 20, 1, interval=args.interval, seed=21).to(DEV)
    tgt = synth.make_batch(2, 12, 20, 1, interval=args.interval, seed=22, start_slot=12).to(DEV)
    res = {}
    for name, model in (("hip", mh), ("torch", mt)):
        tr = ET(model, args, None, None, None, synth.SCALER_MEAN, synth.SCALER_STD)
        tr.logger.setLevel(logging.WARNING)
        model.train()
        loss = tr._loss(model(src, tgt)[0], tgt)
        loss.backward()
        assert model.predictor.backend_used == name
        res[name] = (float(loss.detach()), {k: p.grad for k, p in model.named_parameters() if p.requires_grad})
    assert set(res["hip"][1]) == set(res["torch"][1])
    assert any(k.startswith("pretrain_model.") for k in res["hip"][1]) == finetune
    errs = {"loss": abs(res["hip"][0] - res["torch"][0]) / abs(res["torch"][0])}
    for k, g in res["torch"][1].items():
        errs[k] = _err(res["hip"][1][k], g)
    _check(parity, errs)


def test_eval_trainer_learns_on_the_hip_backend(tmp_path):
    from gptst_amd import data as gdata
    args, sd, model, ET = _front_end(tmp_path, "hip", False, None)
    raw = synth.make_series(20, 3, days=6, seed=3)
    train, val, test, scaler, _, _ = gdata.get_dataloader(args, device=DEV, raw=raw, generator=torch.Generator().manual_seed(1))
    tr = ET(model, args, train, val, test, float(scaler.mean), float(scaler.std))
    tr.logger.setLevel(logging.WARNING)
    losses = [tr.train_epoch(e) for e in (1, 2, 3)]
    assert model.predictor.backend_used == "hip"
    assert losses[2] < losses[0] and all(np.isfinite(losses)), losses
    rows = tr.test(test)
    assert model.predictor.backend_used == "hip"
    assert rows.shape == (13, 4) and bool(torch.isfinite(rows[:, :3]).all())
