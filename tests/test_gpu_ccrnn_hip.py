"""The CCRNN predictor on HIP (``CCRNN(..., backend="hip")``, csrc/ccrnn.hip, predictors/ccrnn_hip.py) on the GPU.  The reference of every
comparison is in fp64 on the CPU: for a step launch its torch restatement (ccrnn_util.REF_OPS, which test_ccrnn_hip_cpu.py shows to compose
into the reference's vectors), for a whole model the torch backend of the same module (pinned to the reference implementation's vectors by
tests/test_predictor_ccrnn.py) and the golden vectors themselves.  The bound is the project's: 1e-4 of the reference tensor's largest
magnitude, for every output, dX and parameter gradient.

Shapes: N 16 (an exact tile), 20 (a ragged one), 37 (three tiles: a two-tile workgroup holds one dead tile), 266 and 250 (the shipped confs);
row tiles forced to 1 and 2 and left to the launch; hidden_size 25, 32, 16; dim_in 16, 64, 128; B 1, 3, 4; 1, 3 and 12 steps; k_hop 1 and 3;
one and two RNN layers; no targets, all forced, none forced and the seeded mix.  Every step launch is run twice and must repeat bit for bit."""
import random

import pytest
import torch

import ccrnn_util as gu
from gptst_amd import ops
from gptst_amd.predictors import CCRNN, ccrnn_hip
from golden_util import load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
G = load("ccrnn_small.npz")


def _err(got, ref):
    ref = torch.as_tensor(ref).double()
    ref = ref.detach()
    return float((got.detach().double().cpu().reshape(ref.shape) - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _g(t):
    return None if t is None else t.float().to(DEV).contiguous()


# ---- 1. the four step launches, each alone, against their restatements ---------------------------------------------------------------------
# (B, N, Hp, Cp, k, tiles, input): input "seq" = hoisted g and no slab input (the encoder's form, Cp = 0), "inp" = a given input, "fb" = the
# feedback formed on load.  Two steps in the seq tensors, the launch works on the second: a wrong (b, t) row offset shows.
STEP_CASES = [(1, 16, 32, 16, 3, 1, "fb"), (3, 20, 32, 16, 3, 2, "inp"), (3, 37, 32, 32, 3, 2, "inp"), (1, 37, 16, 0, 1, 1, "seq"),
              (3, 20, 16, 16, 1, 0, "fb"), (2, 37, 32, 0, 3, 2, "seq"), (3, 37, 16, 16, 3, 2, "fb"), (4, 266, 32, 16, 3, 0, "fb"),
              (4, 250, 32, 32, 3, 0, "inp")]
T2, T1 = 2, 1


def _both(name, cpu_args, outs, **kw):
    """run the restatement on the fp64 CPU tensors and the launch (twice) on fp32 GPU copies; ``outs``: the indices / keywords of the outputs"""
    def split(conv):
        a = [conv(v) if torch.is_tensor(v) else v for v in cpu_args]
        k = {n: (tuple(conv(e) for e in v) if isinstance(v, tuple) else conv(v) if torch.is_tensor(v) else v) for n, v in kw.items()}
        return a, k
    ca, ck = split(lambda v: v.clone())
    gu.REF_OPS[name](*ca, **ck)
    runs = []
    for _ in range(2):
        ga, gk = split(_g)
        getattr(ops, name)(*ga, **gk)
        torch.cuda.synchronize()
        runs.append((ga, gk))
    for o in outs:
        pick = (lambda a, k: a[o]) if isinstance(o, int) else (lambda a, k: k[o])           # noqa: E731
        ref, got, again = pick(ca, ck), pick(*runs[0]), pick(*runs[1])
        if ref is None:
            continue
        assert torch.equal(got, again), (name, o, "not bit-repeatable")
        assert _err(got, ref) < TOL, (name, o, _err(got, ref))


@pytest.mark.parametrize("B,N,Hp,Cp,k,tiles,kind", STEP_CASES)
def test_step_launches_match_their_restatement(B, N, Hp, Cp, k, tiles, kind):
    g = torch.Generator().manual_seed(B * 1000 + N * 10 + Hp + Cp + k)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)          # noqa: E731
    Np, S, rows, Ks, M = 16 * ((N + 15) // 16), B * N, B * T2 * N, Hp + Cp, k + 1
    P = torch.zeros(k, Np, Np, dtype=torch.float64)
    P[:, :N, :N] = rn(k, N, N) / N ** 0.5                                       # non-symmetric: a transposed graph shows
    PT = P.transpose(1, 2).contiguous()
    h, u, r, c = rn(S, Hp), torch.rand(S, Hp, dtype=torch.float64, generator=g), torch.rand(S, Hp, dtype=torch.float64, generator=g), torch.tanh(rn(S, Hp))
    W0, W1 = rn(2 * Hp, M * Ks) / (M * Ks) ** 0.5, rn(Hp, M * Ks) / (M * Ks) ** 0.5
    g0, g1 = (rn(rows, 2 * Hp), rn(rows, Hp)) if kind == "seq" else (rn(2 * Hp), rn(Hp))
    inp = rn(S, Cp) if Cp else None
    fb = (rn(S, Hp), rn(Cp, Hp) / Hp ** 0.5, rn(Cp)) if kind == "fb" else None
    e = lambda *s: torch.zeros(*s, dtype=torch.float64)                        # noqa: E731
    kw = dict(r=e(S, Hp), z=e(rows, M * Ks), tiles=tiles)
    if kind == "fb":
        kw.update(fb=fb, inp_out=e(S, Cp))
    elif Cp:
        kw.update(inp=inp)
    _both("ccrnn_fwd_gates", [P, W0, h, g0, T1, e(S, Hp), e(S, Hp), B, T2, N], [5, 6, "r", "z"] + (["inp_out"] if kind == "fb" else []), **kw)
    kw = dict(c=e(S, Hp), z=e(rows, M * Ks), tiles=tiles)
    if Cp:
        kw.update(inp=inp)
    _both("ccrnn_fwd_state", [P, W1, rn(S, Hp), g1, T1, u, h, e(S, Hp), B, T2, N], [7, "c", "z"], **kw)
    W1T, W0T = rn(Ks, M * Hp) / (M * Hp) ** 0.5, rn(Ks, M * 2 * Hp) / (M * 2 * Hp) ** 0.5
    kw = dict(dh2=rn(S, Hp) if kind != "inp" else None, tiles=tiles)
    if Cp:
        kw.update(dinp=e(S, Cp))
    _both("ccrnn_bwd_cand", [PT, W1T, rn(S, Hp), u, c, r, h, T1, e(rows, Hp), e(rows, 2 * Hp), e(S, Hp), B, T2, N], [8, 9, 10] + (["dinp"] if Cp else []), **kw)
    kw = dict(tiles=tiles)
    if Cp:
        kw.update(dinp=rn(S, Cp))
    _both("ccrnn_bwd_state", [PT, W0T, rn(rows, 2 * Hp), rn(S, Hp), T1, e(S, Hp), B, T2, N], [5] + (["dinp"] if Cp else []), **kw)


def test_steps_leave_the_other_rows_of_a_seq_tensor_alone():
    B, N, Hp, k = 2, 20, 16, 1
    g = torch.Generator().manual_seed(5)
    P = torch.zeros(k, 32, 32)
    P[:, :N, :N] = torch.randn(k, N, N, generator=g) / N ** 0.5
    z = torch.full((B * T2 * N, 2 * Hp), 7.0, device=DEV)
    h = torch.randn(B * N, Hp, generator=g).to(DEV)
    ops.ccrnn_fwd_gates(_g(P), _g(torch.randn(2 * Hp, 2 * Hp, generator=g)), h, _g(torch.randn(B * T2 * N, 2 * Hp, generator=g)), T1,
                        torch.empty_like(h), torch.empty_like(h), B, T2, N, z=z)
    zz = z.view(B, T2, N, -1)
    assert bool((zz[:, 0] == 7.0).all()) and not bool((zz[:, 1] == 7.0).any()) and torch.equal(zz[:, 1, :, :Hp].reshape(B * N, Hp), h)


# ---- 2. whole models against the fp64 torch backend (the oracle) and the golden vectors -----------------------------------------------------
def _pair(N, C, OUT=2, seed=gu.SEED, state=None, vec=0.05, **kw):
    """-> (the fp64 CPU torch-backend model, the fp32 GPU hip-backend model) holding the same parameters, off the initialisation"""
    torch.manual_seed(seed)
    base = CCRNN(gu.model_args(N, kw.pop("sup", gu.support(N)), **kw), "cpu", C, OUT)
    if state is None:
        gu.perturb_(base, vec)
    else:
        base.load_state_dict(state, strict=True)
    ref = CCRNN(gu.model_args(N, gu.support(N), **kw), "cpu", C, OUT).double().train()
    ref.load_state_dict(base.state_dict())
    hip = CCRNN(gu.model_args(N, gu.support(N), **kw), DEV, C, OUT, backend="hip").train()
    hip.load_state_dict(base.state_dict())
    return ref, hip


def _run(model, x, t, w, draw):
    """-> (y, dx, {key: grad}) of (y * w).sum();  draw: None (no targets), a float every ``random.random()`` returns, or "seed" """
    x = x.clone().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    real = random.random
    if draw == "seed":
        random.seed(gu.TF_SEED)
    elif draw is not None:
        random.random = lambda: draw
    try:
        y = model(x, None if draw is None else t)
    finally:
        random.random = real
    (y * w).sum().backward()
    return y.detach(), x.grad, {k: p.grad for k, p in model.named_parameters()}


def _compare(ref, hip, B, T, N, C, P, draw, seed=0):
    g = torch.Generator().manual_seed(seed + N + C)
    x, t, w = torch.randn(B, T, N, C, generator=g), torch.randn(B, P, N, 2, generator=g), torch.randn(B, P, N, 2, generator=g)
    yr, dxr, gr = _run(ref, x.double(), t.double(), w.double(), draw)
    yh, dxh, gh = _run(hip, x.to(DEV), t.to(DEV), w.to(DEV), draw)
    assert hip.backend_used == "hip" and ref.backend_used == "torch" and tuple(yh.shape) == (B, P, N, 2)
    errs = {"y": _err(yh, yr), "dx": _err(dxh, dxr)}
    for k in gr:
        if gr[k] is None:
            assert gh[k] is None, k                                           # w1, w2, b1, b2
        elif "attlinear" in k:
            assert not bool(gr[k].any()) and gh[k] is not None and not bool(gh[k].any()), k
        else:
            errs[k] = _err(gh[k], gr[k])
    print("largest error", max(errs.values()), max(errs, key=errs.get))
    assert max(errs.values()) < TOL, {k: v for k, v in errs.items() if v >= TOL}
    return yh, dxh, gh


# (B, T, N, C, H, P, k, rnn, draw, tiles)
MODEL_CASES = [(3, 3, 37, 128, 32, 3, 1, 2, 0.0, 2), (1, 1, 16, 16, 16, 1, 3, 1, 1.0, 1), (3, 3, 37, 16, 25, 3, 3, 1, 1.0, 2),
               (1, 12, 20, 64, 25, 12, 3, 2, "seed", 1), (3, 1, 16, 64, 32, 3, 1, 1, None, 0), (1, 3, 20, 128, 16, 12, 3, 2, 0.0, 0),
               (3, 12, 37, 64, 25, 3, 3, 1, "seed", 0)]


@pytest.mark.parametrize("B,T,N,C,H,P,k,rnn,draw,tiles", MODEL_CASES)
def test_model_matches_the_fp64_oracle(monkeypatch, B, T, N, C, H, P, k, rnn, draw, tiles):
    monkeypatch.setattr(ccrnn_hip, "TILES", tiles)
    ref, hip = _pair(N, C, H=H, P=P, k_hop=k, rnn=rnn, n_dim=min(10, N))
    _compare(ref, hip, B, T, N, C, P, draw)


@pytest.mark.parametrize("run", ["free", "tf"])
@pytest.mark.parametrize("rnn", [1, 2])
def test_model_matches_the_golden_vectors(rnn, run):
    pre = gu.tag(rnn, 1) + ".sd."
    ref, hip = _pair(20, 64, sup=G["support"], rnn=rnn, state={k[len(pre):]: torch.tensor(G[k]) for k in G.files if k.startswith(pre)})
    x, t, w = (torch.tensor(G[k]).to(DEV) for k in ("x", "targets", "w"))
    y, dx, grads = _run(hip, x, t, w, "seed" if run == "tf" else None)
    pre = "%s.%s." % (gu.tag(rnn, 1), run)
    errs = {"y": _err(y, G[pre + "y"]), "dx": _err(dx, G[pre + "dx"])}
    errs.update({k: _err(v, G[pre + "grad." + k]) for k, v in grads.items() if v is not None and "attlinear" not in k})
    print("largest error", max(errs.values()), max(errs, key=errs.get))
    assert hip.backend_used == "hip" and len(errs) == 2 + (12 if rnn == 1 else 20) and max(errs.values()) < TOL, errs
    assert [k for k, v in grads.items() if v is None] == ["w1", "w2", "b1", "b2"]


@pytest.mark.parametrize("N,C,rnn", [(266, 64, 1), (250, 128, 2)])             # NYC_TAXI; NYC_BIKE, whose encoder is 128 wide
def test_shipped_conf_shapes(N, C, rnn):
    # hidden_size 25, k_hop 3, 12 steps in, 12 out; vec: ccrnn_util.perturb_ and test_ccrnn_hip_cpu.py's test of the fp32 torch gap
    ref, hip = _pair(N, C, n_dim=50, rnn=rnn, vec=0.004)
    _compare(ref, hip, 4, 12, N, C, 12, "seed")


def test_a_step_repeats_bit_for_bit_and_eval_keeps_nothing():
    ref, hip = _pair(20, 64, rnn=2)
    a = _compare(ref, hip, 2, 3, 20, 64, 12, "seed")
    b = _compare(ref, hip, 2, 3, 20, 64, 12, "seed")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2] if a[2][k] is not None)
    hip.eval()
    x = torch.randn(2, 3, 20, 64, generator=torch.Generator().manual_seed(84)).to(DEV).requires_grad_(True)
    before = torch.cuda.memory_allocated()
    y = hip(x)
    assert hip.backend_used == "hip" and not y.requires_grad and y.grad_fn is None
    del y
    assert torch.cuda.memory_allocated() == before                              # nothing is kept
    hip.train()
    with torch.no_grad():
        assert not hip(x).requires_grad and hip.backend_used == "hip"


def test_a_forced_step_sends_no_gradient_into_its_output(monkeypatch):
    _, hip = _pair(20, 16, P=3)
    x, t = torch.randn(1, 2, 20, 16, device=DEV), torch.randn(1, 3, 20, 2, device=DEV)
    grads = {}
    for name, draw in (("all forced", 0.0), ("none forced", 1.0)):
        monkeypatch.setattr(random, "random", lambda d=draw: d)
        y = hip(x, t)
        grads[name], = torch.autograd.grad(y[:, 2].sum(), hip.decoder.out.bias)
    assert hip.backend_used == "hip" and torch.equal(grads["all forced"].cpu(), torch.full((2,), 20.0))
    assert float((grads["none forced"] - 20).abs().min()) > 1e-3


def test_three_graph_conv_layers_fall_back_to_torch():
    ref, hip = _pair(20, 64, gconv=3)
    x = torch.randn(2, 12, 20, 64, generator=torch.Generator().manual_seed(1))
    y = hip(x.to(DEV))
    assert hip.backend_used == "torch" and _err(y, ref(x.double())) < TOL
