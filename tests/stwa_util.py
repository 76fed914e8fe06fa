"""What the ST-WA tests and the golden generator share (test_predictor_stwa.py, test_stwa_hip_cpu.py, test_gpu_stwa_hip.py,
golden/make_golden_stwa.py): the argument set, seeded noise, the move away from the initialisation, the identically zero gradients, and the
two conditions every whole-model input has to meet before a comparison on it means anything.

At the default initialisation the spatial softmax is almost uniform (the mean largest weight of a row is 1.06 - 1.12 x 1 / N at N = 16 .. 170
on the reference): a kernel that read the wrong key rows would pass.  ``perturb_`` multiplies weight and bias of every generator's last Linear
(``weight_generator[4]``, ``bias_generator[4]``) by 3 and touches nothing else; stronger moves push the reference's own fp32 error beyond the
project's bound.  ``conditions`` measures, on a torch module alone, the sharpness that leaves and the fp32-against-fp64 error."""
import re
from types import SimpleNamespace

import torch

SEED = 11
SHARP = 1.5                # the mean largest spatial weight of a row, in units of 1 / N: at least this
FP32 = 2e-5                # fp32 torch against fp64 torch by the project's measure: at most this
ZERO = 1e-6                # an identically zero gradient, over the largest gradient magnitude of the model: at most this

_DEGENERATE = re.compile(r"^layers\.\d+\.(temporal_parameter_generators\.0\.bias_generator\.\d\.(weight|bias)"
                         r"|spatial_parameter_generators\.0\.bias_generator\.4\.bias)$")


def model_args(N, lag=12, horizon=12, C=16, M=16, out=1, dynamic="True"):
    return SimpleNamespace(num_nodes=N, lag=lag, horizon=horizon, in_dim=1, out_dim=out, channels=C, dynamic=dynamic, memory_size=M)


def noise(B, N, M, seed=SEED, dtype=torch.float32, device="cpu"):
    """(eps_d (B, N, M), [eps_l (N, M)] * 3), drawn in float32 from a generator of its own"""
    g = torch.Generator().manual_seed(seed)
    eps_d = torch.randn(B, N, M, generator=g)
    eps_l = [torch.randn(N, M, generator=g) for _ in range(3)]
    return eps_d.to(device=device, dtype=dtype), [e.to(device=device, dtype=dtype) for e in eps_l]


def cast(nz, dtype=None, device=None):
    return nz[0].to(device=device, dtype=dtype), [e.to(device=device, dtype=dtype) for e in nz[1]]


def perturb_(model):
    """x 3 on the last Linear of every weight and bias generator (works on the reference's model too: the attribute names are the same)"""
    with torch.no_grad():
        for layer in model.layers:
            for g in list(layer.temporal_parameter_generators) + list(layer.spatial_parameter_generators):
                for lin in (g.weight_generator[4], g.bias_generator[4]):
                    lin.weight.mul_(3.0)
                    lin.bias.mul_(3.0)
    return model


def degenerate(key):
    """the 21 gradients that are identically zero, 7 per layer: the six tensors of the temporal KEY bias generator (a key bias common to all
    keys of a query cancels in the softmax) and the node-independent part of the spatial key bias"""
    return _DEGENERATE.match(key) is not None


def err(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((got.detach().double().reshape(ref.shape) - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def run(model, x, w, nz, probe=None):
    """one train-mode step of (y * w).sum() -> (y, dx, {key: gradient}); the model's gradients are cleared first"""
    model.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    y = model(x, noise=nz) if probe is None else model(x, noise=nz, probe=probe)
    (y * w).sum().backward()
    return y.detach(), x.grad.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def conditions(model32, x, w, nz):
    """-> (sharpness, fp32 error, zero ratio, fp64 result) of a float32 torch-backend module on the float32 input (x, w, noise): the mean largest
    spatial softmax weight of a row times N, the largest error of y, dx and the non-degenerate gradients of fp32 torch against an fp64 copy,
    and the largest fp32 degenerate gradient over the largest gradient magnitude of the model"""
    import copy
    m64 = copy.deepcopy(model32).double()
    probe = []
    y64, dx64, g64 = run(m64, x.double(), w.double(), cast(nz, torch.float64), probe)
    N = model32.num_nodes
    sharp = float(torch.stack([p.max(dim=-1).values.mean() for p in probe]).mean()) * N
    y32, dx32, g32 = run(model32, x, w, nz)
    e = max(err(y32, y64), err(dx32, dx64))
    gmax = max(float(v.abs().max()) for v in g64.values())
    zero = 0.0
    for k in g64:
        if degenerate(k):
            zero = max(zero, float(g32[k].abs().max()) / gmax, float(g64[k].abs().max()) / gmax)
        else:
            e = max(e, err(g32[k], g64[k]))
    return sharp, e, zero, (y64, dx64, g64)


# ---- one cut in the factored form the kernels use, written out with plain tensor ops (any dtype, any device; differentiable) ----------------
# V (4, 6, C, C), u (4, 6, C), co, cb (B, N, 4, 5), Wl (6, C, C), bl (6, C) as predictors/stwa_hip.pack / coefficients produce them.
HEADS = 8


def gen_map(x, g, co, cb, V, u):
    """x (B, R, N, C) -> x W_g(b, n) + bias_g(b, n) with W_g = V[g, 0] + sum_k co[b, n, g, k] V[g, 1 + k] (and u, cb for the bias)"""
    one = torch.ones_like(co[:, :, g, :1])
    W = torch.einsum("bnk,kij->bnij", torch.cat([one, co[:, :, g]], -1), V[g])
    bias = torch.matmul(torch.cat([one, cb[:, :, g]], -1), u[g])
    return torch.einsum("brni,bnij->brnj", x, W) + bias[:, None]


def _lin(x, l, Wl, bl):
    return torch.matmul(x, Wl[l].t()) + bl[l]


def cut_local(hrows, prox2, outprev, co, cb, V, u, Wl, bl):
    """hrows (B, R, N, C), prox2 (2, N, C), outprev (B, N, C) -> T, Ks, Vs (B, 2, N, C) and the temporal softmax weights (B, 2, R + 2, N, 8)"""
    B, R, N, C = hrows.shape
    hs = C // HEADS
    rows = torch.cat([prox2[None] + outprev[:, None], hrows], 1)
    k, v = gen_map(rows, 0, co, cb, V, u).view(B, R + 2, N, HEADS, hs), gen_map(rows, 1, co, cb, V, u).view(B, R + 2, N, HEADS, hs)
    q = rows[:, :2].reshape(B, 2, N, HEADS, hs)
    a = torch.softmax(torch.einsum("bpnhe,bmnhe->bpmnh", q, k) / hs ** 0.5, dim=2)
    o = torch.einsum("bpmnh,bmnhe->bpnhe", a, v).reshape(B, 2, N, C)
    T = _lin(torch.tanh(_lin(o, 0, Wl, bl)), 1, Wl, bl)
    return T, gen_map(T, 2, co, cb, V, u), gen_map(T, 3, co, cb, V, u), a


def cut_spatial(T, Ks, Vs, Wl, bl):
    """-> out (B, N, C), the mixed values S (B, 2, N, C), the scaled scores' row maxima and sums of exponentials (B, 2, N, 8), the weights"""
    B, _, N, C = T.shape
    hs = C // HEADS
    s = torch.einsum("bpnhe,bpmhe->bpnhm", T.view(B, 2, N, HEADS, hs), Ks.view(B, 2, N, HEADS, hs)) / hs ** 0.5
    mx = s.max(dim=-1).values
    e = torch.exp(s - mx[..., None])
    sm = e.sum(-1)
    a = e / sm[..., None]
    S = torch.einsum("bpnhm,bpmhe->bpnhe", a, Vs.view(B, 2, N, HEADS, hs)).reshape(B, 2, N, C)
    U = _lin(torch.relu(_lin(S, 2, Wl, bl)), 3, Wl, bl)
    g = torch.sigmoid(_lin(torch.relu(_lin(U, 4, Wl, bl)), 5, Wl, bl))
    return (g * U).sum(1), S, mx, sm, a


def layer_by_cuts(h, prox, co, cb, V, u, Wl, bl, cuts, cs):
    """a whole Layer from the two functions above: (B, T, N, C) -> (B, cuts, N, C)"""
    out, outs = torch.zeros_like(h[:, 0]), []
    for i in range(cuts):
        T, Ks, Vs, _ = cut_local(h[:, i * cs:(i + 1) * cs], prox[2 * i:2 * i + 2], out, co, cb, V, u, Wl, bl)
        out = cut_spatial(T, Ks, Vs, Wl, bl)[0]
        outs.append(out)
    return torch.stack(outs, 1)
