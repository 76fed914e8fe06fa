"""Golden vectors for the downstream ST-WA predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_stwa.py          (build container only: needs /root/reference; never run on a GPU machine)
Imports reference model/ST_WA/ST_WA.py (STWA) on the CPU; nothing of the reference is changed or copied, and only data is written
(tests/golden/stwa_small*.npz).

Case A: N = 20, B = 2, lag = horizon = 12, dim_in = 64, C = M = 16, out_dim 1.
Case B: N = 13, B = 3, lag = 8 (a partial cut: cut 1 of the first layer has 2 rows), horizon 12, dim_in = 64, out_dim 2 (the other reshape).

Saves per case (keys ``A.*`` / ``B.*``): the state-dict keys and the seeded state (``init.*``); the state the vectors were made with
(``sd.*``, for the keys stwa_util.perturb_ moved to sharpen the spatial softmax; every other key keeps its ``init.*`` value); the four noise
tensors, recorded by wrapping ``torch.randn_like`` around the reference's float32 forward under ``manual_seed(noise_seed)``; x, w, y, dx and
every parameter gradient of (y * w).sum(), made in float64
(the reference model ``.double()``; parameters, input and noise are drawn in float32 first, so a float32 copy holds the same values).
Asserts on the reference itself: the mean largest spatial weight of a row >= 1.5 / N and fp32 against fp64 <= 2e-5."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "model"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import stwa_util as su                                                          # noqa: E402
from golden_util import save                                                    # noqa: E402

NOISE_SEED = 5


class _Randn:
    """torch.randn_like, recording what it returns (replay = None) or returning the recorded tensors in the dtype asked for"""

    def __init__(self, replay=None):
        self.real, self.seen, self.replay = torch.randn_like, [], replay

    def __call__(self, t):
        e = self.real(t) if self.replay is None else self.replay[len(self.seen)].to(t.dtype)
        assert e.shape == t.shape
        self.seen.append(e)
        return e

    def __enter__(self):
        torch.randn_like = self
        return self

    def __exit__(self, *a):
        torch.randn_like = self.real


def _run(model, x, w, replay, probe=None):
    hooks = []
    if probe is not None:
        def pre(mod, inp):
            o, params = inp
            hs = mod.head_size
            k = torch.cat(torch.split(mod.linear(o, params[0]), hs, dim=-1), dim=0)
            q = torch.cat(torch.split(o, hs, dim=-1), dim=0)
            probe.append(torch.softmax(torch.matmul(q, k.transpose(2, 3)) / hs ** 0.5, dim=-1).detach())
        hooks = [l.spatial_att.register_forward_pre_hook(pre) for l in model.layers]
    model.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    with _Randn(replay) as r:
        y = model(x)
    for h in hooks:
        h.remove()
    (y * w).sum().backward()
    return y.detach(), x.grad.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}, r.seen


def case(tag, out, N, B, lag, out_dim, dim_in=64, C=16, M=16, horizon=12):
    from ST_WA.ST_WA import STWA                                                # noqa: E402  (reference, read-only import)
    ap = SimpleNamespace(adj_mx=[np.eye(N)], num_nodes=N, out_dim=out_dim, channels=C, dynamic="True", horizon=horizon, lag=lag,
                         memory_size=M)
    torch.manual_seed(su.SEED)
    model = STWA(ap, "cpu", dim_in)                                             # the seeded construction: tests rebuild it from SEED
    sd = model.state_dict()
    out[tag + ".init.keys"] = np.asarray(list(sd.keys()))
    for k, v in sd.items():
        out[tag + ".init." + k] = v.clone().numpy()
    su.perturb_(model)
    for k, v in model.state_dict().items():                                     # only what perturb_ moved: the rest of the state is init.*
        if not np.array_equal(v.numpy(), out[tag + ".init." + k]):
            out[tag + ".sd." + k] = v.clone().numpy()
    x, w = torch.randn(B, lag, N, dim_in), torch.randn(B, horizon, N, out_dim)
    model.train()
    torch.manual_seed(NOISE_SEED)
    y32, dx32, g32, nz = _run(model, x, w, None)                                # float32: records the noise, in the reference's order of draws
    assert [tuple(e.shape) for e in nz] == [(B, N, M)] + [(N, M)] * 3
    probe = []
    y, dx, g, _ = _run(model.double(), x.double(), w.double(), nz, probe)
    sharp = float(torch.stack([p.max(dim=-1).values.mean() for p in probe]).mean()) * N
    gmax = max(float(v.abs().max()) for v in g.values())
    e, zero, nz_grads = max(su.err(y32, y), su.err(dx32, dx)), 0.0, 0
    for k in g:
        if su.degenerate(k):
            zero = max(zero, float(g32[k].abs().max()) / gmax, float(g[k].abs().max()) / gmax)
        else:
            assert float(g[k].abs().max()) > 0, k
            e, nz_grads = max(e, su.err(g32[k], g[k])), nz_grads + 1
    print("case", tag, "keys", len(sd), "y", tuple(y.shape), "sharpness x N %.3f" % sharp, "fp32 vs fp64 %.2e" % e,
          "degenerate / largest gradient %.2e" % zero, "largest gradient %.3g" % gmax, "non-degenerate", nz_grads)
    assert sharp >= su.SHARP and e <= su.FP32 and zero <= su.ZERO / 10
    out.update({tag + ".x": x.numpy(), tag + ".w": w.numpy(), tag + ".y": y.numpy(), tag + ".dx": dx.numpy(),
                tag + ".eps_d": nz[0].numpy(), tag + ".noise_seed": np.int64(NOISE_SEED)})
    for i, e_l in enumerate(nz[1:]):
        out[tag + ".eps_l%d" % i] = e_l.numpy()
    for k, v in g.items():
        out[tag + ".grad." + k] = v.numpy()


def main():
    out = {"seed": np.int64(su.SEED)}
    case("A", out, N=20, B=2, lag=12, out_dim=1)
    case("B", out, N=13, B=3, lag=8, out_dim=2)
    n = save("stwa_small.npz", out, HERE)
    print("wrote stwa_small.npz (%d shard(s)):" % n, len(out), "entries")


if __name__ == "__main__":
    main()
