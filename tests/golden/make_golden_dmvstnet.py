"""Golden vectors for the downstream DMVSTNET predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_dmvstnet.py          (build container only: needs /root/reference; never run on a GPU machine)
Imports reference model/DMVSTNET_demand/DMVSTNET.py (DMVSTNet) on the CPU; nothing of the reference is changed or copied, and only data is
written (tests/golden/dmvstnet_small.npz).

The case: (B, T, N, dim_in, dim_out) = (2, 12, 20, 64, 2), hidden_dim 32 (so the LSTM is 64 wide), topo_embedded_dim 16, a dense random
non-negative adjacency with one all-zero row (dmvstnet_util.adjacency).

Saves: the seed and the adjacency; the state-dict keys and the seeded initial state; the state the vectors were made with
(``dmvstnet_util.perturb_``); x, w, y, dx and every parameter gradient of (y * w).sum(), made in float64 (parameters and input are drawn in
float32 first, so a float32 copy holds the same values); the keys that receive no gradient."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "model"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import dmvstnet_util as gu                                                      # noqa: E402
from golden_util import save                                                    # noqa: E402


def main():
    from DMVSTNET_demand.DMVSTNET import DMVSTNet                               # noqa: E402  (reference, read-only import)
    B, T, N, dim_in, dim_out = 2, 12, 20, 64, 2
    A = gu.adjacency(N)
    out = {"seed": np.int64(gu.SEED), "A": A}
    ap = gu.model_args(N, A, T=T, hidden=32, topo=16)
    torch.manual_seed(gu.SEED)
    model = DMVSTNet(ap, "cpu", dim_in, dim_out)                                # the seeded construction: tests rebuild it from SEED
    sd = model.state_dict()
    out["init.keys"] = np.asarray(list(sd.keys()))
    for k, v in sd.items():
        out["init." + k] = v.clone().numpy()
    gu.perturb_(model)
    for k, v in model.state_dict().items():
        out["sd." + k] = v.clone().numpy()
    x = torch.randn(B, T, N, dim_in).double().requires_grad_(True)
    w = torch.randn(B, T, N, dim_out).double()
    model.double().train()
    model.adj_mx = model.adj_mx.double()                                        # plain attributes: .double() does not reach them
    for g in (model.Local_GNN1, model.Local_GNN2, model.Local_GNN3):
        g.adj = model.adj_mx
    y = model(x)
    (y * w).sum().backward()
    out.update({"x": x.detach().numpy(), "w": w.numpy(), "y": y.detach().numpy(), "dx": x.grad.numpy()})
    none = []
    for k, p in model.named_parameters():
        if p.grad is None:
            none.append(k)
        else:
            out["grad." + k] = p.grad.numpy()
    out["nograd.keys"] = np.asarray(none)
    print("keys", len(sd), "no gradient:", none)
    print("y", tuple(y.shape), "mean |y|", float(y.detach().abs().mean()), "max |dx|", float(x.grad.abs().max()))
    n = save("dmvstnet_small.npz", out, HERE)
    print("wrote dmvstnet_small.npz (%d shard(s)):" % n, len(out), "entries")


if __name__ == "__main__":
    main()
