"""Golden vectors for the downstream ST-MGCN predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_stmgcn.py          (build container only: needs /root/reference; never run on a GPU machine)
Imports reference model/STMGCN_demand/STMGCN.py (ST_MGCN) and GCN.py (Adj_Preprocessor) on the CPU; nothing of the reference is changed or
copied, and only data is written (tests/golden/stmgcn_small.npz).

The case: (B, T, N, dim_in, dim_out) = (2, 12, 20, 64, 2), H = 64, three LSTM layers, a distance-like graph whose last node is isolated and
a correlation-like graph whose node 0 has a negative row sum (stmgcn_util.graphs), each through ``Adj_Preprocessor('chebyshev', 2).process``
and ``nan_to_num`` as model/STMGCN_demand/args.py:43-51 does.

Saves: the seed, the raw graphs and both support stacks; the state-dict keys and the seeded initial state; the state the vectors were made
with (``stmgcn_util.perturb_``); x, w, y, dx and every parameter gradient of (y * w).sum(), made in float64 (parameters and input are drawn
in float32 first, so a float32 copy holds the same values)."""
import contextlib
import io
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

import stmgcn_util as gu                                                        # noqa: E402
from golden_util import save                                                    # noqa: E402


def main():
    from STMGCN_demand.STMGCN import ST_MGCN                                    # noqa: E402  (reference, read-only import)
    from STMGCN_demand.GCN import Adj_Preprocessor                              # noqa: E402
    B, T, N, dim_in, dim_out = 2, 12, 20, 64, 2
    dis, pcc = gu.graphs(N)
    pre = Adj_Preprocessor(kernel_type="chebyshev", K=2)
    said = io.StringIO()
    with contextlib.redirect_stdout(said):                                      # the line rescale_laplacian prints when torch.eig raises
        sup = [torch.nan_to_num(pre.process(torch.FloatTensor(g))) for g in (dis, pcc)]
    print("the reference said:", sorted(set(said.getvalue().strip().splitlines())))
    out = {"seed": np.int64(gu.SEED), "dis": dis, "pcc": pcc, "sup.dis": sup[0].numpy(), "sup.pcc": sup[1].numpy()}
    for k in ("sup.dis", "sup.pcc"):
        print(k, "max", float(np.abs(out[k]).max()), "zeros per support", [int((s == 0).sum()) for s in out[k]])

    ap = SimpleNamespace(M=2, seq_len=T, n_nodes=N, lstm_hidden_dim=64, lstm_num_layers=3, gcn_hidden_dim=64, gconv_use_bias=True,
                         sta_kernel_config={"kernel_type": "chebyshev", "K": 2}, dis_graph=sup[0], pcc_graph=sup[1])
    torch.manual_seed(gu.SEED)
    model = ST_MGCN(ap, "cpu", dim_in, dim_out)                                 # the seeded construction: tests rebuild it from SEED
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
    model.sta_adj_list = [g.double() for g in model.sta_adj_list]               # plain attributes: .double() does not reach them
    y = model(x)
    (y * w).sum().backward()
    out.update({"x": x.detach().numpy(), "w": w.numpy(), "y": y.detach().numpy(), "dx": x.grad.numpy()})
    for k, p in model.named_parameters():
        out["grad." + k] = p.grad.numpy()
    print("keys", len(sd), "y", tuple(y.shape), "mean |y|", float(y.detach().abs().mean()), "max |dx|", float(x.grad.abs().max()))
    n = save("stmgcn_small.npz", out, HERE)
    print("wrote stmgcn_small.npz (%d shard(s)):" % n, len(out), "entries")


if __name__ == "__main__":
    main()
