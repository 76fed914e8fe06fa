"""Golden vectors for the downstream MTGNN predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_mtgnn.py          (build container only: needs /root/reference)
Imports reference model/MTGNN/MTGNN.py on the CPU; saves the seeded initial state_dict, the state_dict the vectors were made with (the same
with biases and LayerNorm weights moved off their 0 / 1 initial values and the node embeddings moved so that no top-k cut of the graph is a tie: tests/mtgnn_util.py), the adjacency, an input, the eval-mode output and the gradients of a
scalar loss, and one training-mode case with dropout 0.3 drawn after ``torch.manual_seed`` (it pins the order in which the random stream is
consumed).  N = 20 with subgraph_size 8 so that the top-k cuts, output_dim 2 so that the T = 2 + T = 1 skip sum broadcasts, reduced widths.
Only data is written (tests/golden/mtgnn_small.npz)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "model"))
sys.path.insert(0, REF)

from MTGNN.MTGNN import MTGNN                                                  # noqa: E402  (reference, read-only import)

SEED, TRAIN_SEED = 2468, 97
CFG = dict(num_nodes=20, input_window=12, output_window=12, output_dim=2, gcn_true=True, buildA_true=True, gcn_depth=2, dropout=0.3,
           subgraph_size=8, node_dim=40, dilation_exponential=1, conv_channels=16, residual_channels=16, skip_channels=16, end_channels=32,
           layers=3, propalpha=0.05, tanhalpha=3, layer_norm_affline=True, use_curriculum_learning=True, task_level=0)
DIM_IN, B = 16, 2


def run(model, x0, w, tag, out):
    x = x0.clone().requires_grad_(True)
    model.zero_grad()
    y = model(x)
    (y * w).sum().backward()
    out[tag + "y"], out[tag + "dx"] = y.detach().numpy(), x.grad.numpy()
    for k, p in model.named_parameters():
        if p.grad is not None:                                        # residual_convs.* get none
            out[tag + "grad." + k] = p.grad.clone().numpy()
    return y


def main():
    N, K = CFG["num_nodes"], CFG["subgraph_size"]
    rng = np.random.RandomState(11)
    A = (rng.rand(N, N) < 0.2).astype(np.float32)
    np.fill_diagonal(A, 1)
    ap = types.SimpleNamespace(adj_mx=A, **CFG)
    torch.manual_seed(SEED)
    model = MTGNN(ap, "cpu", DIM_IN, CFG["output_dim"])              # the seeded construction: tests rebuild it from SEED
    init = {k: v.clone().numpy() for k, v in model.state_dict().items()}
    with torch.no_grad():                                            # LayerNorm starts at weight 1 / bias 0: move them, and every bias, so that
        for k, p in model.named_parameters():                        # the vectors see them
            if k.startswith("norm.") or k.endswith(".bias"):
                p.add_(0.2 * torch.randn_like(p))
    sys.path.insert(0, os.path.dirname(HERE))
    from mtgnn_util import clear_topk_cuts, cut_gaps                 # no top-k cut of the learned graph is a tie (what differs between devices)
    gap = clear_topk_cuts(model.gc, K)
    print("smallest gap at a top-k cut %.2e over %d rows that cut among positive values" % (gap, cut_gaps(model.gc, K)[1]))
    x = torch.randn(B, CFG["input_window"], N, DIM_IN)
    w = torch.randn(B, CFG["output_window"], N, CFG["output_dim"])
    out = {"A": A, "seed": np.int64(SEED), "train_seed": np.int64(TRAIN_SEED), "x": x.numpy(), "w": w.numpy()}
    model.eval()
    y = run(model, x, w, "", out)
    model.train()
    torch.manual_seed(TRAIN_SEED)
    yt = run(model, x, w, "train.", out)
    assert float((y - yt).detach().abs().max()) > 1e-2               # the dropout was active
    for k, v in model.state_dict().items():
        out["sd." + k] = v.numpy()
        out["init." + k] = init[k]
    from golden_util import save                   # shards of < 1 MiB, read back by golden_util.load
    n = save("mtgnn_small.npz", out, HERE)
    print("wrote mtgnn_small.npz in %d shard(s):" % n, len(out), "entries, y", tuple(y.shape), float(y.detach().abs().mean()))


if __name__ == "__main__":
    main()
