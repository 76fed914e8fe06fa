"""Golden vectors for the downstream STFGNN predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_stfgnn.py          (build container only: needs /root/reference)
Imports reference model/STFGNN/STFGNN.py (STFGNN) on the CPU, and ``construct_adj_fusion`` / ``compute_dtw`` of model/STFGNN/args.py.

The reference declares its two temporal convolutions as ``nn.Conv1d`` with 2-tuple kernels and applies them to 4-D input.  The PyTorch it was
written for ran that as a 2-D convolution; a current one refuses the input ("Expected 2D (unbatched) or 3D (batched) input to conv1d").  For the
duration of the reference's calls ``nn.Conv1d.forward`` is wrapped here so that a module with a 4-D weight goes through ``F.conv2d`` with the
module's own stride, padding and dilation: what the reference's PyTorch did.  Nothing of the reference is changed.

Saves the two graphs (S non-symmetric) and their fusion matrix, the seeded initial state, and for two variants (output_dim 1 and 2) the state
dict the vectors were made with — the position embeddings set to randn * 0.3: at their initial 1e-4 they would hide an omitted add — an input,
a weight tensor w, the output y, and dx and every parameter gradient of (y * w).sum().  Also ``construct_adj_fusion`` of a small 0/1 pair, the
DTW distances of a few small series pairs, and the reference's prefab PEMS08 fusion matrix as its two N x N blocks.  Only data is written
(tests/golden/stfgnn_small.npz)."""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "model"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import stfgnn_util as fu                                                        # noqa: E402

SEED = 1357
VARIANTS = {"do1": 1, "do2": 2}


@contextlib.contextmanager
def conv1d_runs_4d_weights_as_conv2d():
    real = nn.Conv1d.forward

    def forward(self, x):
        if self.weight.dim() == 4:
            return F.conv2d(x, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups)
        return real(self, x)
    nn.Conv1d.forward = forward
    try:
        yield
    finally:
        nn.Conv1d.forward = real


def main():
    from STFGNN.STFGNN import STFGNN                                            # noqa: E402  (reference, read-only import)
    N, B, T, P, dim_in = 20, 3, 9, 3, 64
    S, D = fu.graphs(N)
    out = {"S": S, "D": D, "seed": np.int64(SEED)}
    try:
        from STFGNN.args import compute_dtw, construct_adj_fusion               # pulls in pandas and the reference's lib
    except Exception as e:                                                       # noqa: BLE001
        print("reference model/STFGNN/args.py does not import here (%r): no fusion / DTW vectors" % (e,))
        compute_dtw = construct_adj_fusion = None
    if construct_adj_fusion is not None:
        adj = np.asarray(construct_adj_fusion(S, D, 4), dtype=np.float64)
        out["adj4"] = adj
        rng = np.random.RandomState(SEED)
        a01, d01 = (rng.rand(7, 7) < 0.3).astype(np.float64), (rng.rand(7, 7) < 0.3).astype(np.float64)
        d01 = np.maximum(d01, d01.T)
        np.fill_diagonal(d01, 1.0)
        out.update({"fusion.A": a01, "fusion.D": d01, "fusion.adj": np.asarray(construct_adj_fusion(a01, d01, 4), dtype=np.float64)})
        series = rng.rand(3, 24, 4) * 3 + np.sin(np.arange(24) / 4.0)[None, :, None]          # (days, slots, nodes)
        pairs = [(0, 1), (0, 3), (2, 3)]
        out.update({"dtw.series": series, "dtw.pairs": np.asarray(pairs), "dtw.band": np.int64(3),
                    "dtw.dist": np.asarray([compute_dtw(series[:, :, i], series[:, :, j], Ts=3) for i, j in pairs], dtype=np.float64)})
    else:
        from gptst_amd import graph
        adj = graph.stfgnn_fusion_graph(S, D).double().numpy()
    prefab = np.load(os.path.join(REF, "data", "STFGNN", "PEMS08", "PEMS08_adj_mx.npy"))
    n8 = prefab.shape[0] // 4
    assert set(np.unique(prefab)) <= {0.0, 1.0}
    out.update({"pems08.S": prefab[n8:2 * n8, n8:2 * n8].astype(np.uint8), "pems08.D": prefab[:n8, 3 * n8:].astype(np.uint8),
                "pems08.rowsum": prefab.sum(1).astype(np.int32), "pems08.colsum": prefab.sum(0).astype(np.int32)})
    for tag, dim_out in VARIANTS.items():
        ap = fu.model_args(N, torch.tensor(adj, dtype=torch.float32), T=T, P=P, output_dim=dim_out)
        torch.manual_seed(SEED)
        model = STFGNN(ap, dim_in)                                              # the seeded construction: tests rebuild it from SEED
        if tag == "do1":
            for k, v in model.state_dict().items():
                out["init." + k] = v.clone().numpy()
        fu.randomize_embeddings_(model)
        x = torch.randn(B, T, N, dim_in, requires_grad=True)
        w = torch.randn(B, P, N, dim_out)
        with conv1d_runs_4d_weights_as_conv2d():
            y = model(x)
            (y * w).sum().backward()
        out.update({tag + ".x": x.detach().numpy(), tag + ".w": w.numpy(), tag + ".y": y.detach().numpy(), tag + ".dx": x.grad.numpy()})
        for k, v in model.state_dict().items():
            out[tag + ".sd." + k] = v.numpy()
        for k, p in model.named_parameters():
            out[tag + ".grad." + k] = p.grad.numpy()
        print(tag, "keys", len(model.state_dict()), "y", tuple(y.shape), float(y.detach().abs().mean()))
    from golden_util import save                   # shards of < 1 MiB, read back by golden_util.load
    n = save("stfgnn_small.npz", out, HERE)
    print("wrote stfgnn_small.npz (%d shard(s)):" % n, len(out), "entries")


if __name__ == "__main__":
    main()
