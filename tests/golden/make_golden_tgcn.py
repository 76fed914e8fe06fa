"""Golden vectors for the downstream TGCN predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_tgcn.py          (build container only: needs /root/reference)
Imports reference model/TGCN/TGCN.py (TGCN, calculate_normalized_laplacian) on the CPU; saves the seeded initial state_dict, the state_dict the vectors
were made with (the same with non-zero gate biases), a non-symmetric adjacency and the reference's normalised graph of it, an input, the output and the
gradients of a scalar loss.  Only data is written (tests/golden/tgcn_small.npz)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "model"))
sys.path.insert(0, REF)

from TGCN.TGCN import TGCN, calculate_normalized_laplacian                    # noqa: E402  (reference, read-only import)

SEED = 4321


def main():
    N, B, T, dim_in, H, dim_out = 20, 2, 12, 64, 100, 1
    rng = np.random.RandomState(11)
    A = (rng.rand(N, N) < 0.2).astype(np.float32)                    # non-symmetric: pins the reference's operand order in the normalisation
    np.fill_diagonal(A, 0)
    A[np.arange(N), (np.arange(N) + 1) % N] = 1                      # connected ring underneath
    assert not np.array_equal(A, A.T)
    L = np.asarray(calculate_normalized_laplacian(A).todense())
    ap = types.SimpleNamespace(adj_mx=A, num_nodes=N, output_dim=dim_out, rnn_units=H, lam=0.0015, input_window=T, output_window=T)
    torch.manual_seed(SEED)
    model = TGCN(ap, "cpu", dim_in)                                  # the seeded construction: tests rebuild it from SEED
    init = {k: v.clone().numpy() for k, v in model.state_dict().items()}
    with torch.no_grad():                                            # the initial biases are 0: move them so that the vectors see them
        for p in (model.tgcn_model.bias_0, model.tgcn_model.bias_1):
            p.add_(0.3 * torch.randn_like(p))
    x = torch.randn(B, T, N, dim_in, requires_grad=True)
    w = torch.randn(B, T, N, dim_out)
    y = model(x)
    (y * w).sum().backward()
    out = {"A": A, "L": L.astype(np.float64), "seed": np.int64(SEED), "x": x.detach().numpy(), "w": w.numpy(), "y": y.detach().numpy(),
           "dx": x.grad.numpy()}
    for k, v in model.state_dict().items():
        out["sd." + k] = v.numpy()
        out["init." + k] = init[k]
    for k, p in model.named_parameters():
        out["grad." + k] = p.grad.numpy()
    sys.path.insert(0, os.path.dirname(HERE))
    from golden_util import save                   # shards of < 1 MiB, read back by golden_util.load
    save("tgcn_small.npz", out, HERE)
    print("wrote tgcn_small.npz:", sorted(out), "y", y.shape, float(y.detach().abs().mean()))


if __name__ == "__main__":
    main()
