"""Golden vectors for the downstream ASTGCN predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_astgcn.py          (build container only: needs /root/reference)
Imports reference model/ASTGCN/ASTGCN.py (ASTGCN, scaled_laplacian, cheb_polynomial) on the CPU.  Saves a non-symmetric adjacency, the reference's
scaled Laplacian (lambda_max from ARPACK) and polynomials, the seeded initial values of the parameters the constructor initialises (the
convolutions, the LayerNorms, final_conv: the others are uninitialised memory there), the state dict the vectors were made with, an input, the
output and the gradients of a scalar loss.  The parameter set is the reference Run.py's xavier pass followed by one move (astgcn_util.
move_score_vectors_): without it the second block's sigmoids saturate and no gradient reaches its score chain.  Only data is written
(tests/golden/astgcn_small.npz)."""
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

from ASTGCN.ASTGCN import ASTGCN, cheb_polynomial, scaled_laplacian            # noqa: E402  (reference, read-only import)
import astgcn_util as au                                                        # noqa: E402

SEED = 4321
SEEDED = ("time_conv", "residual_conv", "ln", "final_conv")


def main():
    N, B, T, dim_in, K, dim_out = 20, 3, 12, 64, 3, 1
    A = au.nonsymmetric_adjacency(N)
    L = scaled_laplacian(A)
    cheb = np.stack(cheb_polynomial(L, K))
    from gptst_amd import graph
    ours = graph.cheb_polynomials(graph.scaled_laplacian(A), K)
    print("ARPACK vs dense eigenvalues: max |L~ difference| %.3e, max |polynomial difference| %.3e"
          % (np.abs(graph.scaled_laplacian(A) - L).max(), np.abs(ours - cheb).max()))
    ap = au.model_args(N, None, K=K)
    ap.A = A
    torch.manual_seed(SEED)
    model = ASTGCN(ap, "cpu", dim_in, dim_out)                       # the seeded construction: tests rebuild it from SEED
    init = {k: v.clone().numpy() for k, v in model.state_dict().items() if k.split(".")[-2] in SEEDED}
    au.xavier_pass_(model)
    au.move_score_vectors_(model)
    x = torch.randn(B, T, N, dim_in, requires_grad=True)
    w = torch.randn(B, 12, N, dim_out)
    zs = []
    with au.recorded_sigmoids(zs):
        y = model(x)
    (y * w).sum().backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    print("share of sigmoid inputs in |z| < 4:", au.assert_condition(zs, grads))
    out = {"A": A, "L": np.asarray(L, dtype=np.float64), "cheb": cheb.astype(np.float64), "seed": np.int64(SEED), "x": x.detach().numpy(),
           "w": w.numpy(), "y": y.detach().numpy(), "dx": x.grad.numpy(),
           "lambda_diff": np.float64(np.abs(ours - cheb).max())}
    for k, v in model.state_dict().items():
        out["sd." + k] = v.numpy()
    for k, v in init.items():
        out["init." + k] = v
    for k, g in grads.items():
        out["grad." + k] = g.numpy()
    from golden_util import save                   # shards of < 1 MiB, read back by golden_util.load
    n = save("astgcn_small.npz", out, HERE)
    print("wrote astgcn_small.npz (%d shard(s)):" % n, len(out), "entries; y", tuple(y.shape), float(y.detach().abs().mean()))


if __name__ == "__main__":
    main()
