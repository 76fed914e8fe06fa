"""Golden vectors for the downstream MSDR predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_msdr.py          (build container only: needs /root/reference; never run on a GPU machine)
Imports reference model/MSDR/gmsdr_model.py (GMSDRModel) on the CPU and the graph functions of model/MSDR/args.py; nothing of the reference is
changed or copied, and only data is written (tests/golden/msdr_small*.npz).

The case: N = 20, B = 2, T = horizon = 12, dim_in = 64, rnn_units 64, two layers, pre_k 4, a non-symmetric adjacency, ``filter_type`` "2000"
(the value the reference's own default resolves to: one scaled Laplacian of max(A, A^T)).

Saves: the state-dict keys and the seeded state after ONE forward (the reference creates Theta and beta inside it: 34 keys before, 42 after);
the state the vectors were made with (``msdr_util.perturb_`` moves W, b and R off zero: at the initialisation every hidden state is exactly 0
and a broken kernel would pass); x, w, y, dx and every parameter gradient of (y * w).sum(), made in float64 (the reference model ``.double()``,
its sparse supports cast with it; parameters and input are drawn in float32 first, so a float32 copy holds the same values); the reference's
support matrices for "2000", ``dual_random_walk``, ``random_walk`` and ``laplacian`` (ARPACK's lambda_max) on that adjacency."""
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

import msdr_util as gu                                                          # noqa: E402
from golden_util import save                                                    # noqa: E402


def main():
    from MSDR.gmsdr_model import GMSDRModel                                     # noqa: E402  (reference, read-only import)
    from MSDR import args as ref_args                                           # noqa: E402
    N, B, T, dim_in, d, out_dim = 20, 2, 12, 64, 64, 1
    A = gu.adjacency(N)
    assert not np.array_equal(A, A.T)
    out = {"A": A, "seed": np.int64(gu.SEED)}
    out["sup.2000"] = np.asarray(ref_args.calculate_scaled_laplacian(A).todense())[None]
    out["sup.laplacian"] = np.asarray(ref_args.calculate_scaled_laplacian(A, lambda_max=None).todense())[None]
    out["sup.random_walk"] = np.asarray(ref_args.calculate_random_walk_matrix(A).T.todense())[None]
    out["sup.dual_random_walk"] = np.stack([np.asarray(ref_args.calculate_random_walk_matrix(A).T.todense()),
                                            np.asarray(ref_args.calculate_random_walk_matrix(A.T).T.todense())])

    ap = SimpleNamespace(adj_mx=torch.FloatTensor(A), max_diffusion_step=1, cl_decay_steps=2000, filter_type="2000", num_nodes=N,
                         num_rnn_layers=2, rnn_units=d, pre_k=4, pre_v=1, input_dim=dim_in, output_dim=out_dim, seq_len=T, horizon=T,
                         use_curriculum_learning=True)
    torch.manual_seed(gu.SEED)
    model = GMSDRModel(ap, "cpu")                                               # the seeded construction: tests rebuild it from SEED
    before = len(model.state_dict())
    with torch.no_grad():
        y0 = model(torch.zeros(B, T, N, dim_in))                                # the first forward creates Theta and beta (no other draw)
    sd = model.state_dict()
    print("keys before the first forward", before, "after", len(sd), "| y at the initialisation is the projection bias:",
          bool((y0 == model.decoder_model.projection_layer.bias).all()))
    out["init.keys"] = np.asarray(list(sd.keys()))
    for k, v in sd.items():
        out["init." + k] = v.clone().numpy()
    out["sup.cell"] = model.encoder_model.gmsdr_layers[0]._supports[0].to_dense().numpy()[None]       # what the cell itself built

    gu.perturb_(model)
    for k, v in model.state_dict().items():
        out["sd." + k] = v.clone().numpy()
    x = torch.randn(B, T, N, dim_in).double().requires_grad_(True)
    w = torch.randn(B, T, N, out_dim).double()
    model.double().train()
    for c in gu.cells(model):                                                   # plain attributes: .double() does not reach them
        c._supports = [s.double() for s in c._supports]
    y = model(x)
    (y * w).sum().backward()
    out.update({"x": x.detach().numpy(), "w": w.numpy(), "y": y.detach().numpy(), "dx": x.grad.numpy()})
    ngrad = 0
    for k, p in model.named_parameters():
        if p.grad is not None:
            out["grad." + k] = p.grad.numpy()
            ngrad += 1
    print("y", tuple(y.shape), "mean |y|", float(y.detach().abs().mean()), "max |h|-like", float(y.detach().abs().max()), "gradients", ngrad,
          "without one", sorted(k for k, p in model.named_parameters() if p.grad is None))
    n = save("msdr_small.npz", out, HERE)
    print("wrote msdr_small.npz (%d shard(s)):" % n, len(out), "entries")


if __name__ == "__main__":
    main()
