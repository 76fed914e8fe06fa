"""What the MSDR tests and the golden generator share (test_predictor_msdr.py, test_gpu_msdr_hip.py, golden/make_golden_msdr.py): a
non-symmetric adjacency, the argument set, and the move away from the initialisation every comparison starts with.

At initialisation W, b and R of every cell are zero: every hidden state is exactly 0, the output is the projection bias and every gradient
below the last layer is 0, so a comparison made there would pass on a broken kernel.  ``perturb_`` draws W ~ N(0, (1/32)^2) and
b, R ~ 0.1 N(0, 1) (a larger W lets the 48 stacked cell applications grow beyond what fp32 resolves)."""
from types import SimpleNamespace

import numpy as np
import torch

SEED = 11


def adjacency(N, seed=SEED, density=0.3):
    """(N, N) fp32, non-negative, NOT symmetric, every row and column with an entry"""
    rng = np.random.RandomState(seed)
    a = rng.rand(N, N) * (rng.rand(N, N) < density)
    a[np.arange(N), (np.arange(N) + 1) % N] = 0.5 + rng.rand(N)            # a directed ring: no empty row or column
    np.fill_diagonal(a, 0.0)
    return a.astype(np.float32)


def model_args(N, supports, T=12, horizon=12, d=64, layers=2, K=4, pre_v=1, mds=1, out=1):
    return SimpleNamespace(num_nodes=N, seq_len=T, horizon=horizon, rnn_units=d, num_rnn_layers=layers, pre_k=K, pre_v=pre_v,
                           max_diffusion_step=mds, output_dim=out, supports=supports)


def cells(model):
    return list(model.encoder_model.gmsdr_layers) + list(model.decoder_model.gmsdr_layers)


def perturb_(model):
    """moves W, b, R of every cell off zero, drawing from torch's global generator in the order of ``cells`` (works on the reference's
    model too: the attribute names are the same)"""
    with torch.no_grad():
        for c in cells(model):
            c.W.copy_(torch.randn(c.W.shape) / 32)
            c.b.copy_(0.1 * torch.randn(c.b.shape))
            c.R.copy_(0.1 * torch.randn(c.R.shape))
    return model

