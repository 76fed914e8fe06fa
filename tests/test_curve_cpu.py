"""The oracle against the first steps of the reference's loss curve at the BASELINE configs[1] shape (tests/golden/curve_c2.npz):
full-size B=32, N=170, C=64 optimiser steps incl. clip + Adam, bit-exact masks.  (Later steps are not comparable pointwise:
the training is chaotic at lr 3e-3, see tests/test_gpu_curve.py.)"""
import os

import numpy as np
import torch

from gptst_amd import data as gdata, synth
from gptst_amd.config import make_args
from oracle import gptst_oracle as O
from golden_util import load


def test_oracle_tracks_reference_curve_first_steps():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    fx = load("curve_c2.npz")
    args = make_args("PEMS08", epochs=int(fx["epochs"]), change_epoch=int(fx["change_epoch"]), batch_size=32)
    raw = synth.make_series(args.num_nodes, 3, interval=5, seed=10)
    train, _, _, scaler, _, _ = gdata.get_dataloader(args, raw=raw)
    args.scaler_zeros = float(scaler.transform(0))
    sd = O.init_state_dict(args, int(fx["sd_seed"]))
    assert O.state_hash(sd) == str(fx["sd0_hash"])
    st = O.Stepper(sd, args, float(scaler.mean), float(scaler.std))
    B, M = 32, 32 * 12 * args.num_nodes
    for step in range(6):
        src = train.windows((torch.arange(B) * 7 + 13 * step) % train.n)[0]
        loss, lf, ls, outs, aux = st.step(src, int(fx["epoch"][step]), noise=synth.make_noise(M, int(fx["seeds"][step][0])))
        masked = torch.from_numpy(np.unpackbits(fx["masks"][step])[:M].astype(np.int64))
        assert torch.equal(outs[2].reshape(-1).long(), masked)
        assert abs(lf - fx["losses"][step, 1]) < 1e-5 * fx["losses"][step, 1], (step, lf, fx["losses"][step, 1])
