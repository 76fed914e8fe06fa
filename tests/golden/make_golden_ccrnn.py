"""Golden vectors for the downstream CCRNN predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_ccrnn.py          (build container only: needs /root/reference; never run on a GPU machine)
Imports reference model/CCRNN_demand/CCRNN.py (EvoNN2) and args.py (preprocessing_for_metric) on the CPU; nothing of the reference is changed
or copied, and only data is written (tests/golden/ccrnn_small*.npz).

The support: the reference's args.py imports ``h5py``, which is not installed.  This script registers a small in-memory stand-in module of
its own under that name (``File(path, mode)`` as a context manager over a dict of arrays) so that ``preprocessing_for_metric`` runs
UNMODIFIED on ccrnn_util.series; what it returns is saved as ``sup.matrix``.

The model cases: (B, T, N, dim_in, dim_out) = (2, 12, 20, 64, 2), hidden_size 25, n_dim 10, k_hop 3, at the (n_rnn_layers, n_gconv_layers)
settings of ccrnn_util.LAYERS, each run with ``targets = None`` ("free") and with targets under ``random.seed(ccrnn_util.TF_SEED)`` ("tf").

Saves, per setting L<r><g>: the state-dict keys and the seeded initial state; the state the vectors were made with (``ccrnn_util.perturb_``);
per run y, dx and every parameter gradient of (y * w).sum(), made in float64 (parameters and inputs are drawn in float32 first, so a float32
copy holds the same values).  A gradient that is None is recorded as absent; ``<run>.none`` lists those keys."""
import contextlib
import io
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "model"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ccrnn_util as gu                                                         # noqa: E402
from golden_util import save                                                    # noqa: E402


def h5py_stand_in(files):
    """files: {path suffix: {dataset name: array}} -> a module that serves ``with h5py.File(path, 'r') as hf: hf[name][:]``"""
    mod = types.ModuleType("h5py")

    class File:
        def __init__(self, path, mode="r"):
            self._d = next(v for k, v in files.items() if str(path).endswith(k))

        def __enter__(self):
            return self._d

        def __exit__(self, *exc):
            return False

    mod.File = File
    return mod


def main():
    out = {"seed": np.int64(gu.SEED), "tf_seed": np.int64(gu.TF_SEED)}

    # ---- the support, by the reference's own function ----
    pick, drop = gu.series()
    sys.modules["h5py"] = h5py_stand_in({"NYC_TAXI/taxi_data.h5": {"taxi_pick": pick, "taxi_drop": drop}})
    from CCRNN_demand import args as ref_args                                   # noqa: E402  (reference, read-only import)
    h, hold = gu.SUPPORT_CASE["hidden_size_data"], gu.SUPPORT_CASE["holdout"]
    with contextlib.redirect_stdout(io.StringIO()):                             # Standard.fit prints its std and mean
        sup = ref_args.preprocessing_for_metric(["taxi"], "NYC_TAXI", h, "Standard", [hold // 2, hold - hold // 2], "randomwalk")
    out.update({"sup.pick": pick, "sup.drop": drop, "sup.matrix": np.asarray(sup, dtype=np.float64)})
    print("support", sup.shape, "row sums", float(sup.sum(1).min()), float(sup.sum(1).max()), "max", float(sup.max()))

    # ---- the model ----
    from CCRNN_demand.CCRNN import EvoNN2                                       # noqa: E402
    B, T, N, dim_in, dim_out = 2, 12, 20, 64, 2
    S = gu.support(N)
    out["support"] = S
    torch.manual_seed(gu.SEED)
    x32 = torch.randn(B, T, N, dim_in)
    w32 = torch.randn(B, T, N, dim_out)
    t32 = torch.randn(B, T, N, dim_out)
    out.update({"x": x32.numpy(), "w": w32.numpy(), "targets": t32.numpy()})
    for rnn, gconv in gu.LAYERS:
        tag = gu.tag(rnn, gconv)
        ap = gu.model_args(N, S, rnn=rnn, gconv=gconv)
        torch.manual_seed(gu.SEED)
        model = EvoNN2(ap, "cpu", dim_in, dim_out)                              # the seeded construction: tests rebuild it from SEED
        sd = model.state_dict()
        out[tag + ".init.keys"] = np.asarray(list(sd.keys()))
        for k, v in sd.items():
            out["%s.init.%s" % (tag, k)] = v.clone().numpy()
        gu.perturb_(model)
        for k, v in model.state_dict().items():
            out["%s.sd.%s" % (tag, k)] = v.clone().numpy()
        model.double().train()
        for run in ("free", "tf"):
            model.zero_grad(set_to_none=True)
            x = x32.double().requires_grad_(True)
            random.seed(gu.TF_SEED)
            state = random.getstate()
            y = model(x, t32.double() if run == "tf" else None, None)
            draws = 0                                                           # how many draws the forward consumed
            probe = random.getstate()
            random.setstate(state)
            while random.getstate() != probe:
                random.random()
                draws += 1
            (y * w32.double()).sum().backward()
            pre = "%s.%s." % (tag, run)
            out.update({pre + "y": y.detach().numpy(), pre + "dx": x.grad.numpy(), pre + "draws": np.int64(draws)})
            none = []
            for k, p in model.named_parameters():
                if p.grad is None:
                    none.append(k)
                else:
                    out[pre + "grad." + k] = p.grad.numpy().copy()
            out[pre + "none"] = np.asarray(none, dtype=str)
            print(tag, run, "keys", len(sd), "draws", draws, "mean |y|", float(y.detach().abs().mean()), "max |dx|", float(x.grad.abs().max()),
                  "None grads", none)
    n = save("ccrnn_small.npz", out, HERE)
    print("wrote ccrnn_small.npz (%d shard(s)):" % n, len(out), "entries")


if __name__ == "__main__":
    main()
