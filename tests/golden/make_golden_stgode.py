"""Golden vectors for the downstream STGODE predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_stgode.py          (build container only: needs /root/reference)
Imports reference model/STGODE/STGODE.py (ODEGCN) on the CPU, and ``get_normalized_adj`` / ``read_data`` of model/STGODE/args.py.

Stand-ins, placed in ``sys.modules`` before the reference is imported; nothing of the reference is changed or copied:
    torchdiffeq   is not installed.  The reference calls ``odeint(f, x, [0, 6], method='euler')[1]``: on a two-point grid that is ONE Euler step,
                  x + 6 f(0, x).  The stand-in module has exactly that ``odeint``.
    fastdtw       is not installed and args.py imports it at the top; it is only called where no DTW distance file exists, which never
                  happens here (the stand-in raises if it were).  So the reference's own DTW distances cannot be compared with here.
    np.float      args.py:120 uses the alias current numpy removed; it is put back for the duration of the call.
``read_data`` is run in a temporary directory laid out as it expects (``../data/STGODE/<name>/<name>_{dtw,spatial}_distance.npy`` next to a
small series file), so the thresholding is the reference's own code.

The model vectors are made in float64 (the reference model ``.double()``, parameters and input drawn in float32 first, so a float32 copy holds
the same values): relu and max decide discontinuously, and at float32 a rounding difference between two correct implementations can flip one.
Saves: the seeded initial state (the dead convolutions' weights in the compact form of golden_util.check); for dim_out 1 and 2, under the
xavier-style redraw (stgode_util.xavier_redraw_), the live state, x, w, y, dx and every parameter gradient of (y * w).sum() with the names of
the parameters without one, the running statistics after that one training forward, and the eval-mode output; ``get_normalized_adj`` and the
thresholding on a small pair; the reference's prefab PEMS08 distance matrices and the two graphs they give.  Only data is written
(tests/golden/stgode_small*.npz)."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "model"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import stgode_util as gu                                                        # noqa: E402
from golden_util import STRIDE, save                                            # noqa: E402

VARIANTS = {"do1": 1, "do2": 2}


def euler_stand_in():
    mod = types.ModuleType("torchdiffeq")

    def odeint(func, y0, t, method=None):
        assert method == "euler" and t.numel() == 2
        return torch.stack([y0, y0 + (t[1] - t[0]) * func(t[0], y0)])
    mod.odeint = mod.odeint_adjoint = odeint
    sys.modules["torchdiffeq"] = mod


def fastdtw_stand_in():
    mod = types.ModuleType("fastdtw")

    def fastdtw(*a, **k):
        raise RuntimeError("fastdtw is not installed: the generator never reaches it")
    mod.fastdtw = fastdtw
    sys.modules.setdefault("fastdtw", mod)


def reference_graph_functions():
    """(get_normalized_adj, thresholds(sp_dist, dtw_dist, sigma1, sigma2, thres1, thres2) -> (sp_matrix, dtw_matrix)) through the reference's
    own code, or (None, None) where args.py does not import"""
    fastdtw_stand_in()
    try:
        from STGODE import args as ref_args
    except Exception as e:                                                       # noqa: BLE001
        print("reference model/STGODE/args.py does not import here (%r): no graph vectors from it" % (e,))
        return None, None

    def thresholds(sp_dist, dtw_dist, sigma1, sigma2, thres1, thres2):
        n = sp_dist.shape[0]
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "work"))
            os.makedirs(os.path.join(tmp, "data", "STGODE", "X"))
            os.makedirs(os.path.join(tmp, "data", "X"))
            np.save(os.path.join(tmp, "data", "STGODE", "X", "X_dtw_distance.npy"), dtw_dist)
            np.save(os.path.join(tmp, "data", "STGODE", "X", "X_spatial_distance.npy"), sp_dist)
            np.savez(os.path.join(tmp, "data", "X", "X.npz"), data=np.random.RandomState(0).rand(8, n, 1))
            a = types.SimpleNamespace(filename="X", filepath=os.path.join(tmp, "data", "X") + "/", sigma1=sigma1, sigma2=sigma2, thres1=thres1,
                                      thres2=thres2)
            had = hasattr(np, "float")
            if not had:
                np.float = float
            os.chdir(os.path.join(tmp, "work"))
            try:
                _, _, _, dtw_matrix, sp_matrix = ref_args.read_data(a)
            finally:
                os.chdir(cwd)
                if not had:
                    del np.float
        return sp_matrix, dtw_matrix
    return ref_args.get_normalized_adj, thresholds


def main():
    euler_stand_in()
    from STGODE.STGODE import ODEGCN                                            # noqa: E402  (reference, read-only import)
    N, B, T, P, dim_in, L = 20, 2, 5, 3, 64, 3
    sp, se = gu.graphs(N)
    out = {"A_sp": sp.numpy(), "A_se": se.numpy(), "seed": np.int64(gu.SEED)}

    norm_adj, thresholds = reference_graph_functions()
    if norm_adj is not None:
        rng = np.random.RandomState(gu.SEED)
        spd = rng.rand(9, 9) * 1000
        spd[rng.rand(9, 9) < 0.3] = np.inf
        dtd = rng.rand(9, 9)
        dtd = dtd + dtd.T
        cfg = (0.5, 10.0, 0.3, 0.5)                                             # sigma1, sigma2, thres1, thres2
        spm, dtm = thresholds(spd, dtd, *cfg)
        out.update({"small.sp_dist": spd, "small.dtw_dist": dtd, "small.cfg": np.asarray(cfg), "small.sp_matrix": spm, "small.dtw_matrix": dtm,
                    "small.A_sp": norm_adj(spm).numpy(), "small.A_se": norm_adj(dtm).numpy()})
        zero_row = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 2.0], [0.5, 0.5, 0.0]])    # a node of degree 0: the floor decides
        out.update({"floor.A": zero_row, "floor.norm": norm_adj(zero_row).numpy()})
        d8, s8 = (np.load(os.path.join(REF, "data", "STGODE", "PEMS08", "PEMS08_%s_distance.npy" % k)) for k in ("dtw", "spatial"))
        spm8, dtm8 = thresholds(s8, d8, 0.1, 10.0, 0.6, 0.5)
        out.update({"pems08.dtw_dist": d8.astype(np.float32), "pems08.sp_dist": s8.astype(np.float32),
                    "pems08.A_sp": norm_adj(spm8).numpy(), "pems08.A_se": norm_adj(dtm8).numpy()})
        # the thresholds decide on float64 distances; stored as float32, an entry within rounding of a threshold could flip: count the margin
        spm32, dtm32 = thresholds(s8.astype(np.float32).astype(np.float64), d8.astype(np.float32).astype(np.float64), 0.1, 10.0, 0.6, 0.5)
        assert np.array_equal(spm32 > 0, spm8 > 0) and np.array_equal(dtm32, dtm8), "float32 storage of the PEMS08 distances moves a threshold"

    for tag, dim_out in VARIANTS.items():
        ap = gu.model_args(N, T=T, P=P, n_layers=L, g=(sp.double(), se.double()))     # (plain attributes there: .double() does not reach them)
        torch.manual_seed(gu.SEED)
        model = ODEGCN(ap, "cpu", dim_in, dim_out)                              # the seeded construction: tests rebuild it from SEED
        if tag == "do1":
            out["init.keys"] = np.asarray(list(model.state_dict().keys()))
            for k, v in model.state_dict().items():
                v = v.clone().numpy()
                if gu.is_dead(k) and not k.startswith("sp_blocks.0.0.temporal1."):
                    f = v.reshape(-1).astype(np.float64)
                    out["init." + k + "::sub"] = v.reshape(-1)[::STRIDE].copy()
                    out["init." + k + "::stats"] = np.asarray([f.sum(), np.abs(f).sum(), f.size])
                else:
                    out["init." + k] = v
        gu.xavier_redraw_(model)
        for k, v in model.state_dict().items():
            if not gu.is_dead(k):
                out[tag + ".sd." + k] = v.clone().numpy()
        x = torch.randn(B, T, N, dim_in).double().requires_grad_(True)
        w = torch.randn(B, P, N, dim_out).double()
        model.double().train()
        y = model(x)
        (y * w).sum().backward()
        out.update({tag + ".x": x.detach().numpy(), tag + ".w": w.numpy(), tag + ".y": y.detach().numpy(), tag + ".dx": x.grad.numpy()})
        nograd = []
        for k, p in model.named_parameters():
            if p.grad is None:
                nograd.append(k)
            else:
                out[tag + ".grad." + k] = p.grad.numpy()
        out[tag + ".nograd"] = np.asarray(nograd)
        for k, v in model.state_dict().items():
            if "running_" in k or "num_batches" in k:
                out[tag + ".run." + k] = v.clone().numpy()
        model.eval()
        with torch.no_grad():
            out[tag + ".y_eval"] = model(x).numpy()
        print(tag, "keys", len(model.state_dict()), "params", len(list(model.parameters())), "without grad", len(nograd), "y", tuple(y.shape),
              float(y.detach().abs().mean()))
    n = save("stgode_small.npz", out, HERE)
    print("wrote stgode_small.npz (%d shard(s)):" % n, len(out), "entries")


if __name__ == "__main__":
    main()
