"""Golden vectors for the downstream STSGCN predictor, generated from the REFERENCE implementation:
    python tests/golden/make_golden_stsgcn.py          (build container only: needs /root/reference)
Imports reference model/STSGCN/STSGCN.py (STSGCN, construct_adj) on the CPU.  The reference moves its position embeddings ``.to('cuda:0')``;
for the duration of the import and the constructions ``torch.Tensor.to`` is wrapped here so that this one destination becomes the CPU.  Saves a
non-symmetric row-normalised adjacency with a zero diagonal and its (3N, 3N) ``construct_adj`` matrix, the seeded initial state, and for three
variants (``individual``, ``sharing``, dim_out = 2) the state dict the vectors were made with — the position embeddings set to randn * 0.3: at
their initial zero they would hide an omitted add — an input, a weight tensor w, the output y, and dx and every parameter gradient of
(y * w).sum().  Also about 200 (pred, true) pairs with the reference ``huber_loss`` of them.  Only data is written
(tests/golden/stsgcn_small.npz)."""
import contextlib
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

import stsgcn_util as su                                                        # noqa: E402

SEED = 2468
VARIANTS = {"ind": ("individual", 1), "sha": ("sharing", 1), "do2": ("individual", 2)}


@contextlib.contextmanager
def cuda0_is_cpu():
    real = torch.Tensor.to

    def to(self, *args, **kw):
        if args and isinstance(args[0], str) and args[0].startswith("cuda"):
            args = ("cpu",) + tuple(args[1:])
        return real(self, *args, **kw)
    torch.Tensor.to = to
    try:
        yield
    finally:
        torch.Tensor.to = real


def main():
    with cuda0_is_cpu():
        from STSGCN.STSGCN import STSGCN, construct_adj                         # noqa: E402  (reference, read-only import)
    from lib.metrics import huber_loss
    N, B, T, P, dim_in = 20, 3, 6, 3, 64
    A = su.adjacency(N)
    out = {"A": A, "adj3": np.asarray(construct_adj(A, 3), dtype=np.float64), "seed": np.int64(SEED)}
    for tag, (module_type, dim_out) in VARIANTS.items():
        ap = su.model_args(N, A, T=T, P=P, module_type=module_type)
        torch.manual_seed(SEED)
        with cuda0_is_cpu():
            model = STSGCN(ap, "cpu", dim_in, dim_out)                          # the seeded construction: tests rebuild it from SEED
        if tag == "ind":
            for k, v in model.state_dict().items():
                out["init." + k] = v.clone().numpy()
        su.randomize_embeddings_(model)
        x = torch.randn(B, T, N, dim_in, requires_grad=True)
        w = torch.randn(B, P, N, dim_out)
        y = model(x)
        (y * w).sum().backward()
        out.update({tag + ".x": x.detach().numpy(), tag + ".w": w.numpy(), tag + ".y": y.detach().numpy(), tag + ".dx": x.grad.numpy()})
        for k, v in model.state_dict().items():
            out[tag + ".sd." + k] = v.numpy()
        for k, p in model.named_parameters():
            out[tag + ".grad." + k] = p.grad.numpy()
        print(tag, "keys", len(model.state_dict()), "y", tuple(y.shape), float(y.detach().abs().mean()))
    # the loss: residuals on both sides of delta = 1, and cells at or below the mask threshold 0.001
    g = torch.Generator().manual_seed(SEED)
    true = torch.rand(200, generator=g, dtype=torch.float64) * 4
    true[::9] = 0.0
    true[4::17] = 0.001
    pred = true + torch.randn(200, generator=g, dtype=torch.float64) * 1.5
    pred[7], pred[8] = true[7] + 1.0, true[8] - 1.0                              # exactly at delta
    res = (pred - true).abs()[true > 0.001]
    assert int((res < 1).sum()) > 40 and int((res > 1).sum()) > 40 and int((true <= 0.001).sum()) > 20
    out.update({"huber.pred": pred.numpy(), "huber.true": true.numpy(), "huber.thresh": np.float64(0.001),
                "huber.loss": np.float64(huber_loss(pred, true, mask_value=0.001)[0]),
                "huber.loss_delta2": np.float64(huber_loss(pred, true, mask_value=0.001, delta=2.0)[0]),
                "huber.loss_nomask": np.float64(huber_loss(pred, true, mask_value=-1.0)[0])})
    from golden_util import save                   # shards of < 1 MiB, read back by golden_util.load
    n = save("stsgcn_small.npz", out, HERE)
    print("wrote stsgcn_small.npz (%d shard(s)):" % n, len(out), "entries")


if __name__ == "__main__":
    main()
