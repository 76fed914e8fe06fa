"""Worker of tests/test_gpu_resume.py::test_data_parallel_run_resumes — one rank of a 2-rank gloo job on ONE GPU (deterministic mode).
Run A: Trainer.train() over two epochs (random-mask, then adaptive + KL; the epoch has padded tail rounds) with a checkpoint after each.
Run B: a new model with ANOTHER initialisation per rank and a new Trainer resume from A's epoch-1 file (rank 0 wrote it, both ranks read it) and
train epoch 2.  Rank 0 prints ONE JSON line."""
import hashlib
import json
import logging
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resume_util as U                         # noqa: E402
from gptst_amd import checkpoint as CK          # noqa: E402
from gptst_amd import data as D, synth          # noqa: E402
from gptst_amd.dist import DataParallel         # noqa: E402
from gptst_amd.model import GPTST_Model, init_seed, xavier_init_   # noqa: E402
from gptst_amd.trainer import Trainer           # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dp = DataParallel("gloo", native=False)
tmp = sys.argv[1]


def run(tag, seed, **kw):
    args = U.small_args(20, device=str(dev), batch_size=64, debug=False, epochs=2, change_epoch=1, steps_per_replay=2, ckpt_every=1,
                        ckpt_path=os.path.join(tmp, tag, "state_{epoch}.pth"), **kw)
    args.log_dir = os.path.join(tmp, tag, "rank%d" % dp.rank)
    raw = synth.make_series(20, 3, interval=5, days=8, seed=3)[:-5]
    train, _, _, scaler, _, _ = D.get_dataloader(args, raw=raw, device=dev, generator=torch.Generator().manual_seed(5))
    args.scaler_zeros = float(scaler.transform(0))
    init_seed(seed)
    model = xavier_init_(GPTST_Model(args)).to(dev)
    if not kw:
        dp.broadcast_(model.flat)               # (run B keeps its ranks' DIFFERENT weights: the file must replace them on both)
    batches, nb = D.epoch_batches(train, 64, dp)
    tr = Trainer(model, args, batches, float(scaler.mean), float(scaler.std), 64, dp=dp, batches_per_epoch=nb, loader=train)
    tr.logger.setLevel(logging.WARNING)
    avgs = {}
    plain = tr.train_epoch
    tr.train_epoch = lambda e: avgs.setdefault(e, plain(e))
    tr.train()
    torch.cuda.synchronize()
    h = hashlib.sha256(model.flat.detach().cpu().numpy().tobytes()).hexdigest()
    hs = [None] * dp.world
    dist.all_gather_object(hs, h)
    return tr, avgs, hs, nb


tr_a, avg_a, hs_a, nb = run("a", 3)
tr_b, avg_b, hs_b, _ = run("b", 4 + dp.rank, resume=os.path.join(tmp, "a", "state_1.pth"))
if dp.rank == 0:
    ck_a, ck_b = CK.load(os.path.join(tmp, "a", "state_2.pth")), CK.load(os.path.join(tmp, "b", "state_2.pth"))
    files = sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".pth"))
    print(json.dumps({"epochs_a": sorted(avg_a), "epochs_b": sorted(avg_b), "avg_a": avg_a[2], "avg_b": avg_b[2], "nb": nb,
                      "replicas_a": len(set(hs_a)) == 1, "replicas_b": len(set(hs_b)) == 1, "same_weights": hs_a[0] == hs_b[0],
                      "same_checkpoint": U.same_tree(ck_a, ck_b), "steps": [tr_a.step.tA, tr_a.step.tB, tr_b.step.tA, tr_b.step.tB],
                      "ragged": sorted(ck_a["rng"]["ragged_class_order"]), "files": files}))
dp.barrier()
dist.destroy_process_group()
