"""Worker of tests/test_gpu_run_shard.py::test_lost_handoff_on_one_rank_is_rerun_on_every_rank — one rank of a 2-rank gloo job on ONE GPU,
node-sharded (N = 41: shards of 21 and 20 nodes).  Three adaptive-phase steps, twice from the same weights: once plain, once with a hand-off
expiry put on record on rank 1 ALONE before the second step (a record, not a fault: gptst_handoff_inject).  Every rank prints one JSON line."""
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gptst_amd import _C, synth                 # noqa: E402
from gptst_amd.config import make_args         # noqa: E402
from gptst_amd.model import GPTST_Model         # noqa: E402
from gptst_amd.shard import DistNodeGroup, ShardedPretrainStep, is_node_local, node_ranges, shard_state_dict   # noqa: E402
from oracle import gptst_oracle as O            # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
N, B = 41, 2
over = dict(num_route=2, scaler_zeros=synth.scaler_zeros(), epochs=30, change_epoch=3, embed_dim=8, HS=5, HT=6)
ranges = node_ranges(N, world)
n0, n1 = ranges[rank]
sd = O.init_state_dict(make_args("PEMS08", num_nodes=N, **over), 8)
args_l = make_args("PEMS08", num_nodes=n1 - n0, node_capacity=max(b - a for a, b in ranges), **over)
srcs = [synth.make_batch(B, 12, N, 1, seed=80 + s)[:, :, n0:n1].contiguous().to(dev) for s in range(3)]
orders = [synth.class_order(5, 5 + s) for s in range(3)]
group = DistNodeGroup(rank, world)
res = []
try:
    for lose in (False, True):
        m = GPTST_Model(args_l)
        m.load_state_dict(shard_state_dict(sd, n0, n1))
        m = m.to(dev)
        st = ShardedPretrainStep(m, args_l, N, group, synth.SCALER_MEAN, synth.SCALER_STD, batch_size=B)
        losses = []
        for i, (src, lc) in enumerate(zip(srcs, orders)):
            if lose and i == 1 and rank == 1:
                torch.cuda.synchronize()
                _C.lib().call("gptst_handoff_inject", 1)
            st.step(src, 20, list_c=lc)
            losses.append(st.losses())
        res.append(dict(losses=losses, lost=st.lost_steps, safe=st.safe_mode, t=[st.tA, st.tB], flat=m.flat.detach().clone()))
finally:
    _C.lib().call("gptst_handoff_reset")
plain, lost = res
# the shared parameters after the re-run: the same on both ranks (one of them is the narrower shard, with capacity padding)
shared = torch.cat([v.reshape(-1) for k, v in m.state_dict().items() if not is_node_local(k)])
both = group.all_gather(shared)
shared_diff = float((both[0] - both[1]).abs().max())
# (one write per rank: both ranks share the parent's pipe, and print() writes the text and the newline separately — two records landed on one line)
sys.stdout.write(json.dumps({"rank": rank, "lost_steps": [plain["lost"], lost["lost"]], "safe_mode": [plain["safe"], lost["safe"]],
                  "counters": [plain["t"], lost["t"]], "losses": [plain["losses"], lost["losses"]],
                  "param_rel": float((plain["flat"] - lost["flat"]).norm() / plain["flat"].norm()), "shared_diff": shared_diff}) + "\n")
sys.stdout.flush()
dist.barrier()
dist.destroy_process_group()
