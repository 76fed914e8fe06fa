"""Unequal node shards (gpt-st_amd/shard.py) on CPU: the split of node_ranges, the flat-buffer layout of models built with a node capacity
(every rank's [flat gradient | statistics] must line up for the all-reduce), and — over a real 2-rank gloo group with N = 7 (shards of 4
and 3 nodes) — the ragged label gather and gather_state_dict."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import free_port  # noqa: E402
import torch.multiprocessing as mp

from gptst_amd import synth
from gptst_amd.config import make_args
from oracle import gptst_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(n, **kw):
    return make_args("PEMS08", num_nodes=n, embed_dim=4, HS=4, HT=4, scaler_zeros=synth.scaler_zeros(), **kw)


def test_node_ranges_cover_contiguously_with_widths_within_one():
    from gptst_amd.shard import node_ranges
    assert [b - a for a, b in node_ranges(170, 8)] == [22, 22, 21, 21, 21, 21, 21, 21]
    assert node_ranges(7, 2) == [(0, 4), (4, 7)]
    for N in (1, 7, 40, 170, 207, 266, 1000, 4096):
        for W in (1, 2, 3, 4, 7, 8, 16):
            if W > N:
                continue
            r = node_ranges(N, W)
            assert len(r) == W and r[0][0] == 0 and r[-1][1] == N
            assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
            w = [b - a for a, b in r]
            assert min(w) >= 1 and max(w) - min(w) <= 1 and w == sorted(w, reverse=True), (N, W, w)
    with pytest.raises(ValueError, match="3 nodes over 4 ranks"):
        node_ranges(3, 4)


def _dense_layout(model):
    """the flat layout without a node capacity, computed independently: segment order, 16-byte aligned true sizes"""
    from gptst_amd.model import _segment
    named = dict(model.named_parameters())
    order = sorted(named, key=lambda k: (_segment(k), model.param_keys.index(k)))
    offs, n = {}, 0
    for k in order:
        offs[k] = n
        n += (named[k].numel() + 3) // 4 * 4
    return offs, n


def test_capacity_gives_every_shard_the_same_layout():
    from gptst_amd.model import GPTST_Model
    from gptst_amd.shard import is_node_local
    a, b = GPTST_Model(_args(21, node_capacity=22)), GPTST_Model(_args(22, node_capacity=22))
    assert a.flat.numel() == b.flat.numel() and (a.nA, a.nB) == (b.nA, b.nB)
    assert a._offs == b._offs                                    # shared keys AND node-local slots
    shared = [k for k in a._offs if not is_node_local(k)]
    assert len(shared) > 100 and len(a._offs) - len(shared) == 9
    # the 22nd node's slot of the 21-node model is zero padding
    used = torch.zeros(a.flat.numel(), dtype=torch.bool)
    for k, t in a.named_parameters():
        used[a._offs[k]:a._offs[k] + t.numel()] = True
        assert t.data_ptr() == a.flat.data_ptr() + 4 * a._offs[k]
    assert int((~used).sum()) > 0 and float(a.flat[~used].abs().sum()) == 0.0
    # a 21-node model without a capacity is laid out differently: the all-reduce would sum unrelated parameters
    c = GPTST_Model(_args(21))
    assert any(c._offs[k] != b._offs[k] for k in shared)


def test_default_capacity_keeps_the_dense_layout():
    from gptst_amd.model import GPTST_Model
    for n in (21, 170):
        m0, m1 = GPTST_Model(_args(n)), GPTST_Model(_args(n, node_capacity=n))
        offs, total = _dense_layout(m0)
        assert m0._offs == offs and m1._offs == offs and m0.flat.numel() == total == m1.flat.numel()
        assert (m0.nA, m0.nB) == (m1.nA, m1.nB)


def test_capacity_keeps_state_dict_shapes_and_values():
    from gptst_amd.model import GPTST_Model
    sd = O.init_state_dict(_args(21), 3)
    m = GPTST_Model(_args(21, node_capacity=22))
    m.load_state_dict(sd)
    got = m.state_dict()
    assert list(got) == list(sd) and all(got[k].shape == sd[k].shape and torch.equal(got[k], sd[k]) for k in sd)
    assert got["encoder.neb4mask"].shape == (21, 4) and got["encoder.STHCN_encode.cap1.adj"].shape[-1] == 21


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from gptst_amd.model import GPTST_Model
    from gptst_amd.shard import DistNodeGroup, gather_node_columns, gather_state_dict, node_ranges, shard_state_dict
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        N, B, T = 7, 2, 3
        ranges = node_ranges(N, world)
        n0, n1 = ranges[rank]
        widths = [b - a for a, b in ranges]
        grp = DistNodeGroup(rank, world)
        glob = torch.arange(B * T * N, dtype=torch.int32).view(B, T, N)
        label_g = gather_node_columns(grp, glob[:, :, n0:n1].contiguous(), widths)            # what ShardedPretrainStep._gather_labels does
        sd = O.init_state_dict(_args(N), 4)
        m = GPTST_Model(_args(n1 - n0, node_capacity=max(widths)))
        m.load_state_dict(shard_state_dict(sd, n0, n1))
        back = gather_state_dict(grp, m.state_dict(), ranges)
        same = list(back) == list(sd) and all(back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]) for k in sd)
        q.put((rank, n1 - n0, label_g.tolist(), same))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_ragged_label_gather_and_checkpoint_gather_over_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    want = torch.arange(2 * 3 * 7, dtype=torch.int32).view(2, 3, 7).tolist()
    assert [w for _, w, _, _ in got] == [4, 3]
    for rank, _, lab, same in got:
        assert lab == want, rank
        assert same, "gather_state_dict did not give back the global state dict on rank %d" % rank
