"""`Run.py -mode pretrain -shard nodes` under torch.distributed.run: three gloo ranks on ONE GPU train a small PEMS08-shaped series with
N = 40 nodes (shards of 14, 13 and 13) for two epochs — random-mask, then adaptive + KL — and must agree with the same command run unsharded
in one process: per-epoch losses, log lines from rank 0 only, a checkpoint in the unsharded run's format.  And a lost in-launch hand-off on
ONE rank of a node-sharded job: every rank skips the update and re-runs the step (tests/shard_handoff_worker.py)."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import free_port  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "gpt-st_amd", "SAVE", "PEMS08", "new_pretrain_model.pth")
# (the unsharded reference run steps one batch per graph replay: -steps_per_replay 1; the sharded stepper always does)
FLAGS = ["-dataset", "PEMS08", "-mode", "pretrain", "-num_nodes", "40", "-batch_size", "16", "-epochs", "2", "-change_epoch", "1",
         "-debug", "True", "-steps_per_replay", "1"]
LOSS_RE = re.compile(r"Train Epoch (\d+): averaged Loss: ([0-9.eE+-]+)")
STEP0_RE = re.compile(r"Train Epoch 1: 0/\S+ Loss: ([0-9.eE+-]+)")
CKPT_BOUND, CKPT_BOUND_T_ADJ = 0.15, 0.3


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GPTST_DETERMINISTIC="1", **kw)
    return env


@pytest.fixture
def keep_user_checkpoint(tmp_path):
    """Run.py writes its checkpoint to a fixed place in the tree: a file a user left there is moved aside for the test and put back after it;
    the test's own checkpoints are removed"""
    aside = tmp_path / "user_checkpoint.pth"
    had = os.path.exists(CKPT)
    if had:
        shutil.move(CKPT, aside)
    try:
        yield
    finally:
        if os.path.exists(CKPT):
            os.remove(CKPT)
        if had:
            shutil.move(aside, CKPT)


def _run(cmd, env):
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    log = r.stdout + r.stderr
    assert os.path.exists(CKPT), log[-3000:]
    ck = torch.load(CKPT, map_location="cpu")
    os.remove(CKPT)
    return log, ck


def test_run_py_node_shards_match_the_unsharded_run(tmp_path, parity, keep_user_checkpoint):
    from gptst_amd import synth
    from gptst_amd.config import make_args
    from gptst_amd.model import GPTST_Model
    os.makedirs(tmp_path / "PEMS08")
    np.savez(tmp_path / "PEMS08" / "PEMS08.npz", data=synth.make_series(40, 3, interval=5, days=2, seed=3))     # 576 steps: 21 batches
    flags = FLAGS + ["-data_root", str(tmp_path)]
    run_py = os.path.join(ROOT, "gpt-st_amd", "Run.py")
    ref_log, ref_ck = _run([sys.executable, run_py] + flags, _env())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), run_py] + flags + ["-shard", "nodes"]
    log, ck = _run(cmd, _env(GPTST_DIST_BACKEND="gloo"))

    ref = [float(v) for _, v in LOSS_RE.findall(ref_log)]
    got = LOSS_RE.findall(log)
    assert [int(e) for e, _ in got] == [1, 2], log[-3000:]                # one line per epoch: rank 0 alone logs
    assert log.count("Train Epoch 1: 0/") == 1, log[-3000:]
    assert log.count("Saving current best model") == 1 and log.count("Average Horizon") == 1, log[-3000:]
    assert len(ref) == 2
    # the first step starts from the same weights with the same mask: data columns, initialisation and scaler are those of the unsharded run
    first, first_ref = (float(STEP0_RE.search(s).group(1)) for s in (log, ref_log))
    e0 = abs(first - first_ref) / abs(first_ref)
    parity("first_step_loss_rel", e0)
    assert e0 < 2e-4, (first, first_ref)
    # Epoch averages then follow two fp32 trajectories (other summation order over the nodes).  Measured: 6.9e-6 after the random-mask
    # epoch (21 Adam steps); 1.2e-2 and 1.4e-2 (two runs) after the adaptive epoch, whose masks follow the argmax of the cluster classifier.
    for (ep, v), r, bound in zip(got, ref, (1e-4, 3e-2)):
        e = abs(float(v) - r) / abs(r)
        parity("epoch%s_loss_rel" % ep, e)
        assert e < bound, (got, ref)

    assert list(ck) == list(ref_ck) and all(ck[k].shape == ref_ck[k].shape for k in ck)
    m = GPTST_Model(make_args("PEMS08", num_nodes=40))
    m.load_state_dict(ck)
    # the weights themselves (node-local tensors assembled from all three ranks, shared ones from rank 0): per tensor, rel-L2 to the unsharded
    # run's.  cap*.t_adj apart: its gradient is a difference of products summed over the nodes, round-off that Adam turns into steps of up to
    # +-lr (tests/test_gpu_shard.py).  Measured after 42 steps (two runs): 0.137 for t_adj, 8.7e-2 for the worst other tensor (decoder hyperTem1
    # weights_pool) — the adaptive epoch's masks follow the classifier's argmax, and its 21 steps move the two runs apart.  A wrong node order
    # or shard in the gathered checkpoint would be O(1).
    worst = {False: (0.0, None), True: (0.0, None)}
    for k, v in ref_ck.items():
        e = float((ck[k] - v).norm()) / max(float(v.norm()), 1e-12)
        t = k.endswith(".t_adj")
        if e > worst[t][0]:
            worst[t] = (e, k)
    parity("checkpoint_rel_l2_worst", worst[False][0])
    parity("checkpoint_rel_l2_worst_t_adj", worst[True][0])
    assert worst[False][0] < CKPT_BOUND, worst
    assert worst[True][0] < CKPT_BOUND_T_ADJ, worst


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused_heads", "unfused_heads"])
def test_lost_handoff_on_one_rank_is_rerun_on_every_rank(fused):
    """fused_heads: the expiry reaches the other rank through the statistics the loss heads fold into the all-reduced buffer; unfused_heads
    (GPTST_SHARD_FUSED=0): through the zero-row fold the unfused path enqueues for it"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "shard_handoff_worker.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(GPTST_DIST_BACKEND="gloo", GPTST_SHARD_FUSED=fused), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    outs = sorted((json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")), key=lambda o: o["rank"])
    assert [o["rank"] for o in outs] == [0, 1], r.stdout[-2000:]
    for o in outs:
        assert o["lost_steps"] == [0, 1] and o["safe_mode"] == [False, True], o
        assert o["counters"] == [[3, 3], [3, 3]], o
        assert o["param_rel"] < 1e-3, o
        assert o["shared_diff"] <= 1e-6, o
        for a, b in zip(*o["losses"]):
            for x, y in zip(a, b):
                assert abs(x - y) <= 2e-4 * max(abs(y), 1e-3), o
