"""GPU: a pretraining run continued from a checkpoint is THE SAME run (gpt-st_amd/checkpoint.py, PretrainStep / ShardedPretrainStep
state_dict / load_state_dict, Trainer.save_state / load_state).  With fixed-order reductions (deterministic mode) a step sequence is
bit-reproducible, the mask noise is Philox keyed by (noise_seed, step count) and the class order comes from the stepper's own stream — so
"the same" is torch.equal on weights, both Adam moments, the last mask and the loss triple.  Across rank layouts (a checkpoint of two node
shards continued unsharded or on three) the bounds are the ones tests/test_gpu_shard.py holds a sharded run to against the unsharded one: the
resume adds no allowance of its own.  Shapes: the smallest that reach every route (tests/resume_util.py)."""
import json
import logging
import os
import re

import pytest
import torch

import resume_util as U
from gptst_amd import checkpoint as CK
from gptst_amd import data as D
from gptst_amd import synth

pytestmark = pytest.mark.gpu
DEV = U.DEV
N1 = 20                                           # unsharded cases
NS = 40                                           # shards: 20 / 20 at W = 2, 14 / 13 / 13 at W = 3 (the split with capacity padding)
_CACHE = {}


def _run_a(use_graph):
    """the uninterrupted run: nine single steps (EPOCHS and one more), a snapshot after each — computed once per launch form"""
    key = ("A", use_graph)
    if key not in _CACHE:
        args = U.small_args(N1)
        st = U.new_stepper(args, U.init_sd(args), use_graph=use_graph)
        snaps = []
        for e, src in zip(U.EPOCHS + (3,), U.batches(N1, 9)):
            st.step(src, e)
            snaps.append(U.snapshot(st))
        _CACHE[key] = snaps
    return _CACHE[key]


def _five_steps_then_checkpoint(use_graph, deterministic=True):
    args = U.small_args(N1)
    st = U.new_stepper(args, U.init_sd(args), use_graph=use_graph, deterministic=deterministic)
    for e, src in zip(U.EPOCHS[:5], U.batches(N1, 5)):
        st.step(src, e)                           # (nobody looks at the losses: state_dict() settles the steps in flight itself)
    return st, U.through_buffer(st.state_dict())


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_resumed_steps_are_bit_identical_to_the_uninterrupted_run(use_graph):
    run_a = _run_a(use_graph)
    _, sd = _five_steps_then_checkpoint(use_graph)
    assert (sd["optimizer"]["step"], sd["optimizer"]["step_kl"]) == (5, 2)
    assert list(sd["model"]) == list(U.init_sd(U.small_args(N1))) and len(sd["model"]) == 159
    args = U.small_args(N1)
    st = U.new_stepper(args, U.init_sd(args, seed=6), use_graph=use_graph)      # other weights: everything must come from the checkpoint
    st.load_state_dict(sd)
    for i, (e, src) in enumerate(zip(U.EPOCHS, U.batches(N1, 8))):
        if i >= 5:
            st.step(src, e)
            U.assert_same_run(U.snapshot(st), run_a[i], "step %d" % (i + 1))
    assert st.tA == 8 and st.tB == 5


def test_group_replay_after_a_resume_lines_up_with_single_steps():
    """the resumed stepper starts a replay of four steps at step count 5 — no multiple of the group: counters, bias corrections and Philox keys of
    the four sub-steps must be those of single steps 6..9"""
    run_a = _run_a(True)
    _, sd = _five_steps_then_checkpoint(True)
    args = U.small_args(N1)
    st = U.new_stepper(args, U.init_sd(args, seed=6), use_graph=True)
    st.load_state_dict(sd)
    assert st.group_ok(3)
    st.step_group(U.batches(N1, 9)[5:], 3)
    assert st.last_replay_steps == 4, "the four steps did not run as one replay"
    triples = st.losses_group()
    assert triples == [s["loss"] for s in run_a[5:]], (triples, [s["loss"] for s in run_a[5:]])
    U.assert_same_run(U.snapshot(st), run_a[8], "after the group")
    assert (st.tA, st.tB) == (9, 6)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_load_into_a_live_stepper_keeps_its_graphs(use_graph):
    from gptst_amd import ops
    other, sd = _five_steps_then_checkpoint(use_graph)
    args = U.small_args(N1)
    st = U.new_stepper(args, U.init_sd(args, seed=6), use_graph=use_graph)
    srcs = U.batches(N1, 9)

    def traced(epoch, src):
        ops.TIMER = []
        try:
            st.step(src, epoch)
            torch.cuda.synchronize()
            return [rec[0] for rec in ops.TIMER]
        finally:
            ops.TIMER = None

    st.step(srcs[0], 1)
    st.step(srcs[1], 3)                            # both phases captured
    before = traced(3, srcs[2])
    graphs = dict(st.graphs)
    assert (len(graphs) == 2) == use_graph and bool(before) != use_graph      # a replay makes no call of its own; an eager step makes all of them
    st.load_state_dict(sd)
    for i in (5, 6, 7):
        names = traced(3, srcs[i])
        other.step(srcs[i], 3)
        if i == 5:
            assert names == before, "the step behind the load launches something else than the step before it"
        U.assert_same_run(U.snapshot(st), U.snapshot(other), "step %d" % (i + 1))
    assert list(st.graphs) == list(graphs) and all(st.graphs[k][0] is graphs[k][0] and st.graphs[k][1] is graphs[k][1] for k in graphs)
    U.assert_same_run(U.snapshot(st), _run_a(use_graph)[7], "against the uninterrupted run")


def test_default_mode_restores_the_state_and_the_next_mask():
    """With float atomics two uninterrupted runs already differ, so the claim is narrower: what was saved is what is loaded, bit for bit, and the
    first resumed step masks the cells the in-process stepper masks (the forward has no atomics)."""
    other, sd = _five_steps_then_checkpoint(True, deterministic=False)
    args = U.small_args(N1)
    st = U.new_stepper(args, U.init_sd(args, seed=6), use_graph=True, deterministic=False)
    st.load_state_dict(sd)
    torch.cuda.synchronize()
    for a, b in ((st.model.flat, other.model.flat), (st.m, other.m), (st.v, other.v)):
        assert torch.equal(a, b)
    assert (st.tA, st.tB, st.lr, st.noise_seed) == (other.tA, other.tB, other.lr, other.noise_seed)
    src = U.batches(N1, 6)[5]
    st.step(src, 3)
    other.step(src, 3)
    torch.cuda.synchronize()
    assert torch.equal(st.last_mask, other.last_mask) and int((st.last_mask == 0).sum()) == int(U.B * U.T * N1 * args.mask_ratio)


# ---- node shards ------------------------------------------------------------------------------------------------------------------
# Two identical node-sharded runs on thread-emulated ranks with the library's fixed-order reductions ARE bit-identical: measured on the commit
# before this feature (three runs each of W = 3 and W = 2, four steps, N = 40: weights, moments, masks and losses of every rank equal).  So
# test_sharded_resume_same_layout asks for bit-identity, not for the cross-layout bounds.
SHARD_EPOCHS = (1, 3, 3, 3)


def _sharded(W, epochs, srcs, sd0, load=None, checkpoint_after=None):
    """W thread-emulated ranks from the global weights `sd0` [continuing from the checkpoint `load`] take `epochs` -> per rank a dict with the
    snapshot after the last step, the padding check after the load and — `checkpoint_after` steps in — the collective state_dict() with this
    rank's own moment views beside it"""
    def rank_main(r, group):
        st, (n0, n1) = U.local_stepper(sd0, NS, W, r, group)
        out = dict(range=(n0, n1))
        if load is not None:
            st.load_state_dict(load)
            out["pad_after_load"] = U.padding_max(st)
        for i, (e, src) in enumerate(zip(epochs, srcs)):
            st.step(src[:, :, n0:n1].contiguous(), e)
            if checkpoint_after == i + 1:
                out["ckpt"] = st.state_dict()
                torch.cuda.synchronize()
                out["own"] = {w: {k: v.cpu().clone() for k, v in st.model.views_of(buf).items()} for w, buf in (("exp_avg", st.m), ("exp_avg_sq", st.v))}
        out["snap"] = U.shard_snapshot(st)
        out["pad"] = U.padding_max(st)
        return out
    return U.run_ranks(W, rank_main)


def _w3_with_checkpoint():
    if "w3" not in _CACHE:
        args_g = U.small_args(NS)
        _CACHE["w3"] = _sharded(3, SHARD_EPOCHS, U.batches(NS, 4), U.init_sd(args_g), checkpoint_after=2)
    return _CACHE["w3"]


def test_sharded_checkpoint_is_global_and_assembled_in_node_order():
    from gptst_amd.model import GPTST_Model
    from gptst_amd.shard import is_node_local
    out = _w3_with_checkpoint()
    args_g = U.small_args(NS)
    gmodel = GPTST_Model(args_g)
    ck = out[0]["ckpt"]
    assert list(ck["model"]) == list(gmodel.state_dict()) and all(ck["model"][k].shape == v.shape for k, v in gmodel.state_dict().items())
    for w in ("exp_avg", "exp_avg_sq"):
        assert list(ck["optimizer"][w]) == [k for k, _ in gmodel.named_parameters()]
        assert all(ck["optimizer"][w][k].shape == p.shape and not ck["optimizer"][w][k].is_cuda for k, p in gmodel.named_parameters())
        for k in ck["optimizer"][w]:
            if is_node_local(k):
                want = torch.cat([o["own"][w][k] for o in out], dim=-1 if k.endswith(".adj") else 0)
                assert torch.equal(ck["optimizer"][w][k], want), k
            else:
                assert all(torch.equal(o["own"][w][k], out[0]["own"][w][k]) for o in out), "shared moment %s differs between ranks" % k
                assert torch.equal(ck["optimizer"][w][k], out[0]["own"][w][k]), k
        assert any(bool(ck["optimizer"][w][k].any()) for k in ck["optimizer"][w] if is_node_local(k))
    assert (ck["optimizer"]["step"], ck["optimizer"]["step_kl"]) == (2, 1)
    assert all(U.same_tree(o["ckpt"], ck) for o in out[1:])                  # every rank holds the same global checkpoint
    assert [o["pad"][1] > 0 for o in out] == [False, True, True] and all(o["pad"][0] == 0.0 for o in out)


def test_sharded_resume_same_layout():
    """W = 3 (14 / 13 / 13): a checkpoint after two steps, loaded into three fresh ranks that take the other two steps, against the run that was never
    interrupted.  Two identical sharded runs repeat bit for bit (see above), so the resumed one must be bit-identical too."""
    out = _w3_with_checkpoint()
    args_g = U.small_args(NS)
    sd = U.through_buffer(out[0]["ckpt"])
    got = _sharded(3, SHARD_EPOCHS[2:], U.batches(NS, 4)[2:], U.init_sd(args_g, seed=6), load=sd)
    for r, (g, o) in enumerate(zip(got, out)):
        assert g["pad_after_load"][0] == 0.0 and g["pad"][0] == 0.0 and g["pad_after_load"][1] == o["pad"][1], (r, g["pad_after_load"], g["pad"])
        assert (g["snap"]["tA"], g["snap"]["tB"]) == (4, 3)
        assert torch.equal(g["snap"]["mask"], o["snap"]["mask"]), "global mask differs on rank %d" % r
        U.assert_same_run(g["snap"], o["snap"], "rank %d" % r)


@pytest.mark.parametrize("target", ["unsharded", "w3"])
def test_checkpoint_of_two_shards_continues_on_another_layout(target):
    from gptst_amd.shard import unshard_state_dicts
    args_g = U.small_args(NS)
    sd0 = U.init_sd(args_g)
    epochs, srcs = (1, 3, 3), U.batches(NS, 3)
    if "ref3" not in _CACHE:
        st = U.new_stepper(args_g, sd0)
        for e, src in zip(epochs, srcs):
            st.step(src, e)
        snap = U.snapshot(st)
        snap["sd"] = {k: v.detach().cpu().clone() for k, v in st.model.state_dict().items()}
        _CACHE["ref3"] = snap
        _CACHE["w2ckpt"] = U.through_buffer(_sharded(2, epochs[:2], srcs[:2], sd0, checkpoint_after=2)[0]["ckpt"])
    ref, sd = _CACHE["ref3"], _CACHE["w2ckpt"]
    assert (sd["optimizer"]["step"], sd["optimizer"]["step_kl"]) == (2, 1)
    other = U.init_sd(args_g, seed=6)
    if target == "unsharded":
        st = U.new_stepper(args_g, other)
        st.load_state_dict(sd)
        st.step(srcs[2], 3)
        snaps = [U.snapshot(st)]
        got_sd = {k: v.detach().cpu().clone() for k, v in st.model.state_dict().items()}
    else:
        got = _sharded(3, epochs[2:], srcs[2:], other, load=sd)
        assert all(g["pad_after_load"][0] == 0.0 and g["pad"][0] == 0.0 for g in got) and sum(g["pad"][1] > 0 for g in got) == 2
        snaps = [g["snap"] for g in got]
        got_sd = unshard_state_dicts([g["snap"]["sd"] for g in got])
    for s in snaps:
        assert torch.equal(s["mask"], ref["mask"]), "global mask differs"
        U.assert_losses_close(s["loss"], ref["loss"], target)
        assert (s["tA"], s["tB"]) == (3, 2)
    U.assert_within_shard_bounds(got_sd, ref["sd"], sd0, args_g.lr_init, target)


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
AVG_RE = re.compile(r"Train Epoch (\d+): averaged Loss")


def _trainer_args(tmp, **kw):
    args = U.small_args(N1, batch_size=64, debug=False, **kw)
    args.log_dir = str(tmp)
    return args


def _train(args, seed, use_graph=True):
    """Trainer.train() on a tiny synthetic series (ragged last batch) -> (trainer, {epoch: returned average}, {epoch: log line}, best state)"""
    from gptst_amd.model import GPTST_Model, init_seed, xavier_init_
    from gptst_amd.trainer import Trainer
    raw = synth.make_series(N1, 3, interval=5, days=8, seed=3)[:-5]
    train, _, _, scaler, _, _ = D.get_dataloader(args, raw=raw, device=DEV, generator=torch.Generator().manual_seed(5))
    assert train.n % args.batch_size != 0
    args.scaler_zeros = float(scaler.transform(0))
    init_seed(seed)
    model = xavier_init_(GPTST_Model(args)).to(DEV)
    tr = Trainer(model, args, lambda epoch: (x.contiguous() for x in train.iter_x()), float(scaler.mean), float(scaler.std), args.batch_size,
                 use_graph=use_graph, batches_per_epoch=len(train), loader=train)
    avgs, lines = {}, {}
    plain = tr.train_epoch

    def train_epoch(epoch):
        avgs[epoch] = plain(epoch)
        return avgs[epoch]
    tr.train_epoch = train_epoch

    class Keep(logging.Handler):
        def emit(self, rec):
            m = AVG_RE.search(rec.getMessage())
            if m:
                lines[int(m.group(1))] = rec.getMessage()
    h = Keep()
    tr.logger.addHandler(h)
    try:
        best = tr.train()
    finally:
        tr.logger.removeHandler(h)
    return tr, avgs, lines, best


def test_trainer_resumes_from_the_epoch_2_checkpoint(tmp_path, monkeypatch):
    monkeypatch.setenv("GPTST_DETERMINISTIC", "1")
    over = dict(epochs=4, change_epoch=2, lr_decay_step="3", ckpt_every=2)
    a = _trainer_args(tmp_path / "a", ckpt_path=str(tmp_path / "a" / "state_{epoch}.pth"), **over)
    tr_a, avg_a, log_a, best_a = _train(a, seed=3)
    assert sorted(avg_a) == [1, 2, 3, 4] and sorted(f for f in os.listdir(tmp_path / "a") if f.endswith(".pth")) == ["state_2.pth", "state_4.pth"]

    b = _trainer_args(tmp_path / "b", ckpt_path=str(tmp_path / "b" / "state_{epoch}.pth"), resume=str(tmp_path / "a" / "state_2.pth"), **over)
    tr_b, avg_b, log_b, best_b = _train(b, seed=4)                     # (another initialisation: the weights come from the file)
    assert sorted(avg_b) == [3, 4]
    for e in (3, 4):
        assert avg_b[e] == avg_a[e] and log_b[e] == log_a[e], (e, avg_a, avg_b, log_a[e], log_b[e])
    assert list(best_a) == list(best_b) and all(torch.equal(best_a[k], best_b[k]) for k in best_a)
    assert (tr_a.best_loss, tr_a.not_improved, tr_a.step.lr) == (tr_b.best_loss, tr_b.not_improved, tr_b.step.lr)
    assert abs(tr_a.step.lr - a.lr_init * a.lr_decay_rate) < 1e-12 and (tr_a.step.tA, tr_a.step.tB) == (tr_b.step.tA, tr_b.step.tB)
    ck_a, ck_b = CK.load(str(tmp_path / "a" / "state_4.pth")), CK.load(str(tmp_path / "b" / "state_4.pth"))
    assert ck_a["trainer"]["epoch"] == 4 and ck_a["optimizer"]["step"] == tr_a.step.tA
    assert U.same_tree(ck_a, ck_b)

    # -resume auto with no file to find: the fresh run
    c = _trainer_args(tmp_path / "c", ckpt_path=str(tmp_path / "c" / "state_{epoch}.pth"), resume="auto", epochs=4, change_epoch=2, lr_decay_step="3")
    tr_c, avg_c, log_c, best_c = _train(c, seed=3)
    assert avg_c == avg_a and log_c == log_a and all(torch.equal(best_a[k], best_c[k]) for k in best_a)
    assert not [f for f in os.listdir(tmp_path / "c") if f.endswith(".pth")]


def test_trainer_resume_auto_picks_up_the_latest_checkpoint(tmp_path, monkeypatch):
    """the preempted job: the same command line again (-ckpt_every 1 -resume auto) continues behind the last epoch that was written"""
    monkeypatch.setenv("GPTST_DETERMINISTIC", "1")
    path = str(tmp_path / "state.pth")
    over = dict(change_epoch=1, ckpt_every=1, ckpt_path=path, resume="auto")
    tr_a, avg_a, _, _ = _train(_trainer_args(tmp_path, epochs=2, **over), seed=3)
    assert sorted(avg_a) == [1, 2] and CK.load(path)["trainer"]["epoch"] == 2
    with pytest.raises(ValueError, match="epochs"):                    # the schedule is part of what a resumed run must share
        _train(_trainer_args(tmp_path, epochs=3, **over), seed=3)
    tr_b, avg_b, _, _ = _train(_trainer_args(tmp_path, epochs=2, **over), seed=4)
    assert avg_b == {} and tr_b.epoch == 2 and tr_b.step.tA == tr_a.step.tA
    assert torch.equal(tr_b.model.flat, tr_a.model.flat)


def test_defaults_leave_the_run_as_it_was(tmp_path):
    """ckpt_every = 0, no resume: no state file, and every step of a two-epoch Trainer.train() makes the launches it made before this feature —
    tests/golden/resume_default_launches.json was written down from the same run on the commit before it (eager steps: every launch is a call)."""
    from gptst_amd import ops
    want = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "resume_default_launches.json")))
    args = U.small_args(N1, batch_size=128, debug=False, epochs=2, change_epoch=1)
    args.log_dir = str(tmp_path)
    assert (args.ckpt_every, args.resume) == (0, "")
    ops.TIMER = []
    try:
        _train(args, seed=3, use_graph=False)
        torch.cuda.synchronize()
        names = [rec[0] for rec in ops.TIMER]
    finally:
        ops.TIMER = None
    assert names[0] == want["marker"]
    steps = []
    for n in names:
        if n == want["marker"]:
            steps.append([])
        steps[-1].append(n)
    assert len(steps) == len(want["steps"]) == 2 * want["batches_per_epoch"]
    for i, (got, k) in enumerate(zip(steps, want["steps"])):
        assert got == want["sequences"][k], "step %d launches %s, before: %s" % (i + 1, got, want["sequences"][k])
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".pth")]


# ---- Run.py and data parallelism --------------------------------------------------------------------------------------------------
def _run_py(argv, monkeypatch):
    """Run.py's main() in this process (its flags are what is under test, not the interpreter start)"""
    import runpy
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setattr(sys, "argv", ["Run.py"] + argv)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    runpy.run_path(os.path.join(root, "gpt-st_amd", "Run.py"), run_name="__main__")


def test_run_py_flags_checkpoint_and_resume(tmp_path, monkeypatch):
    """`-ckpt_every 1 -ckpt_path .../state_{epoch}.pth` writes a file per epoch; the same command with `-resume auto` after the last file was lost (the
    preempted job) trains only the missing epoch and writes the same file again, bit for bit; `-shard nodes` continues from a file the unsharded
    run wrote."""
    import numpy as np
    monkeypatch.setenv("GPTST_DETERMINISTIC", "1")
    os.makedirs(tmp_path / "PEMS08")
    np.savez(tmp_path / "PEMS08" / "PEMS08.npz", data=synth.make_series(N1, 3, interval=5, days=8, seed=3))
    pattern = str(tmp_path / "state_{epoch}.pth")
    flags = ["-dataset", "PEMS08", "-mode", "pretrain", "-num_nodes", str(N1), "-embed_dim", "8", "-HS", "5", "-HT", "6", "-batch_size", "256",
             "-epochs", "2", "-change_epoch", "1", "-debug", "False", "-data_root", str(tmp_path), "-ckpt_every", "1", "-ckpt_path", pattern]
    _run_py(flags, monkeypatch)
    one, two = str(tmp_path / "state_1.pth"), str(tmp_path / "state_2.pth")
    first = CK.load(two)
    assert CK.load(one)["trainer"]["epoch"] == 1 and first["trainer"]["epoch"] == 2
    assert first["optimizer"]["step"] == 2 * CK.load(one)["optimizer"]["step"] and first["rng"]["loader"] is not None
    os.remove(two)
    _run_py(flags + ["-resume", "auto"], monkeypatch)
    assert U.same_tree(CK.load(two), first)
    os.remove(two)
    _run_py(flags + ["-resume", one, "-shard", "nodes"], monkeypatch)        # one rank owning all nodes: the sharded branch of Run.py
    again = CK.load(two)
    assert again["trainer"]["epoch"] == 2 and again["optimizer"]["step"] == first["optimizer"]["step"]
    assert list(again["model"]) == list(first["model"]) and U.same_tree(again["dims"], first["dims"])
    assert torch.equal(again["rng"]["loader"], first["rng"]["loader"])


def test_data_parallel_run_resumes(tmp_path):
    """Two gloo ranks on this GPU (tests/resume_dp_worker.py): rank 0 writes, both ranks read and end up with the same bits; the resumed run trains
    epoch 2 only — padded tail rounds and their steppers' class-order streams included — and writes the epoch-2 file the first run wrote."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import free_port
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(root, "tests", "resume_dp_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, cwd=root, env=dict(os.environ, GPTST_DIST_BACKEND="gloo", GPTST_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["epochs_a"] == [1, 2] and out["epochs_b"] == [2], out
    assert out["files"] == ["a/state_1.pth", "a/state_2.pth", "b/state_2.pth"], out          # rank 0 alone wrote, one file per epoch
    assert out["replicas_a"] and out["replicas_b"], "the replicas diverged"
    assert out["steps"][:2] == out["steps"][2:] == [2 * out["nb"], out["nb"]], out
    assert out["ragged"] == [13, 64], out                                                  # the steppers of the ragged batch and of the padded full round
    assert out["avg_a"] == out["avg_b"] and out["same_weights"] and out["same_checkpoint"], out
