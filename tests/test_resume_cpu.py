"""CPU: the portable pretraining state (gpt-st_amd/checkpoint.py) — the file format and its checks, the atomic write, the shard algebra the
moments go through, the torch.optim.Adam converters against the textbook update in fp64, and the epoch shuffle's generator state."""
import os
import random
from types import SimpleNamespace

import pytest
import torch

import resume_util as U
from gptst_amd import checkpoint as CK


def _model(n=20, **kw):
    from gptst_amd.model import GPTST_Model
    args = U.small_args(n, **kw)
    m = GPTST_Model(args)
    return m, args


def _global_model(n=20):
    m, args = _model(n)
    m.load_state_dict(U.init_sd(args))
    return m, args


def _moments(model, seed, tB=2):
    """random moments of the parameters' shapes; zero where the optimiser keeps no state (never-trained blocks; the KL path while tB == 0)"""
    g = torch.Generator().manual_seed(seed)
    exp_avg, exp_avg_sq = {}, {}
    for k, p in model.named_parameters():
        dead = CK._stateless(k, tB)
        exp_avg[k] = torch.zeros(p.shape) if dead else torch.randn(p.shape, generator=g) * 1e-2
        exp_avg_sq[k] = torch.zeros(p.shape) if dead else torch.rand(p.shape, generator=g) * 1e-3 + 1e-6
    return exp_avg, exp_avg_sq


def _checkpoint(seed=1, tA=5, tB=2):
    model, args = _global_model()
    m, v = _moments(model, seed, tB)
    rng = random.Random(3)
    rng.shuffle(list(range(5)))
    sd = {k: t.detach().clone() for k, t in model.state_dict().items()}
    ckpt = CK.pack(sd, dict(exp_avg=m, exp_avg_sq=v, step=tA, step_kl=tB, lr=3e-3 * 0.3),
                   dict(noise_seed=1234567, class_order=rng.getstate(), ragged_class_order={1: random.Random(0).getstate()},
                        loader=torch.Generator().manual_seed(5).get_state()),
                   dict(epoch=2, best_loss=0.25, not_improved=1, best_state={k: t + 1 for k, t in sd.items()}, lr=3e-3 * 0.3), CK.dims_of(args))
    return ckpt, model, args


def test_checkpoint_round_trip_and_format_checks(tmp_path):
    ckpt, model, args = _checkpoint()
    assert len(ckpt["model"]) == 159 and list(ckpt["model"]) == list(model.state_dict())
    assert list(ckpt["optimizer"]["exp_avg"]) == [k for k, _ in model.named_parameters()]
    path = CK.save(ckpt, str(tmp_path / "sub" / "state.pth"))
    back = CK.load(path, CK.dims_of(args))
    assert U.same_tree(ckpt, back)
    r = random.Random(0)
    r.setstate(CK.rng_state(back["rng"]["class_order"]))            # the class-order stream continues where it was
    r0 = random.Random(0)
    r0.setstate(ckpt["rng"]["class_order"])
    assert [r.random() for _ in range(4)] == [r0.random() for _ in range(4)]
    assert not [f for f in os.listdir(tmp_path / "sub") if f != "state.pth"]            # no temporary file left behind

    for bad in (dict(version=2), dict(version=None), dict(format="something.else")):
        with pytest.raises(ValueError, match=list(bad)[0]):
            CK.validate(dict(ckpt, **bad))
        torch.save(dict(ckpt, **bad), str(tmp_path / "bad.pth"))
        with pytest.raises(ValueError, match=list(bad)[0]):
            CK.load(str(tmp_path / "bad.pth"))
        with pytest.raises(ValueError):
            CK.save(dict(ckpt, **bad), str(tmp_path / "never.pth"))
    assert not os.path.exists(tmp_path / "never.pth")


@pytest.mark.parametrize("key", CK.DIM_KEYS)
def test_checkpoint_dims_mismatch_names_the_key(key, tmp_path):
    ckpt, _, args = _checkpoint()
    path = CK.save(ckpt, str(tmp_path / "state.pth"))
    dims = CK.dims_of(args)
    other = dict(dims)
    other[key] = "one" if key == "ada_type" else dims[key] + 1
    with pytest.raises(ValueError) as e:
        CK.load(path, other)
    msg = str(e.value)
    assert key in msg.split() and repr(dims[key]) in msg and repr(other[key]) in msg, msg
    free = SimpleNamespace(**vars(args))
    free.batch_size, free.seed, free.lr_init = 7, 99, 1.0                   # not part of what a resumed run must share
    CK.load(path, CK.dims_of(free))
    assert CK.dims_of(U.small_args(13), num_nodes=40)["num_nodes"] == 40   # a shard's arguments, the global node count


def test_save_is_atomic_when_the_write_dies_half_way(tmp_path, monkeypatch):
    ckpt, _, args = _checkpoint(seed=1)
    newer, _, _ = _checkpoint(seed=2, tA=9)
    path = CK.save(ckpt, str(tmp_path / "state.pth"))
    plain = torch.save

    def dies(obj, f, *a, **k):
        with open(f, "wb") as fh:                       # part of a file reaches the disk, then the job is killed
            fh.write(b"PK\x03\x04 half a checkpoint")
        raise KeyboardInterrupt("preempted")

    monkeypatch.setattr(torch, "save", dies)
    with pytest.raises(KeyboardInterrupt):
        CK.save(newer, path)
    monkeypatch.setattr(torch, "save", plain)
    assert os.listdir(tmp_path) == ["state.pth"]
    back = CK.load(path, CK.dims_of(args))
    assert U.same_tree(ckpt, back) and back["optimizer"]["step"] == 5
    CK.save(newer, path)
    assert CK.load(path)["optimizer"]["step"] == 9


def test_named_moments_survive_the_shard_algebra_and_leave_padding_zero():
    """N = 40 over 14 / 13 / 13: moments keyed by name go through shard_state_dict / unshard_state_dicts like the weights, and placed into a model
    laid out with node_capacity = 14 (the stepper's own staging code) every element no parameter owns stays zero."""
    from gptst_amd.shard import is_node_local, node_ranges, shard_state_dict, unshard_state_dicts
    from gptst_amd.step import PretrainStep
    N, W = 40, 3
    gmodel, _ = _model(N)
    m, _ = _moments(gmodel, 7)
    m = {k: t + 1.0 for k, t in m.items()}                                   # no zeros of its own
    ranges = node_ranges(N, W)
    assert [b - a for a, b in ranges] == [14, 13, 13]
    parts = [shard_state_dict(m, a, b) for a, b in ranges]
    back = unshard_state_dicts(parts)
    assert list(back) == list(m) and all(torch.equal(back[k], m[k]) for k in m)
    padded = 0
    for (a, b), part in zip(ranges, parts):
        local, _ = _model(b - a, node_capacity=14)
        img = PretrainStep._stage_flat(SimpleNamespace(model=local), part, "exp_avg")
        assert img.numel() == local.flat.numel()
        owned = torch.zeros(img.numel(), dtype=torch.bool)
        for k, view in local.views_of(img).items():
            assert torch.equal(view, part[k]), k
            o, n, slot = local._offs[k], view.numel(), local._slot_numel[k]
            owned[o:o + n] = True
            if is_node_local(k):
                assert slot == n // (b - a) * 14
                assert float(img[o + n:o + slot].abs().max()) == 0.0 if slot > n else True, k
                padded += slot - n
        assert float(img[~owned].abs().max()) == 0.0
    assert padded > 0                                                           # the 13-node ranks do carry capacity padding
    with pytest.raises(ValueError, match="shape"):
        PretrainStep._stage_flat(SimpleNamespace(model=local), parts[0], "exp_avg")      # a 14-node part into a 13-node model
    with pytest.raises(KeyError):
        PretrainStep._stage_flat(SimpleNamespace(model=local), {}, "exp_avg")


@pytest.mark.parametrize("tA,tB", [(5, 0), (5, 2)])
def test_torch_adam_continues_from_the_checkpoint(tA, tB):
    """to_torch_adam_state -> torch.optim.Adam.load_state_dict -> one step() on random gradients == the textbook Adam update in fp64 with the step
    counts a parameter's segment has seen; parameters that never had a gradient carry no state; from_torch_adam_state inverts."""
    from gptst_amd.model import _segment
    model, args = _global_model()
    exp_avg, exp_avg_sq = _moments(model, 11, tB)
    lr = 3e-3 * 0.3
    section = dict(exp_avg=exp_avg, exp_avg_sq=exp_avg_sq, step=tA, step_kl=tB, lr=lr)
    state = CK.to_torch_adam_state(dict(optimizer=section), model)
    named = list(model.named_parameters())
    want_stateless = {k for k, _ in named if _segment(k) == 2 or (_segment(k) == 1 and tB == 0)}
    assert {named[i][0] for i in range(len(named)) if i not in state["state"]} == want_stateless
    assert any(_segment(k) == 1 for k, _ in named) and sum(_segment(k) == 2 for k, _ in named) == 20       # two TimeFeature blocks of 5 Linears
    opt = torch.optim.Adam(model.parameters(), lr=args.lr_init, eps=1e-8, weight_decay=0, amsgrad=False)
    opt.load_state_dict(state)
    assert opt.param_groups[0]["lr"] == lr
    inv = CK.from_torch_adam_state(opt.state_dict(), model)
    assert U.same_tree(inv, section)

    g = torch.Generator().manual_seed(21)
    before = {k: p.detach().double().clone() for k, p in named}
    for _, p in named:
        p.grad = torch.randn(p.shape, generator=g)
    opt.step()
    b1, b2, eps = 0.9, 0.999, 1e-8
    worst = 0.0
    for k, p in named:
        t = 1 + (0 if k in want_stateless else (tB if _segment(k) == 1 else tA))
        gr = p.grad.double()
        m = b1 * (0.0 if k in want_stateless else exp_avg[k].double()) + (1 - b1) * gr
        v = b2 * (0.0 if k in want_stateless else exp_avg_sq[k].double()) + (1 - b2) * gr * gr
        want = before[k] - lr * (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps)
        worst = max(worst, float((p.detach().double() - want).abs().max()))
        assert int(opt.state[p]["step"]) == t, k
    assert worst <= 1e-6, worst
    with pytest.raises(ValueError, match="never trained"):          # (this test gave EVERY parameter a gradient: a pretraining run never does)
        CK.from_torch_adam_state(opt.state_dict(), model)


def test_from_torch_adam_state_refuses_what_the_fused_optimiser_is_not():
    model, args = _global_model()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-8, weight_decay=1e-2)
    with pytest.raises(ValueError, match="weight_decay"):
        CK.from_torch_adam_state(opt.state_dict(), model)
    fresh = CK.from_torch_adam_state(torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-8).state_dict(), model)
    assert (fresh["step"], fresh["step_kl"]) == (0, 0) and all(not bool(t.any()) for t in fresh["exp_avg"].values())
    assert CK.to_torch_adam_state(fresh, model)["state"] == {}


def test_epoch_shuffle_continues_from_the_saved_generator_state():
    from gptst_amd.data import WindowLoader
    series = torch.arange(100 * 3 * 3, dtype=torch.float32).view(100, 3, 3)

    def loader(seed):
        return WindowLoader(series, 12, 12, 8, shuffle=True, generator=torch.Generator().manual_seed(seed))
    a = loader(5)
    for _ in range(2):                                  # epochs 1 and 2
        list(a.iter_x())
    saved = U.through_buffer(dict(loader=a.gen.get_state()))["loader"]
    nxt = [x.clone() for x in a.iter_x()]               # epoch 3 of the uninterrupted run
    order = a._last_order.clone()
    b = loader(999)                                     # a fresh process: another generator, restored
    b.gen.set_state(saved)
    got = list(b.iter_x())
    assert torch.equal(b._last_order, order) and not torch.equal(order, torch.arange(a.n))
    assert len(got) == len(nxt) and all(torch.equal(x, y) for x, y in zip(got, nxt))
