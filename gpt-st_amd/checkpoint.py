"""The portable state of a pretraining run: what ``Trainer.save_state`` writes once per ``-ckpt_every`` epochs and ``-resume`` reads.

A plain ``torch.save`` dictionary, the same whichever run mode wrote it (one GPU, data parallel, node shards of any count):

    format, version     "gptst_amd.pretrain_state", 1
    model               the GLOBAL state dict in the reference's format: the 159 keys of an unsharded model, in their order, on the CPU
    optimizer           exp_avg / exp_avg_sq as {parameter key: tensor of the parameter's GLOBAL shape}, step (tA: updates of the reconstruction
                        path), step_kl (tB: updates of the KL path), lr.  The flat buffers are never stored: segment order, 16-byte alignment,
                        node_capacity padding and the number of ranks are layout, not state.
    rng                 noise_seed (Philox key of the mask noise, with the step count), class_order (random.Random state of the stepper),
                        ragged_class_order ({batch size: state} of the steppers of ragged / tail batches), loader (torch.Generator state of the
                        train loader's epoch shuffle, None when the loader draws from the global generator)
    trainer             epoch (last completed), best_loss, not_improved, best_state (global format, or None), lr (after that epoch's MultiStepLR
                        decision)
    dims                the arguments a resumed run must share (DIM_KEYS; num_nodes is the global count)

``to_torch_adam_state`` / ``from_torch_adam_state`` carry the optimizer section to and from ``torch.optim.Adam(model.parameters(), ...)`` — the
reference's own loop (Run.py:134) continues a run pretrained here, and the other way round.
"""
import os

import torch

FORMAT = "gptst_amd.pretrain_state"
VERSION = 1
DIM_KEYS = ("num_nodes", "hidden_dim", "HS", "HT", "HT_Tem", "embed_dim", "embed_dim_spa", "input_base_dim", "num_route", "lag",
            "change_epoch", "epochs", "mask_ratio", "ada_mask_ratio", "ada_type")
BETAS, EPS = (0.9, 0.999), 1e-8               # the optimiser's constants (step.py::_fill; Run.py:134 of the reference)


def dims_of(args, num_nodes=None):
    """The `dims` section of a run with these arguments.  num_nodes: the GLOBAL node count of a node-sharded run (args holds the shard's)."""
    d = {k: getattr(args, k) for k in DIM_KEYS}
    if num_nodes is not None:
        d["num_nodes"] = int(num_nodes)
    return d


def check_dims(saved, dims):
    """ValueError naming the first key on which the checkpoint's dims and the run's disagree (and both values)."""
    for k in DIM_KEYS:
        if k not in saved:
            raise ValueError("checkpoint dims lack %r" % k)
        if saved[k] != dims[k]:
            raise ValueError("checkpoint was written with %s = %r, this run has %s = %r" % (k, saved[k], k, dims[k]))


def validate(ckpt, dims=None):
    """-> ckpt, after checking format, version, the sections and (dims given) that the run's arguments match the checkpoint's."""
    if not isinstance(ckpt, dict) or ckpt.get("format") != FORMAT:
        raise ValueError("not a pretraining state: format = %r (expected %r)" % (ckpt.get("format") if isinstance(ckpt, dict) else type(ckpt), FORMAT))
    if ckpt.get("version") != VERSION:
        raise ValueError("pretraining state has version = %r, this build reads version %d" % (ckpt.get("version"), VERSION))
    for sec in ("model", "optimizer", "rng", "trainer", "dims"):
        if sec not in ckpt:
            raise ValueError("pretraining state lacks its %r section" % sec)
    if dims is not None:
        check_dims(ckpt["dims"], dims)
    return ckpt


def pack(model, optimizer, rng, trainer, dims):
    return dict(format=FORMAT, version=VERSION, model=model, optimizer=optimizer, rng=rng, trainer=trainer, dims=dict(dims))


def save(ckpt, path):
    """Atomic: written under a temporary name in the target's directory, then os.replace — a job killed mid-write leaves the previous file."""
    validate(ckpt)
    path = os.path.abspath(path)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = "%s.tmp.%d" % (path, os.getpid())
    try:
        torch.save(ckpt, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def load(path, dims=None):
    """The checkpoint at `path` (a file name or a file object), on the CPU, validated."""
    return validate(torch.load(path, map_location="cpu", weights_only=True), dims)


def rng_state(state):
    """random.Random.setstate wants tuples: (version, tuple of words, gauss_next) however the container came back from the file"""
    return (int(state[0]), tuple(int(w) for w in state[1]), state[2])


# ---- torch.optim.Adam -------------------------------------------------------------------------------------------------------------
def _stateless(key, step_kl):
    """Parameters torch.optim.Adam keeps no state for — they never had a gradient: the KL path before its first step, and always the decoder's two
    unused time-feature blocks (optim.ClipAdam skips the same set)."""
    from .model import _segment
    seg = _segment(key)
    return seg == 2 or (seg == 1 and step_kl == 0)


def to_torch_adam_state(ckpt, model):
    """The optimizer section of `ckpt` (a whole checkpoint or the section alone) as the dictionary
    ``torch.optim.Adam(model.parameters(), lr, eps=1e-8).load_state_dict`` accepts: per-parameter state in ``model.parameters()`` order — `step` is
    the reconstruction path's count or the KL path's, by the parameter's segment — and one parameter group with the installed torch's defaults.
    `model`: a GPTST_Model (or the reference's) with the checkpoint's GLOBAL shapes; only its parameter names and order are read."""
    from .model import _segment
    opt = ckpt["optimizer"] if "optimizer" in ckpt else ckpt
    named = list(model.named_parameters())
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=float(opt["lr"]), betas=BETAS, eps=EPS, weight_decay=0, amsgrad=False)
    group = dict(ref.state_dict()["param_groups"][0])
    group["params"] = list(range(len(named)))
    tA, tB = int(opt["step"]), int(opt["step_kl"])
    state = {}
    for i, (k, p) in enumerate(named):
        if tA == 0 or _stateless(k, tB):
            continue
        m, v = opt["exp_avg"][k], opt["exp_avg_sq"][k]
        if tuple(m.shape) != tuple(p.shape):
            raise ValueError("%s: the checkpoint's moments have shape %s, the model's parameter %s" % (k, tuple(m.shape), tuple(p.shape)))
        state[i] = dict(step=torch.tensor(float(tB if _segment(k) == 1 else tA), dtype=torch.float32),
                        exp_avg=m.detach().clone(), exp_avg_sq=v.detach().clone())
    return dict(state=state, param_groups=[group])


def from_torch_adam_state(state, model):
    """Inverse: ``torch.optim.Adam.state_dict()`` over ``model.parameters()`` -> the optimizer section.  Parameters without state get zero moments."""
    from .model import _segment
    named = list(model.named_parameters())
    group = state["param_groups"][0]
    if len(state["param_groups"]) != 1 or len(group["params"]) != len(named):
        raise ValueError("expected ONE parameter group over all %d parameters of the model" % len(named))
    if tuple(group["betas"]) != BETAS or group["eps"] != EPS or group.get("weight_decay", 0) != 0 or group.get("amsgrad", False):
        raise ValueError("the fused optimiser is Adam(betas=%s, eps=%g, weight_decay=0, amsgrad=False)" % (BETAS, EPS))
    exp_avg, exp_avg_sq, steps = {}, {}, [set(), set()]
    for idx, (k, p) in zip(group["params"], named):
        st = state["state"].get(idx)
        if st is None:
            exp_avg[k] = torch.zeros(p.shape, dtype=torch.float32)
            exp_avg_sq[k] = torch.zeros(p.shape, dtype=torch.float32)
            continue
        seg = _segment(k)
        if seg == 2:
            raise ValueError("%s carries optimizer state, but is never trained in pretraining" % k)
        steps[seg].add(int(st["step"]))
        exp_avg[k] = st["exp_avg"].detach().to("cpu", torch.float32).clone()
        exp_avg_sq[k] = st["exp_avg_sq"].detach().to("cpu", torch.float32).clone()
    for seg, what in ((0, "reconstruction"), (1, "KL")):
        if len(steps[seg]) > 1:
            raise ValueError("the %s path's parameters disagree on their step count: %s" % (what, sorted(steps[seg])))
    return dict(exp_avg=exp_avg, exp_avg_sq=exp_avg_sq, step=max(steps[0], default=0), step_kl=max(steps[1], default=0), lr=float(group["lr"]))
