"""CPU: the assembling and checking code of the sharded / data-parallel gradient checks (tests/step_grad_util.py::assemble_sharded, check_sharded,
check_dp, ThreadDP) is proven before it is trusted.  The fp32 oracle's gradients of the GLOBAL problem, dressed as what W ranks leave behind
(node-local keys sliced to the rank's nodes and padded to the widest shard's slot, shared keys replicated, path A multiplied by the kept count),
pass against the fp64 oracle; each defect the GPU file is there to catch fails, with the offending key or statistic named."""
import threading

import pytest
import torch

import step_grad_util as U
from gptst_amd.shard import ThreadNodeGroup, is_node_local, is_replicated_compute, node_ranges, shard_state_dict
from oracle import gptst_oracle as O

W, N, B = 3, 40, 2                                  # shards 14 / 13 / 13: two ranks carry capacity padding
SEEDS = (6, 11)                                     # (sd_seed, source seed) of the GPU file's N = 40 cases
REPL = "encoder.STHCN_encode.cap1.t_adj"
SHARED = "decoder.STHCN_decode.hyperTem2.weights_pool"
LOCAL_ADJ, LOCAL_ROWS = "decoder.STHCN_decode.cap1.adj", "encoder.STHCN_encode.node_embeddings"


def _slot(t, key, width, cap):
    """a node-local tensor's whole slot in the flat buffer: the tensor, then zeros for the nodes up to the capacity (model.py)"""
    return torch.cat([t.reshape(-1), torch.zeros(t.numel() // width * (cap - width), dtype=t.dtype)])


@pytest.fixture(scope="module", params=[1, 20], ids=["rand", "ada"])
def dressed(request):
    epoch = request.param
    args = U.dist_args(num_nodes=N, **U.SMALL_DIST)
    sd = O.init_state_dict(args, SEEDS[0])
    src = U.make_src(args, B, seed=SEEDS[1])
    inj = U.noise_inject(args, B, epoch)
    g64, _, m64, kept = U.oracle_grads(args, sd, src, epoch, inj, torch.float64)
    g32, _, m32, _ = U.oracle_grads(args, sd, src, epoch, inj, torch.float32)
    assert torch.equal(m32, m64) and kept == U.kept_count(args, src, m64)
    offs, nA, nB = U.layout_of(args)
    stored = {k: (torch.zeros_like(sd[k]) if g is None else g * kept if offs[k] < nA else g.clone()) for k, g in g32.items()}
    ranges = node_ranges(N, W)
    cap = max(b - a for a, b in ranges)
    stats = torch.zeros(8)
    stats[1], stats[4] = kept, U.grad_norm(g32) ** 2               # (in the random phase the KL path has no gradient: grad_norm skips it)
    per_rank = []
    for a, b in ranges:
        g, w = shard_state_dict(stored, a, b), {k: v for k, v in shard_state_dict(sd, a, b).items() if k in stored}
        loc = [k for k in g if is_node_local(k)]
        per_rank.append(dict(g=g, w=w, stats=stats.clone(), kl=epoch > args.change_epoch, mask=m64.clone(),
                             slots_g={k: _slot(g[k], k, b - a, cap) for k in loc}, slots_w={k: _slot(w[k], k, b - a, cap) for k in loc}))
    return dict(args=args, per_rank=per_rank, ranges=ranges, g64=g64, g32=g32, kept=kept, src=src, m64=m64, stored=stored, cap=cap, epoch=epoch)


def _copy(per_rank):
    return [dict(p, g=dict(p["g"]), w=dict(p["w"]), slots_g=dict(p["slots_g"]), slots_w=dict(p["slots_w"]), stats=p["stats"].clone())
            for p in per_rank]


def _check(d, per_rank):
    seen = {}
    allowed = U.check_sharded(per_rank, d["ranges"], d["args"], d["g64"], lambda: d["g32"], d["kept"], seen.__setitem__)
    return allowed, seen


def test_keys_of_the_dressing(dressed):
    g = dressed["per_rank"][0]["g"]
    assert is_replicated_compute(REPL) and REPL in g
    assert SHARED in g and not is_node_local(SHARED) and not is_replicated_compute(SHARED)
    assert is_node_local(LOCAL_ADJ) and is_node_local(LOCAL_ROWS) and LOCAL_ADJ in g and LOCAL_ROWS in g
    widths = [p["g"][LOCAL_ROWS].shape[0] for p in dressed["per_rank"]]
    assert widths == [14, 13, 13] == [p["g"][LOCAL_ADJ].shape[-1] for p in dressed["per_rank"]]
    assert [p["slots_g"][LOCAL_ROWS].numel() > p["g"][LOCAL_ROWS].numel() for p in dressed["per_rank"]] == [False, True, True]


def test_honest_dressing_passes(dressed):
    allowed, seen = _check(dressed, dressed["per_rank"])
    assert allowed == {}
    trained = [k for k, g in dressed["g64"].items() if g is not None]
    assert sorted(k for k in seen if k.startswith("grad:")) == sorted("grad:" + k for k in trained)
    assert max(v for k, v in seen.items() if k.startswith("grad:")) < U.GRAD_TOL
    assert seen["pad_max_grad"] == 0.0 and seen["pad_max_weights"] == 0.0 and seen["grad_norm"] < 1e-5
    got, rep = U.assemble_sharded(dressed["per_rank"], dressed["ranges"], dressed["args"])
    assert all(rep["shared_identical"].values()) and all(torch.equal(got[k], v) for k, v in dressed["stored"].items())
    # the same gradients as W data-parallel replicas
    reps = [dict(g=dict(dressed["stored"]), w={}, stats=dressed["per_rank"][0]["stats"].clone()) for _ in range(2)]
    assert U.check_dp(reps, dressed["args"], dressed["g64"], lambda: dressed["g32"], dressed["kept"], seen.__setitem__) == {}


def test_each_defect_fails_with_its_key_named(dressed):
    d = dressed

    def fails(per_rank, *words):
        with pytest.raises(AssertionError) as ei:
            _check(d, per_rank)
        for w in words:
            assert w in str(ei.value), (w, str(ei.value)[:400])

    # 1. a replicated-compute key not divided by W: W times too large on all ranks
    pr = _copy(d["per_rank"])
    for p in pr:
        p["g"][REPL] = p["g"][REPL] * W
    fails(pr, REPL)
    # 2. a shared key summed over W - 1 of the W ranks
    pr = _copy(d["per_rank"])
    for p in pr:
        p["g"][SHARED] = p["g"][SHARED] * ((W - 1) / W)
    fails(pr, SHARED)
    # 3. a node-local shard shifted by one node (rank 1 holds [a + 1, b + 1)), on either node axis
    for key in (LOCAL_ADJ, LOCAL_ROWS):
        pr = _copy(d["per_rank"])
        a, b = d["ranges"][1]
        t = shard_state_dict({key: d["stored"][key]}, a + 1, b + 1)[key]
        pr[1]["g"][key], pr[1]["slots_g"][key] = t, _slot(t, key, b - a, d["cap"])
        fails(pr, key)
    # 4. a nonzero value in a padding slot, of the gradient and of the weights
    for what, word in (("slots_g", "gradient padding"), ("slots_w", "weight padding")):
        pr = _copy(d["per_rank"])
        s = pr[2][what][LOCAL_ADJ].clone()
        s[-1] = 1e-30
        pr[2][what][LOCAL_ADJ] = s
        fails(pr, word, LOCAL_ADJ)
    # 5. a shared key differing in one ulp on one rank, gradient and post-step weight
    for what, word in (("g", "shared gradients differ"), ("w", "shared weights differ")):
        pr = _copy(d["per_rank"])
        t = pr[1][what][SHARED].clone()
        t.view(-1)[3] = torch.nextafter(t.view(-1)[3], torch.tensor(float("inf")))
        pr[1][what][SHARED] = t
        fails(pr, word, SHARED)
    # 6. a clip norm that leaves out the other ranks' node-local part (3e-5 .. 4e-5 off here: under the 1e-4 against the oracle, caught by
    #    the comparison with the gradient the ranks hold)
    offs, nA, _ = U.layout_of(d["args"])
    pr = _copy(d["per_rank"])
    for p in pr:
        sq = sum(float(((v.double() / (d["kept"] if offs[k] < nA else 1.0)) ** 2).sum()) for k, v in p["g"].items())
        p["stats"][4] = sq
    fails(pr, "clip norm")
    # 7. a kept count from one rank only
    pr = _copy(d["per_rank"])
    for p, (a, b) in zip(pr, d["ranges"]):
        p["stats"][1] = U.kept_count(d["args"], d["src"][:, :, a:b], d["m64"][:, :, a:b])
    assert sum(float(p["stats"][1]) for p in pr) == d["kept"]
    fails(pr, "kept count")


def test_thread_dp_collectives():
    """ThreadDP between three threads on CPU tensors: the all-reduce leaves the same bits on every rank, the label gather is in rank order"""
    Wd = 3
    shared = ThreadNodeGroup.Shared(Wd)
    bufs = [torch.randn(1000, generator=torch.Generator().manual_seed(r)) for r in range(Wd)]
    want = bufs[0] + bufs[1] + bufs[2]
    out = [None] * Wd

    def run(r):
        dp = U.ThreadDP(r, shared)
        b = bufs[r].clone()
        dp.allreduce_(b)
        lab = dp.gather_labels(torch.full((4,), r, dtype=torch.int32), out=torch.zeros(4 * Wd, dtype=torch.int32))
        cnt = dp.sum_counts_(torch.tensor([r, 1], dtype=torch.int32))
        out[r] = (b, lab, cnt, dp.rows_of(torch.arange(6 * Wd), 6))

    ths = [threading.Thread(target=run, args=(r,)) for r in range(Wd)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(60)
    assert not any(t.is_alive() for t in ths)
    for r, (b, lab, cnt, rows) in enumerate(out):
        assert torch.equal(b, want) and lab.tolist() == [0] * 4 + [1] * 4 + [2] * 4 and cnt.tolist() == [3, 3]
        assert rows.tolist() == list(range(6 * r, 6 * r + 6))
