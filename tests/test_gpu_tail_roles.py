"""GPU: the end of the backward as three launches that carry the gradient reductions as further workgroups (tail roles: engine.tail_roles_ok,
gptst_encin_ht1_bwd_jobs / gptst_gram_bwd_jobs / gptst_timefeat_jobs_bwd_jobs) against the stand-alone launches (GPTST_TAIL_ROLES=0)."""
import pytest
import torch

from gptst_amd import synth
from gptst_amd.config import make_args
from step_grad_util import noise_inject, one_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T, C = 2, 12, 64
PJ_MAX = 112                     # jobs one table holds (csrc/poolgen_dev.h)
# float atomics collect the kind-2 (embedding) targets and the time-feature gradients: two runs of the SAME launches differ in their last bits
ATOMIC = dict(rtol=1e-5, atol=1e-6)
GUIDE_EMB = ("encoder.teb4mask.", "encoder.neb4mask")


def rnd(*shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


class Table:
    """the reduction jobs every host is tested with, on fresh zeroed targets: build() -> (PoolJobs, kind-1 targets, kind-2 targets)"""

    def __init__(self, N, g, HS=5, d=6):
        # The operands of the kind-2 jobs are POSITIVE.  A kind-2 target element is the sum of up to n = 18 per-chunk partials (4096 / 256 columns,
        # + 2 chunks of the scalar-column job) added by float atomics in any order: two orders differ by at most (n - 1) 2^-24 sum|partial| ~ 1e-6
        # sum|partial|.  Without cancellation sum|partial| is the result itself, so ATOMIC's rtol 1e-5 holds by an order of magnitude; with signed
        # random data the result can be 100 times smaller than the partials and no relative bound would mean anything.
        pos = lambda *s: rnd(*s, g=g).abs()      # noqa: E731
        self.N, self.HS, self.d = N, HS, d
        self.te, self.ne = rnd(B * T, d, g=g), rnd(N, d, g=g)
        self.dWb = pos(B * T, C * C + C)                       # a float4 matrix and its column window
        self.dl = pos(B * T, HS * N)                           # HS * N = 85 / 350 columns: the scalar-column path
        self.dWn = pos(2 * N, C * C)                           # two row splits
        self.pool_w, self.pool_b, self.pool_l = pos(d, C * C), pos(d, C), pos(d, HS * N)
        assert (HS * N) % 4 != 0

    def build(self):
        z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
        k1 = [z(self.d, C * C), z(self.d, C), z(self.d, self.HS * self.N)]
        k2 = [z(self.N, self.d), z(B * T, self.d)]
        pj = _pool_jobs()
        pj.bwd_pool(self.te, self.dWb[:, :C * C], k1[0])                 # kind 1, cols % 4 == 0
        pj.bwd_pool(self.te, self.dWb[:, C * C:], k1[1])
        pj.bwd_pool(self.te, self.dl, k1[2])                            # kind 1, cols = HS * N
        pj.bwd_emb(self.dWn, self.pool_w, k2[0], nsplit=2)              # kind 2, nsplit = 2
        pj.bwd_emb(self.dWb[:, :C * C], self.pool_w, k2[1])             # two kind-2 jobs (one of them scalar columns) into the same demb
        pj.bwd_emb(self.dl, self.pool_l, k2[1])
        return pj, k1, k2


def _pool_jobs():
    from gptst_amd import ops
    return ops.PoolJobs()


class Recorded:
    """names of the launches enqueued inside the block (ops.TIMER)"""

    def __enter__(self):
        from gptst_amd import ops
        self.names, ops.TIMER = [], []
        return self

    def __exit__(self, *exc):
        from gptst_amd import ops
        self.names += [r[0] for r in ops.TIMER]
        ops.TIMER = None


def _check_tables(k1, k2, ref1, ref2):
    for i, (a, b) in enumerate(zip(k1, ref1)):
        assert torch.equal(a, b), ("kind-1 target", i)
    for i, (a, b) in enumerate(zip(k2, ref2)):
        torch.testing.assert_close(a, b, msg="kind-2 target %d" % i, **ATOMIC)


def _encin_inputs(N, g):
    from gptst_amd import ops
    src = rnd(B, T, N, 3, g=g)
    mask = (torch.rand(B * T * N, generator=g) > 0.4).float().to(DEV)
    w, bi = rnd(C, 1, g=g, scale=0.3), rnd(C, g=g, scale=0.3)
    G, Wbt, bbt = rnd(N, T, T, g=g, scale=0.2), rnd(B * T, C, C, g=g, scale=0.1), rnd(B * T, C, g=g)
    _, ab, wv = ops.encin_ht1_fwd(src, 1, mask, -0.7, w, bi, G, Wbt, bbt)
    dPre = rnd(B, T, N, C, g=g)
    return (dPre, src, mask, -0.7, w, bi, Wbt, ab, wv)


@pytest.fixture(scope="module", params=[17, 70], ids=["N17", "N70"])
def case(request):
    """per N: the table, its stand-alone results, and the hosts' inputs — computed once, left unchanged"""
    N = request.param
    g = torch.Generator().manual_seed(500 + N)
    tab = Table(N, g)
    pj, ref1, ref2 = tab.build()
    pj.launch()
    torch.cuda.synchronize()
    return dict(N=N, g=g, tab=tab, ref1=ref1, ref2=ref2, encin=_encin_inputs(N, g))


def test_encin_bwd_carries_a_table(case):
    from gptst_amd import ops
    ref = ops.encin_ht1_bwd(*case["encin"])
    for empty in (True, False):
        pj, k1, k2 = case["tab"].build()
        if empty:
            pj.jobs = []
        with Recorded() as rec:
            got = ops.encin_ht1_bwd(*case["encin"], jobs=pj)
        assert rec.names == ["gptst_encin_ht1_bwd"] and not pj.jobs
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
        if not empty:
            _check_tables(k1, k2, case["ref1"], case["ref2"])


@pytest.mark.parametrize("nsplit", [1, B], ids=["nsplit1", "nsplitB"])
def test_gram_bwd_carries_a_table(case, nsplit):
    from gptst_amd import ops
    N, L, Hm = case["N"], 3, 5
    g = torch.Generator().manual_seed(600 + N + nsplit)
    A, dG = rnd(L * N, Hm, T, g=g), rnd(L, nsplit, N, T, T, g=g)
    ref = ops.gram_bwd(A, dG, layers=L, nsplit=nsplit)
    for empty in (True, False):
        pj, k1, k2 = case["tab"].build()
        if empty:
            pj.jobs = []
        with Recorded() as rec:
            got = ops.gram_bwd(A, dG, layers=L, nsplit=nsplit, jobs=pj)
        assert rec.names == ["gptst_gram_bwd"] and not pj.jobs
        assert torch.equal(got, ref)
        if not empty:
            _check_tables(k1, k2, case["ref1"], case["ref2"])


def test_timefeat_bwd_carries_a_table(case):
    """two instances of different E (16 on B*T rows, 4 on B rows of 12 indices) next to the table"""
    from gptst_amd import ops
    g = torch.Generator().manual_seed(700 + case["N"])
    tidx = rnd(B, T, 2, g=g)

    def params(E, K):
        return [rnd(E, K, g=g), rnd(E, g=g), rnd(E, K, g=g), rnd(E, g=g), rnd(E, E, g=g), rnd(E, g=g), rnd(E, E, g=g), rnd(E, g=g), rnd(E, E, g=g),
                rnd(E, g=g)]
    inst = [(params(16, 1), B * T, 1), (params(4, T), B, T)]
    douts = [rnd(rows, pp[1].numel(), g=g) for pp, rows, K in inst]

    def tf():
        grads = [[torch.zeros_like(t) for t in pp] for pp, _, _ in inst]
        return [ops.TimefeatJob(pp, rows, K, gr, do) for (pp, rows, K), gr, do in zip(inst, grads, douts)], grads
    jobs, ref = tf()
    ops.timefeat_jobs_bwd(jobs, tidx)
    for empty in (True, False):
        pj, k1, k2 = case["tab"].build()
        if empty:
            pj.jobs = []
        jobs, got = tf()
        with Recorded() as rec:
            ops.timefeat_jobs_bwd(jobs, tidx, jobs=pj)
        assert rec.names == ["gptst_timefeat_jobs"] and not pj.jobs
        for q, (ga, gb) in enumerate(zip(got, ref)):
            for i, (a, b) in enumerate(zip(ga, gb)):
                torch.testing.assert_close(a, b, msg="time-feature instance %d tensor %d" % (q, i), **ATOMIC)
        if not empty:
            _check_tables(k1, k2, case["ref1"], case["ref2"])


@pytest.mark.parametrize("host", ["encin", "gram", "timefeat"])
def test_a_table_longer_than_one_launch_holds_is_applied_once(case, host):
    """PJ_MAX + 3 jobs of different weights, each with a target of its own: the heaviest PJ_MAX ride, the rest follow — every target equals the
    stand-alone launch's (a job applied twice, or not at all, does not)"""
    from gptst_amd import ops
    N = case["N"]
    g = torch.Generator().manual_seed(800 + N)
    n = PJ_MAX + 3
    rows = [1 + (7 * q) % 23 for q in range(n)]                 # 1 .. 23 partial rows: the cost order is not the call order
    xs = [rnd(r, 8, g=g) for r in rows]
    ones = [torch.ones(r, 1, device=DEV) for r in rows]

    def table():
        pj, outs = _pool_jobs(), [torch.zeros(1, 8, device=DEV) for _ in range(n)]
        for o, x, e in zip(outs, xs, ones):
            pj.bwd_pool(e, x, o)
        return pj, outs
    pj, ref = table()
    pj.launch()
    pj, outs = table()
    with Recorded() as rec:
        if host == "encin":
            ops.encin_ht1_bwd(*case["encin"], jobs=pj)
        elif host == "gram":
            ops.gram_bwd(rnd(N, 3, T, g=g), rnd(1, 1, N, T, T, g=g), jobs=pj)
        else:
            pp = [rnd(4, 1, g=g), rnd(4, g=g), rnd(4, 1, g=g), rnd(4, g=g), rnd(4, 4, g=g), rnd(4, g=g), rnd(4, 4, g=g), rnd(4, g=g), rnd(4, 4, g=g), rnd(4, g=g)]
            ops.timefeat_jobs_bwd([ops.TimefeatJob(pp, B * T, 1, [torch.zeros_like(t) for t in pp], rnd(B * T, 4, g=g))], rnd(B, T, 2, g=g), jobs=pj)
    assert len(rec.names) == 1 and not pj.jobs
    for q, (a, b) in enumerate(zip(outs, ref)):
        assert torch.equal(a, b), ("job", q, rows[q])


# ---- step level -----------------------------------------------------------------------------------------------------------------------
def _args(dataset, **over):
    return make_args(dataset, **dict(dict(scaler_zeros=synth.scaler_zeros(), epochs=30, change_epoch=3), **over))


def _step(args, Bs, tail, epoch, **kw):
    """one fused step from the seed-3 state with injected noise, the tail-role form switched by `tail` -> (gradients, losses, mask, launch names)"""
    from gptst_amd import engine
    keep = engine.TAIL_ROLES
    engine.TAIL_ROLES = tail
    try:
        grads, _, mask, names, st = one_step(args, Bs, epoch, sd_seed=3, inject=noise_inject(args, Bs, epoch), **kw)
    finally:
        engine.TAIL_ROLES = keep
    return grads, st.losses(), mask, names


HOSTS = ("gptst_encin_ht1_bwd", "gptst_gram_bwd", "gptst_timefeat_jobs")
SHAPES = [("PEMS08", 32, {}), ("METR_LA", 8, {}), ("PEMS08", 2, dict(num_nodes=24, embed_dim=8, HS=6, HT=8))]


@pytest.mark.parametrize("epoch", [1, 20], ids=["phase0", "phase1"])
@pytest.mark.parametrize("dataset,Bs,over", SHAPES, ids=["bench_N170_B32", "metr_la_N207", "small_N24"])
def test_tail_roles_step_equals_the_four_launches(dataset, Bs, over, epoch):
    args = _args(dataset, **over)
    assert args.hidden_dim == 64
    g0, l0, m0, n0 = _step(args, Bs, False, epoch)
    g1, l1, m1, n1 = _step(args, Bs, True, epoch)
    print("launches: off %d, on %d" % (len(n0), len(n1)))
    assert len(n1) == len(n0) - 1
    behind = lambda names: names[max(i for i, n in enumerate(names) if "route" in n and "bwd" in n) + 1:]      # noqa: E731  (the last routing backward)
    assert all(h in behind(n1) for h in HOSTS) and "gptst_pool_jobs" not in behind(n1), behind(n1)
    assert "gptst_pool_jobs" in behind(n0), behind(n0)
    assert torch.equal(m0, m1), "mask"
    assert l0 == l1, (l0, l1)
    for k in g0:
        if k.startswith(GUIDE_EMB):
            torch.testing.assert_close(g1[k], g0[k], msg=k, **ATOMIC)
        else:
            torch.testing.assert_close(g1[k], g0[k], rtol=2e-3, atol=1e-5, msg=k)


OTHER = {
    "deterministic": ("PEMS08", 2, dict(num_nodes=24, embed_dim=8, HS=6, HT=8), dict(deterministic=True)),
    "safe_mode": ("PEMS08", 2, dict(num_nodes=24, embed_dim=8, HS=6, HT=8), dict(safe_mode=True)),
    "no_carry_B128_N20": ("PEMS08", 128, dict(num_nodes=20, embed_dim=8, HS=5, HT=6, num_route=2), {}),
    "nyc_taxi_no_encin": ("NYC_TAXI", 4, {}, {}),
}


@pytest.mark.parametrize("name", list(OTHER))
def test_other_steps_enqueue_the_same_launches(name):
    dataset, Bs, over, kw = OTHER[name]
    args = _args(dataset, **over)
    _, l0, m0, n0 = _step(args, Bs, False, 20, **kw)
    _, l1, m1, n1 = _step(args, Bs, True, 20, **kw)
    assert n0 == n1
    assert torch.equal(m0, m1) and l0 == l1
