"""Downstream CCRNN predictor against golden vectors generated from the reference implementation (tests/golden/make_golden_ccrnn.py:
reference model/CCRNN_demand/CCRNN.py, args.py): the argument set of the two demand confs and the refusal of every other dataset, the
parameter tree in the reference's order at three layer settings, the seeded initialisation (the SVD's node vectors up to sign), the output
and every gradient with and without teacher forcing (in float64, off the initialisation: ccrnn_util.perturb_), the None and zero gradient
pattern, the support, the backend switch, the front end's hand-over of the targets and Run.py's dispatch."""
import importlib.util
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ccrnn_util as gu
from gptst_amd import config, graph
from gptst_amd.config import make_args, predictor_args
from gptst_amd.predictors import CCRNN
from golden_util import load

G = load("ccrnn_small.npz")
TOL = 1e-5                 # largest absolute error over the reference tensor's largest magnitude (both sides float64: the bound of test_predictor_stmgcn.py)
B, T, N, C, OUT, H, ND, K = 2, 12, 20, 64, 2, 25, 10, 3
NOGRAD = ["w1", "w2", "b1", "b2"]


def _cell_keys(prefix, gconv):
    return ["%s.%s.%s" % (prefix, conv, k) for conv in ("ru_gate_g_conv", "candidate_g_conv")
            for k in ["graphconv.%d.out.%s" % (i, wb) for i in range(gconv) for wb in ("weight", "bias")] + ["attlinear.weight", "attlinear.bias"]]


def _keys(rnn, gconv):
    return (["nodevec1", "nodevec2", "w1", "w2", "b1", "b2"] + [k for l in range(rnn) for k in _cell_keys("encoder.%d" % l, gconv)]
            + [k for l in range(rnn) for k in _cell_keys("decoder.%d" % l, gconv)] + ["decoder.out.weight", "decoder.out.bias"])


def _ap(rnn=1, gconv=1, **kw):
    return gu.model_args(N, G["support"], rnn=rnn, gconv=gconv, **kw)


def _err(got, ref):
    ref = torch.as_tensor(ref).detach().double()
    return float((got.detach().double().reshape(ref.shape) - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _golden_model(rnn=1, gconv=1, backend="torch"):
    m = CCRNN(_ap(rnn, gconv), "cpu", C, OUT, backend=backend)
    pre = gu.tag(rnn, gconv) + ".sd."
    m.load_state_dict({k[len(pre):]: torch.tensor(G[k]) for k in G.files if k.startswith(pre)}, strict=True)
    return m


@pytest.mark.parametrize("ds,n,layers", [("NYC_TAXI", 266, 1), ("NYC_BIKE", 250, 2)])
def test_confs_parse_to_the_reference_values(ds, n, layers):
    pa = predictor_args(ds, "CCRNN")
    assert (pa.num_nodes, pa.n_rnn_layers, pa.num_input, pa.num_predict) == (n, layers, 12, 12) and make_args(ds).num_nodes == n
    assert (pa.n_dim, pa.hidden_size, pa.n_supports, pa.k_hop, pa.n_gconv_layers, pa.cl_decay_steps, pa.hidden_size_data) == (50, 25, 1, 3, 1, 300, 20)
    assert (pa.normalized_category, pa.Normal_Method, pa.input_dim, pa.output_dim) == ("randomwalk", "Standard", 2, 2)
    assert (pa.seed, pa.seed_mode, pa.xavier, pa.loss_func, pa.batch_size) == (12, True, False, "mask_mae", 64)
    over = predictor_args(ds, "CCRNN", ["--hidden_size", "32", "--k_hop", "1"])
    assert over.hidden_size == 32 and over.k_hop == 1 and over.num_nodes == n
    assert config._PRED_DIRS["CCRNN"] == "CCRNN_demand"


@pytest.mark.parametrize("ds", ["PEMS08", "METR_LA"])
def test_other_datasets_are_refused_with_the_references_message(ds):
    with pytest.raises(ValueError, match="Demand prediction baseline. Please select NYC_TAXI or NYC_BIKE dataset!"):
        predictor_args(ds, "CCRNN")


def test_gwn_is_still_refused_and_the_message_names_ccrnn():
    with pytest.raises(ValueError) as e:
        predictor_args("PEMS08", "GWN")
    assert all(name in str(e.value) for name in ("STGCN", "TGCN", "MTGNN", "ASTGCN", "STSGCN", "STFGNN", "STGODE", "MSDR", "STWA", "STMGCN", "CCRNN"))


@pytest.mark.parametrize("rnn,gconv,count", [(1, 1, 24), (2, 1, 40), (1, 3, 40)])
def test_state_dict_is_the_reference_tree(rnn, gconv, count):
    m = CCRNN(_ap(rnn, gconv), "cpu", C, OUT)
    keys = [str(k) for k in G[gu.tag(rnn, gconv) + ".init.keys"]]
    assert len(keys) == count and keys == _keys(rnn, gconv) and list(m.state_dict()) == keys and len(list(m.parameters())) == count
    sd = m.state_dict()
    for k in keys:
        assert tuple(sd[k].shape) == tuple(G["%s.init.%s" % (gu.tag(rnn, gconv), k)].shape), k
    assert tuple(sd["nodevec1"].shape) == (N, ND) and tuple(sd["nodevec2"].shape) == (ND, N) and tuple(sd["w1"].shape) == (ND, ND)
    assert tuple(sd["encoder.0.ru_gate_g_conv.graphconv.0.out.weight"].shape) == (2 * H, (C + H) * (K + 1))
    assert tuple(sd["decoder.0.candidate_g_conv.graphconv.0.out.weight"].shape) == (H, (OUT + H) * (K + 1))
    assert tuple(sd["encoder.0.ru_gate_g_conv.attlinear.weight"].shape) == (1, N * 2 * H) and tuple(sd["decoder.out.weight"].shape) == (OUT, H)
    assert m.takes_targets is True and not list(m.named_buffers())


def test_construction_refusals_and_k_hop_zero():
    with pytest.raises(ValueError, match="n_dim"):
        CCRNN(_ap(n_dim=N + 1), "cpu", C, OUT)
    with pytest.raises(ValueError, match="n_gconv_layers"):
        CCRNN(_ap(gconv=4), "cpu", C, OUT)
    with pytest.raises(ValueError, match="support"):
        CCRNN(gu.model_args(N + 1, G["support"]), "cpu", C, OUT)
    m = CCRNN(_ap(k_hop=0), "cpu", C, OUT)
    assert tuple(m.encoder[0].ru_gate_g_conv.graphconv[0].out.weight.shape) == (2 * H, C + H)
    assert tuple(m(torch.zeros(1, T, N, C)).shape) == (1, T, N, OUT)


@pytest.mark.parametrize("rnn,gconv", gu.LAYERS)
def test_seeded_construction_equals_the_reference(rnn, gconv):
    torch.manual_seed(int(G["seed"]))
    sd = CCRNN(_ap(rnn, gconv), "cpu", C, OUT).state_dict()
    pre = gu.tag(rnn, gconv) + ".init."
    for k in sd:
        if not k.startswith("nodevec"):
            assert torch.equal(sd[k], torch.tensor(G[pre + k])), k
    v1, v2 = torch.tensor(G[pre + "nodevec1"]), torch.tensor(G[pre + "nodevec2"])
    assert _err(sd["nodevec1"] @ sd["nodevec2"], (v1 @ v2).double()) < 1e-5
    for j in range(ND):                                                        # a singular vector pair is defined up to one common sign
        s = 1.0 if float((sd["nodevec1"][:, j] * v1[:, j]).sum()) > 0 else -1.0
        assert _err(s * sd["nodevec1"][:, j], v1[:, j]) < 1e-4 and _err(s * sd["nodevec2"][j], v2[j]) < 1e-4, j
    assert torch.equal(sd["w1"], torch.eye(ND)) and not bool(sd["b2"].any())


@pytest.mark.parametrize("run", ["free", "tf"])
@pytest.mark.parametrize("rnn,gconv", gu.LAYERS)
def test_torch_backend_reproduces_the_vectors(rnn, gconv, run):
    m = _golden_model(rnn, gconv).double().train()
    pre = "%s.%s." % (gu.tag(rnn, gconv), run)
    x = torch.tensor(G["x"]).double().requires_grad_(True)
    random.seed(int(G["tf_seed"]))
    before = random.getstate()
    y = m(x, torch.tensor(G["targets"]).double() if run == "tf" else None, None)
    after = random.getstate()
    random.setstate(before)
    for _ in range(int(G[pre + "draws"])):
        random.random()
    assert random.getstate() == after and int(G[pre + "draws"]) == (T if run == "tf" else 0)      # exactly num_predict draws with targets, none without
    assert m.backend_used == "torch" and tuple(y.shape) == (B, T, N, OUT)
    (y * torch.tensor(G["w"]).double()).sum().backward()
    assert _err(y, G[pre + "y"]) < TOL and _err(x.grad, G[pre + "dx"]) < TOL
    none = [str(k) for k in G[pre + "none"]]
    assert none == (NOGRAD if gconv == 1 else [])
    for k, p in m.named_parameters():
        if k in none:
            assert p.grad is None, k                                          # graph-conv layer 0 reads graph 0 alone
            continue
        ref = G[pre + "grad." + k]
        if gconv == 1 and "attlinear" in k:
            assert not np.any(ref) and not bool(p.grad.any()), k               # the softmax over one entry: exactly zero
        elif k.endswith("attlinear.bias"):
            assert float(np.abs(ref).max()) < 1e-12 and float(p.grad.abs().max()) < 1e-12, k      # one bias under every logit: zero but for rounding
        else:
            assert float(np.abs(ref).max()) > 0 and _err(p.grad, ref) < TOL, k


def test_sampling_threshold_serves_a_caller_that_passes_batch_seen():
    m = _golden_model()
    assert m._compute_sampling_threshold(0) == 300 / 301 and abs(m._compute_sampling_threshold(3000) - 300 / (300 + np.exp(10))) < 1e-15
    x, t = torch.tensor(G["x"]), torch.tensor(G["targets"])
    with torch.no_grad():
        for seen in (None, 1700):                                             # the constant 0.5, and 300 / (300 + e^(17 / 3)) = 0.509
            thr = 0.5 if seen is None else m._compute_sampling_threshold(seen)
            random.seed(5)
            forced = [random.random() < thr for _ in range(T)]
            g = m.graphs()
            want = m.decoder(g, m.encoder(x, g), t, forced=forced)
            random.seed(5)
            assert torch.equal(m(x, t, seen), want) and any(forced) and not all(forced)


@pytest.mark.parametrize("cat", ["randomwalk", "none"])
def test_support_matches_the_reference(cat):
    x = np.stack([G["sup.pick"], G["sup.drop"]], axis=2)
    s = graph.ccrnn_support(x, normalized_category=cat, **gu.SUPPORT_CASE)
    assert s.shape == (N, N) and s.dtype == np.float64 and not np.any(np.diag(s))
    if cat == "randomwalk":
        assert np.abs(s - G["sup.matrix"]).max() / np.abs(G["sup.matrix"]).max() < 1e-9
        assert np.abs(s.sum(1) - 1).max() < 1e-12
    else:
        rw = s / s.sum(1, keepdims=True)
        assert np.abs(rw - G["sup.matrix"]).max() / np.abs(G["sup.matrix"]).max() < 1e-9 and np.abs(s - s.T).max() < 1e-12


def test_support_refusals():
    x = np.stack([G["sup.pick"], G["sup.drop"]], axis=2)
    with pytest.raises(ValueError, match="laplacian"):
        graph.ccrnn_support(x, 6, "laplacian", 10)
    with pytest.raises(ValueError, match="holdout"):
        graph.ccrnn_support(x, 6, "randomwalk", x.shape[0])
    with pytest.raises(ValueError, match=r"\(T, N, 2\)"):
        graph.ccrnn_support(x[..., 0], 6, "randomwalk", 10)


def test_backend_switch_and_defaults():
    assert config.FINETUNE_DEFAULTS["ccrnn_backend"] == "torch" and make_args("NYC_TAXI").ccrnn_backend == "torch"
    base = ["-dataset", "NYC_TAXI", "-mode", "eval", "-model", "CCRNN"]
    assert config.parse_args("cpu", base).ccrnn_backend == "torch"
    assert config.parse_args("cpu", base + ["-ccrnn_backend", "hip"]).ccrnn_backend == "hip"
    with pytest.raises(SystemExit):
        config.parse_args("cpu", base + ["-ccrnn_backend", "triton"])
    with pytest.raises(ValueError):
        CCRNN(_ap(), "cpu", C, OUT, backend="triton")
    assert CCRNN(_ap(), "cpu", C, OUT).backend == "torch"


@pytest.mark.parametrize("targets", [False, True])
def test_hip_backend_on_a_cpu_input_takes_the_torch_path_bit_equally(targets):
    a, b = _golden_model(backend="hip").train(), _golden_model(backend="torch").train()
    x, t = torch.tensor(G["x"]).float(), torch.tensor(G["targets"]).float() if targets else None
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    random.seed(11)
    ya = a(xa, t)
    random.seed(11)
    yb = b(xb, t)
    assert (a.backend, a.backend_used, b.backend_used) == ("hip", "torch", "torch") and torch.equal(ya, yb)
    ya.square().sum().backward()
    yb.square().sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert (p.grad is None and q.grad is None) if k in NOGRAD else torch.equal(p.grad, q.grad), k


def test_front_end_hands_targets_to_this_predictor_only(monkeypatch):
    from gptst_amd import enhance
    args = make_args("NYC_TAXI", mode="eval", num_nodes=N, scaler_zeros=0.0)
    eb = torch.randn(B, T, N, args.hidden_dim)
    monkeypatch.setattr(enhance, "fusion_gate", lambda *a, **k: eb)

    class Stub(torch.nn.Module):
        def forward(self, source, label):
            return (torch.zeros(1),)

    class Plain(torch.nn.Module):
        def forward(self, *a):
            self.got = a
            return a[0]

    class Takes(Plain):
        takes_targets = True

    label = torch.randn(B, T, N, args.input_base_dim + 3)
    for cls in (Plain, Takes):
        fe = enhance.EnhanceFrontEnd(args, predictor=cls())
        fe.pretrain_model = Stub()
        out = fe(torch.zeros(B, T, N, args.input_base_dim + 2), label)
        assert len(out) == 5 and out[0] is eb
        if cls is Plain:
            assert len(fe.predictor.got) == 1 and fe.predictor.got[0] is eb
        else:
            got = fe.predictor.got
            assert len(got) == 3 and got[0] is eb and torch.equal(got[1], label[..., :args.input_base_dim]) and got[2] is None
            fe(torch.zeros(B, T, N, args.input_base_dim + 2), None)
            assert fe.predictor.got[1] is None and fe.predictor.got[2] is None


def test_run_py_dispatches_ccrnn(tmp_path, capsys):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpt-st_amd", "Run.py")
    spec = importlib.util.spec_from_file_location("gptst_run_for_ccrnn_test", path)
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    assert "CCRNN" in run.EVAL_MODELS and "GWN" not in run.EVAL_MODELS and run.CCRNN_HOLDOUT == 1700
    src = open(path).read()
    assert 'str(args.model) == "CCRNN"' in src and "ccrnn_support(args, pargs, data_root" in src and "args.ccrnn_backend" in src
    pargs = SimpleNamespace(hidden_size_data=6, normalized_category="randomwalk")
    raw = np.stack([G["sup.pick"], G["sup.drop"], np.zeros_like(G["sup.pick"])], axis=2)
    from gptst_amd import data as gdata
    os.makedirs(tmp_path / "NYC_TAXI")
    np.savez(os.path.join(str(tmp_path), gdata.DATASETS["NYC_TAXI"][0]), data=raw)
    a = SimpleNamespace(dataset="NYC_TAXI")
    loaders = (SimpleNamespace(series=torch.tensor(raw[:40]).float()), None, None)
    scaler = SimpleNamespace(mean=0.0, std=1.0)
    s = run.ccrnn_support(a, pargs, str(tmp_path), loaders, scaler, holdout=10)              # the raw file, all but the held-out frames
    assert s.dtype == torch.float32 and _err(s, G["sup.matrix"]) < 1e-6 and "training split" not in capsys.readouterr().out
    s2 = run.ccrnn_support(a, pargs, str(tmp_path), loaders, scaler)                          # 60 frames cannot hold 1700 out: the project's fallback
    said = capsys.readouterr().out
    assert said.count("\n") == 1 and "training split" in said
    assert _err(s2, graph.ccrnn_support(raw[:40, :, :2], 6, "randomwalk", 0)) < 1e-6
