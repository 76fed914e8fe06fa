"""Which C-ABI calls does a downstream predictor's HIP forward + backward make, in which order — and what does it compute, bit for bit?

    python tools/downstream_trace.py [config ...] > trace.txt

For every configuration below: the predictor with backend="hip" in train mode from a fixed seed, one forward + backward; the ordered
(name, tag) of every call through ops._call (ops.TIMER), then one SHA-256 each of the output, the input gradient and every parameter
gradient in named_parameters order.  Only the public predictor classes are used, so two trees agree on what the predictors do exactly when
their outputs are identical line for line (tools/launch_trace.py does the same for the pretraining step).  A second or so of GPU time each.
"""
import hashlib
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gptst_amd import graph, ops  # noqa: E402
from gptst_amd.config import predictor_args  # noqa: E402
from gptst_amd.enhance import xavier_downstream_  # noqa: E402
from gptst_amd.predictors import ASTGCN, MSDR, MTGNN, STFGNN, STGCN, STGODE, STSGCN, TGCN  # noqa: E402

DEV = "cuda:0"
T, C = 12, 64


def stgcn(N):
    ap = SimpleNamespace(Ks=3, Kt=3, num_nodes=N, G=graph.stgcn_graph(graph.synthetic_adjacency(N, 2)), blocks1=[64, 32, 128], drop_prob=0, outputl_ks=3)
    return STGCN(ap, DEV, C, 1, backend="hip").to(DEV)


def tgcn(N):                                      # rnn_units 100: channels padded to 112
    ap = SimpleNamespace(num_nodes=N, input_window=T, output_window=T, rnn_units=100, output_dim=1, G=graph.tgcn_graph(graph.synthetic_adjacency(N, 2)))
    return TGCN(ap, DEV, C, backend="hip").to(DEV)


def mtgnn(N):                                     # dropout 0.3: the masked paths, the masks drawn on the device from the seed
    conf = vars(predictor_args("PEMS08", "MTGNN"))
    ap = SimpleNamespace(**{**conf, "num_nodes": N, "subgraph_size": min(conf["subgraph_size"], N), "dropout": 0.3}, adj_mx=None)
    return MTGNN(ap, DEV, C, 1, backend="hip").to(DEV)


def astgcn(N):
    ap = predictor_args("PEMS08", "ASTGCN")
    ap.num_nodes, ap.G = N, graph.astgcn_graph(graph.synthetic_adjacency(N, 2), ap.K)
    m = ASTGCN(ap, DEV, C, 1, backend="hip")
    xavier_downstream_(m)                         # the conf's xavier pass: the model has no other initial state
    with torch.no_grad():                         # and the score vectors centred, so that the sigmoids pass gradient
        for blk in m.BlockList:
            for p in (blk.TAt.U1, blk.TAt.U3, blk.SAt.W1, blk.SAt.W3):
                p.copy_(0.25 * (p - 0.5))
    return m


def stsgcn(N):                                    # the conf's four layers of [64, 64, 64], GLU, a weight per window
    ap = predictor_args("PEMS08", "STSGCN")
    a = graph.synthetic_adjacency(N, 2)
    ap.num_nodes, ap.A = N, a / a.sum(1, keepdims=True)       # rows normalised: a raw adjacency grows the activations layer by layer
    m = STSGCN(ap, DEV, C, 1, backend="hip")
    with torch.no_grad():                         # non-zero position embeddings, as after training: at zero they hide an omitted add
        for k, p in m.named_parameters():
            if k.endswith("_emb"):
                p.normal_(0, 0.3)
    return m


def stfgnn(N):                                    # the conf's three layers of [64, 64, 64], GLU, a weight per window
    ap = predictor_args("PEMS08", "STFGNN")
    s, d = graph.synthetic_adjacency(N, 2), graph.synthetic_adjacency(N, 5)
    d = ((d + d.T) > 0).astype("float32")
    s, d = s / s.sum(1, keepdims=True), d / d.sum(1, keepdims=True)       # rows normalised, as for STSGCN; the temporal graph symmetric
    d[range(N), range(N)] = 1.0                                           # with a unit diagonal, as graph.dtw_graph gives it
    ap.num_nodes, ap.adj = N, graph.stfgnn_fusion_graph(s, d)
    m = STFGNN(ap, DEV, C, backend="hip")
    with torch.no_grad():                         # position embeddings of the size they have after training
        for k, p in m.named_parameters():
            if k.endswith("_embedding"):
                p.normal_(0, 0.3)
    return m


def stgode(N):                                    # the conf's n_layers = 3 on two normalised graphs, under the xavier redraw the confs ask for
    ap = predictor_args("PEMS08", "STGODE")
    s, d = graph.synthetic_adjacency(N, 2), graph.synthetic_adjacency(N, 5)
    ap.num_nodes, ap.A_sp_wave, ap.A_se_wave = N, graph.stgode_normalized_adj(s), graph.stgode_normalized_adj(((d + d.T) > 0).astype("float32"))
    return xavier_downstream_(STGODE(ap, DEV, C, 1, backend="hip"))


def msdr(N):                                      # the conf's 2 + 2 layers of pre_k = 4 states; rnn_units 100: channels padded to 112
    ap = predictor_args("PEMS08", "MSDR")
    ap.num_nodes, ap.rnn_units = N, 100
    ap.supports = graph.msdr_supports(graph.synthetic_adjacency(N, 2), ap.filter_type)
    m = MSDR(ap, DEV, C, backend="hip")
    with torch.no_grad():                         # W, b, R off their zero initialisation: at it every state is 0 and a wrong product hides
        for c in m.cells():
            c.W.normal_(0, 1 / 32)
            c.b.normal_(0, 0.1)
            c.R.normal_(0, 0.1)
    return m


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(make, B, N):
    torch.manual_seed(0)
    m = make(N).train()
    x = torch.randn(B, T, N, C, device=DEV, requires_grad=True)
    y = m(x)                                      # (untraced: the first call loads the library)
    w = torch.randn_like(y)
    for p in m.parameters():
        p.grad = None
    x.grad = None
    torch.manual_seed(1)
    ops.TIMER = []
    try:
        y = m(x)
        (y * w).sum().backward()
        torch.cuda.synchronize()
        calls = [rec[:2] for rec in ops.TIMER]
    finally:
        ops.TIMER = None
    assert m.backend_used == "hip"
    print("-- forward + backward: %d calls" % len(calls))
    for name, tag in calls:
        print("   %s %s" % (name, tag))
    print("-- sha256 y %s" % sha(y))
    print("-- sha256 dx %s" % sha(x.grad))
    for k, p in m.named_parameters():
        print("-- sha256 d %s %s" % (k, "none" if p.grad is None else sha(p.grad)))


CONFIGS = {}
for _name, _make in (("stgcn", stgcn), ("tgcn", tgcn), ("mtgnn", mtgnn), ("astgcn", astgcn), ("stsgcn", stsgcn), ("stfgnn", stfgnn), ("stgode", stgode),
                     ("msdr", msdr)):
    CONFIGS[_name + "_b2_n37"] = lambda make=_make: run(make, 2, 37)            # a padded node tile, several row tiles
    CONFIGS[_name + "_b1_n170"] = lambda make=_make: run(make, 1, 170)

if __name__ == "__main__":
    for name in sys.argv[1:] or list(CONFIGS):
        print("==== %s" % name, flush=True)
        CONFIGS[name]()
        sys.stdout.flush()
