"""The row layer the HIP predictors share (predictors/rows_hip.py), without a GPU: the padded-graph cache on the two graph ranks it serves."""
import types

import pytest
import torch

from gptst_amd import graph
from gptst_amd.predictors import STGCN, TGCN, rows_hip as R

N = 20


def _tgcn_owner():
    ap = types.SimpleNamespace(num_nodes=N, input_window=12, output_window=12, rnn_units=32, output_dim=1,
                               G=graph.tgcn_graph(graph.synthetic_adjacency(N, 2)))
    cell = TGCN(ap, "cpu", 64, backend="hip").tgcn_model
    return cell, "L", 1


def _stgcn_owner():
    ap = types.SimpleNamespace(Ks=3, Kt=3, num_nodes=N, G=graph.stgcn_graph(graph.synthetic_adjacency(N, 2)), blocks1=[64, 32, 128], drop_prob=0,
                               outputl_ks=3)
    return STGCN(ap, "cpu", 64, 1, backend="hip").st_conv1.sconv, "Lk", 3


@pytest.mark.parametrize("make", [_tgcn_owner, _stgcn_owner], ids=["tgcn_2d", "stgcn_3d"])
def test_padded_graph_cache(make):
    owner, attr, ks = make()
    g = getattr(owner, attr)
    assert g.dim() == (2 if ks == 1 else 3)
    lp, lpt = R.padded_graph(owner, g, "_lp_cache", True)
    assert lp.shape == (ks, 32, 32) and torch.equal(lp[:, :N, :N], g.reshape(ks, N, N))
    assert float(lp[:, N:].abs().max()) == 0 and float(lp[:, :, N:].abs().max()) == 0
    assert lpt.is_contiguous() and torch.equal(lpt, lp.transpose(1, 2)) and not torch.equal(lpt, lp)
    again = R.padded_graph(owner, g, "_lp_cache", True)
    assert again[0] is lp and again[1] is lpt                           # the same objects on a second call
    with torch.no_grad():
        g.mul_(2)                                                       # written in place: rebuilt
    lp2, lpt2 = R.padded_graph(owner, g, "_lp_cache", True)
    assert lp2 is not lp and torch.equal(lp2[:, :N, :N], g.reshape(ks, N, N)) and lpt2.is_contiguous() and torch.equal(lpt2, lp2.transpose(1, 2))
    setattr(owner, attr, g.clone())                                     # the buffer replaced by an equal one: rebuilt
    g3 = getattr(owner, attr)
    lp3, lpt3 = R.padded_graph(owner, g3, "_lp_cache", True)
    assert lp3 is not lp2 and torch.equal(lp3, lp2) and lpt3.is_contiguous() and torch.equal(lpt3, lp3.transpose(1, 2))
    assert R.padded_graph(owner, g3, "_lp_cache", True)[0] is lp3


def test_pad16_and_the_shared_checks():
    assert [R.pad16(n) for n in (1, 16, 17, 170)] == [16, 16, 32, 176]
    assert R.nodemix_fits(1136) and not R.nodemix_fits(1137)            # 1136 * 36 * 4 = 163584 <= 160 KB < 1152 * 36 * 4
    assert R.widths_ok([16, 64, 128]) and not R.widths_ok([64, 8]) and not R.widths_ok([144]) and not R.widths_ok([24])
    assert not R.is_hip_input(torch.zeros(1, 2, 3, 16))                 # a CPU tensor
