"""GATModel (models/full_graph.py:78-97) on the MI355X: the reference's own logits (tests/golden/g18_gat_h64.pt, written by
tests/golden/make_golden_gat.py) and the plain-torch restatement of tests/gat_graphs.py at the wider built widths."""
import pytest
import torch

import gnnome_amd
from gnnome_amd import ops
from gnnome_amd.models import GATModel

import gat_graphs as gg
from conftest import load_golden

pytestmark = pytest.mark.gpu

BAR = 1e-4          # the project's golden bar on edge probabilities (tests/test_hip_parity.py)


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("g18_gat_h64.pt")


@pytest.mark.parametrize("on_device", (False, True))
@pytest.mark.parametrize("directed", (True, False))
def test_reference_state_dict_loads_and_reproduces_the_reference_logits(golden, directed, on_device):
    g = golden
    m = GATModel(2, 2, g["hidden"], g["hidden_ne"], g["layers"], g["hs"], "batch", directed=directed)
    m.load_state_dict(g["state_dict"], strict=True)
    m.eval()
    x, e = (g["x"].to(dev()), g["e"].to(dev())) if on_device else (g["x"], g["e"])   # CPU inputs are staged, the logits come back
    if on_device:
        m.to(dev())
    got = m((g["src"], g["dst"], g["num_nodes"]), x, e)
    want = g["logits_directed" if directed else "logits_undirected"]
    assert got.shape == want.shape == (g["src"].numel(), 1) and got.device == x.device
    diff = gg.prob_diff(got, want)
    print(f"gat directed={directed} on_device={on_device}: max |dp| = {diff:.2e}")
    assert diff < BAR


def _model(hidden, hs, nl, directed, seed):
    m = GATModel(2, 2, hidden, 16, nl, hs, "batch", dropout=0.1, directed=directed)
    sd = gg.random_state_dict(m, seed=seed)
    m.load_state_dict(sd)
    return m.to(dev()).eval(), sd


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("hidden,hs", ((128, 32), (256, 128)))
def test_wider_models_match_the_plain_torch_restatement(hidden, hs, directed):
    n, e_cnt, nl = 40, 200, 2
    src, dst, x, e = gg.model_graph(n, e_cnt, seed=hidden)
    m, sd = _model(hidden, hs, nl, directed, seed=hidden + hs)
    got = m((src, dst, n), x.to(dev()), e.to(dev()))
    with torch.no_grad():
        want = gg.gat_model(sd, src, dst, n, x, e, nl, directed=directed)
    diff = gg.prob_diff(got, want)
    print(f"gat H={hidden} hs={hs} directed={directed}: max |dp| = {diff:.2e}")
    assert got.is_cuda and got.shape == (e_cnt, 1) and diff < BAR


@pytest.mark.parametrize("directed", (True, False))
def test_edge_order_reversed_views_and_a_graph_without_edges(directed):
    n, e_cnt, nl, hidden = 40, 200, 3, 64
    src, dst, x, e = gg.model_graph(n, e_cnt, seed=9)
    m, sd = _model(hidden, 64, nl, directed, seed=21)
    xd, ed = x.to(dev()), e.to(dev())
    with torch.no_grad():
        want = gg.gat_model(sd, src, dst, n, x, e, nl, directed=directed)
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    got = m(views, xd, ed)
    assert gg.prob_diff(got, want) < BAR
    assert torch.equal(got, m(views, xd, ed))                                   # two runs leave equal bits
    # a permuted edge list gives the same logits, permuted the same way
    perm = torch.randperm(e_cnt, generator=torch.Generator().manual_seed(2))
    got_p = m((src[perm], dst[perm], n), xd, ed[perm])
    assert gg.prob_diff(got_p, want[perm]) < BAR
    # views.reversed(): the model of the swapped edge list
    with torch.no_grad():
        want_r = gg.gat_model(sd, dst, src, n, x, e, nl, directed=directed)
    assert gg.prob_diff(m(views.reversed(), xd, ed), want_r) < BAR
    if directed:
        assert gg.prob_diff(want, want_r) > 1e-3                                # (the swap matters: the check above can tell)
    # every node has in-degree 0 - g' holds the loops only: nothing to score, and nothing faults
    none = torch.zeros(0, dtype=torch.int32)
    out = m((none, none, n), xd, torch.zeros(0, 2, device=dev()))
    assert out.shape == (0, 1)


def test_refusals_on_the_device_path():
    m = GATModel(2, 2, 64, 16, 1, 64, "batch", dropout=None).to(dev())   # (None means 0.0 here)
    src, dst, x, e = gg.model_graph(10, 30, seed=1)
    m.train()
    with pytest.raises(NotImplementedError, match="eval mode"):
        m((src, dst, 10), x.to(dev()), e.to(dev()))
    m.eval()
    assert m((src, dst, 10), x.to(dev()), e.to(dev())).shape == (30, 1)
    with pytest.raises(ValueError, match="rows"):
        m((src, dst, 10), x[:5].to(dev()), e.to(dev()))
    assert gnnome_amd.GATModel is GATModel
