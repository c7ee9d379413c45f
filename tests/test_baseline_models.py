"""GCNModel and SAGEModel (models/full_graph.py:56-75, :100-119) on the MI355X: the reference's own logits
(tests/golden/g17_baselines_h64.pt, written by tests/golden/make_golden_baselines.py) and the plain-torch restatement of
tests/baseline_graphs.py at the wider built widths."""
import pytest
import torch

import gnnome_amd
from gnnome_amd import engine_baselines, ops
from gnnome_amd.models import GCNModel, SAGEModel

import baseline_graphs as bg
from conftest import load_golden

pytestmark = pytest.mark.gpu

BAR = 1e-4          # the project's golden bar on edge probabilities (tests/test_hip_parity.py)
MODELS = {"gcn": GCNModel, "sage": SAGEModel}


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("g17_baselines_h64.pt")


@pytest.mark.parametrize("on_device", (False, True))
@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("kind", ("gcn", "sage"))
def test_reference_state_dict_loads_and_reproduces_the_reference_logits(golden, kind, directed, on_device):
    g, case = golden, golden["cases"][kind]
    m = MODELS[kind](2, 2, g["hidden"], g["hidden_ne"], g["layers"], g["hs"], "batch", directed=directed)
    m.load_state_dict(case["state_dict"], strict=True)
    m.eval()
    x, e = (g["x"].to(dev()), g["e"].to(dev())) if on_device else (g["x"], g["e"])   # CPU inputs are staged, the logits come back
    if on_device:
        m.to(dev())
    got = m((g["src"], g["dst"], g["num_nodes"]), x, e)
    want = case["logits_directed" if directed else "logits_undirected"]
    assert got.shape == want.shape == (g["src"].numel(), 1) and got.device == x.device
    diff = bg.prob_diff(got, want)
    print(f"{kind} directed={directed} on_device={on_device}: max |dp| = {diff:.2e}")
    assert diff < BAR


def _model(kind, hidden, hs, nl, directed, seed):
    m = MODELS[kind](2, 2, hidden, 16, nl, hs, "batch", dropout=0.1, directed=directed)
    sd = bg.random_state_dict(m, seed=seed)
    m.load_state_dict(sd)
    return m.to(dev()).eval(), sd


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("hidden,hs", ((128, 32), (256, 128)))
@pytest.mark.parametrize("kind", ("gcn", "sage"))
def test_wider_models_match_the_plain_torch_restatement(kind, hidden, hs, directed):
    n, e_cnt, nl = 40, 200, 2
    src, dst, x, e = bg.model_graph(n, e_cnt, seed=hidden)
    m, sd = _model(kind, hidden, hs, nl, directed, seed=hidden + hs)
    got = m((src, dst, n), x.to(dev()), e.to(dev()))
    with torch.no_grad():
        want = bg.baseline_model(kind, sd, src, dst, n, x, e, nl, directed=directed)
    diff = bg.prob_diff(got, want)
    print(f"{kind} H={hidden} hs={hs} directed={directed}: max |dp| = {diff:.2e}")
    assert got.is_cuda and got.shape == (e_cnt, 1) and diff < BAR


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("kind", ("gcn", "sage"))
def test_edge_order_reversed_views_and_a_graph_without_edges(kind, directed):
    n, e_cnt, nl, hidden = 40, 200, 3, 64
    src, dst, x, e = bg.model_graph(n, e_cnt, seed=9)
    m, sd = _model(kind, hidden, 64, nl, directed, seed=21)
    xd, ed = x.to(dev()), e.to(dev())
    with torch.no_grad():
        want = bg.baseline_model(kind, sd, src, dst, n, x, e, nl, directed=directed)
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    got = m(views, xd, ed)
    assert bg.prob_diff(got, want) < BAR
    assert torch.equal(got, m(views, xd, ed))                                   # two runs leave equal bits
    # the scale vectors are made once per (graph, directed) and kept with the views
    assert engine_baselines.scales_for(views, directed) is engine_baselines.scales_for(views, directed)
    # a permuted edge list gives the same logits, permuted the same way
    perm = torch.randperm(e_cnt, generator=torch.Generator().manual_seed(2))
    got_p = m((src[perm], dst[perm], n), xd, ed[perm])
    assert bg.prob_diff(got_p, want[perm]) < BAR
    # views.reversed(): the model of the swapped edge list
    with torch.no_grad():
        want_r = bg.baseline_model(kind, sd, dst, src, n, x, e, nl, directed=directed)
    assert bg.prob_diff(m(views.reversed(), xd, ed), want_r) < BAR
    if directed:
        assert bg.prob_diff(want, want_r) > 1e-3                                # (the swap matters: the check above can tell)
    # every node has in-degree 0 - g' holds the loops only: nothing to score, and nothing faults
    none = torch.zeros(0, dtype=torch.int32)
    out = m((none, none, n), xd, torch.zeros(0, 2, device=dev()))
    assert out.shape == (0, 1)


def test_a_graph_whose_nodes_see_only_their_loops_scores_like_the_restatement():
    """A bipartite graph, six edges from nodes 0..5 to nodes 6..11: every source has in-degree 0, so in g' it sees its own loop alone,
    and every target sees exactly one neighbour and itself."""
    n, hidden, nl = 12, 64, 2
    src = torch.arange(0, 6, dtype=torch.int32)
    dst = torch.arange(6, 12, dtype=torch.int32)
    g = torch.Generator().manual_seed(4)
    x, e = torch.rand(n, 2, generator=g), torch.randn(6, 2, generator=g)
    for kind in ("gcn", "sage"):
        m, sd = _model(kind, hidden, 64, nl, True, seed=5)
        with torch.no_grad():
            want = bg.baseline_model(kind, sd, src, dst, n, x, e, nl, directed=True)
        assert bg.prob_diff(m((src, dst, n), x, e), want) < BAR


def test_refusals_on_the_device_path():
    for cls in (GCNModel, SAGEModel):
        with pytest.raises(ValueError, match="64, 128, 256"):
            cls(2, 2, 96, 16, 2, 64, "batch")
        with pytest.raises(ValueError, match="32, 64, 128"):
            cls(2, 2, 64, 16, 2, 48, "batch")
        m = cls(2, 2, 64, 16, 1, 64, "batch", dropout=None).to(dev())   # (SAGEModel: None means 0.0 here)
        src, dst, x, e = bg.model_graph(10, 30, seed=1)
        m.train()
        with pytest.raises(NotImplementedError, match="eval mode"):
            m((src, dst, 10), x.to(dev()), e.to(dev()))
        m.eval()
        assert m((src, dst, 10), x.to(dev()), e.to(dev())).shape == (30, 1)
        with pytest.raises(ValueError, match="rows"):
            m((src, dst, 10), x[:5].to(dev()), e.to(dev()))
        with pytest.raises(NotImplementedError, match="GCNModel / SAGEModel"):
            m.gnn(None, None, None)
    assert gnnome_amd.GCNModel is GCNModel and gnnome_amd.SAGEModel is SAGEModel
