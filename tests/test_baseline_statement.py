"""GCNModel / SAGEModel without a GPU: the plain-torch restatement the device tests compare with (tests/baseline_graphs.py) reproduces
the logits the reference's own classes produced (tests/golden/g17_baselines_h64.pt, written by tests/golden/make_golden_baselines.py),
and the modules here have the reference's state-dict keys and shapes."""
import pytest
import torch

import baseline_graphs as bg
from conftest import load_golden
from gnnome_amd.models import GCNModel, SAGEModel

STATEMENT_BAR = 1e-5      # SURVEY section 7's bar for a CPU restatement, on edge probabilities
MODELS = {"gcn": GCNModel, "sage": SAGEModel}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g17_baselines_h64.pt")


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("kind", ("gcn", "sage"))
def test_restatement_reproduces_the_reference_logits(golden, kind, directed):
    g, case = golden, golden["cases"][kind]
    with torch.no_grad():
        got = bg.baseline_model(kind, case["state_dict"], g["src"], g["dst"], g["num_nodes"], g["x"], g["e"], g["layers"], directed=directed)
    want = case["logits_directed" if directed else "logits_undirected"]
    assert got.shape == want.shape == (g["src"].numel(), 1)
    diff = bg.prob_diff(got, want)
    print(f"{kind} directed={directed}: max |dp| = {diff:.2e}")
    assert diff < STATEMENT_BAR
    # directed and undirected are different functions of the same parameters on this graph
    assert bg.prob_diff(case["logits_directed"], case["logits_undirected"]) > 1e-3


@pytest.mark.parametrize("kind", ("gcn", "sage"))
def test_modules_have_the_reference_state_dict_keys_and_shapes(golden, kind):
    g, case = golden, golden["cases"][kind]
    m = MODELS[kind](2, 2, g["hidden"], g["hidden_ne"], g["layers"], g["hs"], "batch")
    own = m.state_dict()
    assert list(own) == case["keys"] == list(case["state_dict"])
    assert [tuple(v.shape) for v in own.values()] == [tuple(s) for s in case["shapes"]]
    m.load_state_dict(case["state_dict"], strict=True)
    assert len(m.gnn.convs) == g["layers"]
    # the conv definitions' initialisation: zero biases, weights inside the Xavier-uniform bound (SAGEConv: with the ReLU gain)
    fresh, H = MODELS[kind](2, 2, g["hidden"], g["hidden_ne"], 1, g["hs"], "batch").gnn.convs[0], g["hidden"]
    assert torch.count_nonzero(fresh.bias) == 0
    for w, gain in ((fresh.weight, 1.0),) if kind == "gcn" else ((fresh.fc_self.weight, 2 ** 0.5), (fresh.fc_neigh.weight, 2 ** 0.5)):
        assert w.shape == (H, H) and 0 < w.abs().max().item() <= gain * (6.0 / (2 * H)) ** 0.5


def test_constructor_refusals_and_defaults_without_a_gpu():
    for cls in (GCNModel, SAGEModel):
        with pytest.raises(ValueError, match="64, 128, 256"):
            cls(2, 2, 96, 16, 2, 64, "batch")
        with pytest.raises(ValueError, match="32, 64, 128"):
            cls(2, 2, 64, 16, 2, 48, "batch")
        m = cls(2, 2, 64, 16, 2, 64, "batch")
        assert m.directed is True and cls(2, 2, 64, 16, 2, 64, "layer", None, False).directed is False
        m.train()
        with pytest.raises(NotImplementedError, match="eval mode"):
            m((torch.tensor([0]), torch.tensor([1]), 2), torch.zeros(2, 2), torch.zeros(1, 2))
    assert SAGEModel(2, 2, 64, 16, 2, 64, "batch", dropout=None).gnn.convs[0].feat_drop.p == 0.0
    assert SAGEModel(2, 2, 64, 16, 2, 64, "batch", dropout=0.25).gnn.convs[1].feat_drop.p == 0.25
