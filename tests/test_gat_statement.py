"""GATModel without a GPU: the plain-torch restatement the device tests compare with (tests/gat_graphs.py) reproduces the logits the
reference's own class produced (tests/golden/g18_gat_h64.pt, written by tests/golden/make_golden_gat.py), and the modules here have the
reference's state-dict keys, shapes and initialisation."""
import pytest
import torch

import gat_graphs as gg
from conftest import load_golden
from gnnome_amd.layers import GAT_processor, GATConv
from gnnome_amd.models import GATModel

STATEMENT_BAR = 1e-5      # SURVEY section 7's bar for a CPU restatement, on edge probabilities (tests/test_baseline_statement.py)


@pytest.fixture(scope="module")
def golden():
    return load_golden("g18_gat_h64.pt")


@pytest.mark.parametrize("directed", (True, False))
def test_restatement_reproduces_the_reference_logits(golden, directed):
    g = golden
    with torch.no_grad():
        got = gg.gat_model(g["state_dict"], g["src"], g["dst"], g["num_nodes"], g["x"], g["e"], g["layers"], directed=directed)
    want = g["logits_directed" if directed else "logits_undirected"]
    assert got.shape == want.shape == (g["src"].numel(), 1)
    diff = gg.prob_diff(got, want)
    print(f"gat directed={directed}: max |dp| = {diff:.2e}")
    assert diff < STATEMENT_BAR


def test_directed_and_undirected_are_different_functions(golden):
    assert gg.prob_diff(golden["logits_directed"], golden["logits_undirected"]) > 1e-3


def test_module_has_the_reference_state_dict_keys_and_shapes(golden):
    g = golden
    m = GATModel(2, 2, g["hidden"], g["hidden_ne"], g["layers"], g["hs"], "batch")
    own = m.state_dict()
    assert list(own) == g["keys"] == list(g["state_dict"])
    assert [tuple(v.shape) for v in own.values()] == [tuple(s) for s in g["shapes"]]
    m.load_state_dict(g["state_dict"], strict=True)
    assert len(m.gnn.convs) == len(m.gnn.linears) == g["layers"]
    H = g["hidden"]
    assert [k for k in own if k.startswith("gnn.convs.0.")] == ["gnn.convs.0." + t for t in ("attn_l", "attn_r", "bias", "fc.weight")]
    assert own["gnn.convs.0.fc.weight"].shape == (3 * H, H) and own["gnn.convs.0.attn_l"].shape == (1, 3, H)
    assert own["gnn.convs.0.bias"].shape == (3 * H,) and own["gnn.linears.1.weight"].shape == (H, 3 * H)


def test_a_fresh_conv_has_a_zero_bias_and_xavier_normal_weights():
    torch.manual_seed(0)
    conv = GATModel(2, 2, 64, 16, 1, 64, "batch").gnn.convs[0]
    assert torch.count_nonzero(conv.bias) == 0
    assert torch.count_nonzero(conv.attn_l) == conv.attn_l.numel() and torch.count_nonzero(conv.attn_r) == conv.attn_r.numel()
    # Xavier normal with the ReLU gain: std = sqrt(2) * sqrt(2 / (fan_in + fan_out)); fc [192, 64]: 0.125 (12 288 samples: within 5 %)
    assert abs(conv.fc.weight.std().item() - 0.125) < 0.05 * 0.125
    assert conv.negative_slope == 0.2 and conv.num_heads == 3


def test_constructor_refusals_and_defaults_without_a_gpu():
    with pytest.raises(ValueError, match="64, 128, 256"):
        GATModel(2, 2, 96, 16, 2, 64, "batch")
    with pytest.raises(ValueError, match="32, 64, 128"):
        GATModel(2, 2, 64, 16, 2, 48, "batch")
    with pytest.raises(ValueError, match="3 heads"):
        GAT_processor(2, 64, num_heads=2)
    with pytest.raises(ValueError, match="3 heads"):
        GATConv(64, 64, num_heads=2)
    m = GATModel(2, 2, 64, 16, 2, 64, "batch")
    assert m.kind == "gat" and m.directed is True and GATModel(2, 2, 64, 16, 2, 64, "layer", None, False).directed is False
    m.train()
    with pytest.raises(NotImplementedError, match="eval mode"):
        m((torch.tensor([0]), torch.tensor([1]), 2), torch.zeros(2, 2), torch.zeros(1, 2))
    with pytest.raises(NotImplementedError, match="GATModel"):
        m.gnn(None, None, None)
    assert GATModel(2, 2, 64, 16, 2, 64, "batch", dropout=None).gnn.convs[0].feat_drop.p == 0.0
    assert GATModel(2, 2, 64, 16, 2, 64, "batch", dropout=0.25).gnn.convs[1].feat_drop.p == 0.25


def test_folded_projection_weight_restates_el_and_er():
    """engine_gat.projection_weight (host only): rows 0..3H-1 are fc, row 3H + k is attn_l[k] fc_k, row 3H + 4 + k attn_r[k] fc_k, the rest
    zero - so h Wp^T carries feat, el and er of the unfolded statement (fp64 here: the fold is an identity, not an approximation)."""
    from gnnome_amd import engine_gat
    torch.manual_seed(1)
    H = 64
    conv = GATConv(H, H, num_heads=3)
    Wp = engine_gat.projection_weight(conv)
    assert Wp.shape == (3 * H + 64, H) and Wp.dtype == torch.float32
    assert torch.equal(Wp[:3 * H], conv.fc.weight.detach())
    used = [3 * H + k for k in (0, 1, 2, 4, 5, 6)]
    rest = [r for r in range(3 * H, 3 * H + 64) if r not in used]
    assert torch.count_nonzero(Wp[rest]) == 0 and all(torch.count_nonzero(Wp[r]) for r in used)
    h = torch.randn(9, H, dtype=torch.float64)
    feat = (h @ conv.fc.weight.detach().double().t()).view(9, 3, H)
    P = h @ Wp.double().t()
    el, er = (feat * conv.attn_l.detach().double()).sum(-1), (feat * conv.attn_r.detach().double()).sum(-1)
    tol = (h.abs() @ Wp.double().abs().t()) * 2.0 ** -24        # the one rounding of every folded weight to fp32
    assert ((P[:, 3 * H:3 * H + 3] - el).abs() <= tol[:, 3 * H:3 * H + 3]).all()
    assert ((P[:, 3 * H + 4:3 * H + 7] - er).abs() <= tol[:, 3 * H + 4:3 * H + 7]).all()
