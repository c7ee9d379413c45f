"""GatedGCNModel (models/full_graph.py:33-53) on the MI355X: the reference's own logits (tests/golden/g16_gated_h64.pt, written by
tests/golden/make_golden_gated.py), a plain-torch restatement at the wider built widths, and bit-equality with a SymGatedGCNModel that
carries the same parameters and a zero A_3."""
import pytest
import torch

import gnnome_amd
from gnnome_amd import layers, ops
from gnnome_amd.models import GatedGCNModel, SymGatedGCNModel

import gated_graphs as gg
from conftest import load_golden

pytestmark = pytest.mark.gpu

BAR = 1e-4          # the project's golden bar on edge probabilities (tests/test_hip_parity.py)


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("g16_gated_h64.pt")


def _prob_diff(got, want):
    return (torch.sigmoid(got.detach().cpu()) - torch.sigmoid(want)).abs().max().item()


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("norm", ("batch", "layer"))
def test_reference_state_dict_loads_and_reproduces_the_reference_logits(golden, norm, directed):
    g, case = golden, golden["cases"][norm]
    m = GatedGCNModel(2, 2, g["hidden"], g["hidden_ne"], g["layers"], g["hs"], norm, directed=directed)
    m.load_state_dict(case["state_dict"], strict=True)
    m.eval()
    got = m((g["src"], g["dst"], g["num_nodes"]), g["x"], g["e"])          # CPU inputs: staged to the device, logits come back
    want = case["logits_directed" if directed else "logits_undirected"]
    assert got.shape == want.shape == (g["src"].numel(), 1) and got.device.type == "cpu"
    diff = _prob_diff(got, want)
    print(f"{norm} directed={directed}: max |dp| = {diff:.2e}")
    assert diff < BAR


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("norm", ("batch", "layer"))
@pytest.mark.parametrize("hidden,hs", ((128, 32), (256, 128)))
def test_wider_models_match_a_plain_torch_restatement(hidden, hs, norm, directed):
    n, e_cnt, nl = 40, 200, 2
    src, dst, x, e = gg.model_graph(n, e_cnt, seed=hidden)
    m = GatedGCNModel(2, 2, hidden, 16, nl, hs, norm, directed=directed)
    sd = gg.random_gated_state_dict(m, seed=hidden + hs)
    m.load_state_dict(sd)
    m.to(dev()).eval()
    got = m((src, dst, n), x.to(dev()), e.to(dev()))
    with torch.no_grad():
        want = gg.gated_model(sd, src, dst, n, x, e, nl, directed=directed)
    diff = _prob_diff(got, want)
    print(f"H={hidden} hs={hs} {norm} directed={directed}: max |dp| = {diff:.2e}")
    assert got.is_cuda and diff < BAR


def _sym_twin(m, hidden, hs, nl, norm):
    """A SymGatedGCNModel with m's parameters and buffers and A_3 = 0."""
    sym = SymGatedGCNModel(2, 2, hidden, 16, nl, hs, norm)
    sd = {}
    for k, v in m.state_dict().items():
        k = k.replace("node_encoder.linear1", "linear1_node").replace("node_encoder.linear2", "linear2_node")
        k = k.replace("edge_encoder.linear1", "linear1_edge").replace("edge_encoder.linear2", "linear2_edge")
        sd[k] = v.clone()
    for i in range(nl):
        sd[f"gnn.convs.{i}.A_3.weight"] = torch.zeros(hidden, hidden)
        sd[f"gnn.convs.{i}.A_3.bias"] = torch.zeros(hidden)
    sym.load_state_dict(sd, strict=True)
    return sym


@pytest.mark.parametrize("norm", ("batch", "layer"))
@pytest.mark.parametrize("hidden", (64, 128, 256))
def test_bit_equal_to_the_symmetric_model_with_a_zero_a3(hidden, norm):
    """Eval mode, a graph without hubs: the [N,4H] projection, the shared gate and the in-edge aggregation leave the bits the symmetric
    model's kernels leave when its A_3 is zero."""
    n, e_cnt, nl, hs = 300, 2400, 3, 64
    src, dst, x, e = gg.model_graph(n, e_cnt, seed=7)
    m = GatedGCNModel(2, 2, hidden, 16, nl, hs, norm)
    m.load_state_dict(gg.random_gated_state_dict(m, seed=hidden))
    sym = _sym_twin(m, hidden, hs, nl, norm).to(dev()).eval()
    m.to(dev()).eval()
    views = gnnome_amd.graph.views_for((src, dst, n), dev())
    got, want = m(views, x.to(dev()), e.to(dev())), sym(views, x.to(dev()), e.to(dev()))
    assert torch.isfinite(got).all() and torch.equal(got, want)
    # ... and on the views of dgl.reverse(g), which this model rebuilds over the swapped edge list
    got_r, want_r = m(views.reversed(), x.to(dev()), e.to(dev())), sym(views.reversed(), x.to(dev()), e.to(dev()))
    assert _prob_diff(got_r, want_r.cpu()) < BAR


@pytest.mark.parametrize("norm", ("batch", "layer"))
def test_layer_level_forward_takes_and_returns_edge_id_order(norm):
    hidden, n, e_cnt = 64, 40, 200
    src, dst, _, _ = gg.model_graph(n, e_cnt, seed=2)
    conv = layers.GatedGCN(hidden, hidden, norm)
    sd = gg.random_gated_state_dict(conv, seed=4)
    conv.load_state_dict(sd)
    conv.eval()
    g = torch.Generator().manual_seed(1)
    h, e = torch.randn(n, hidden, generator=g), torch.randn(e_cnt, hidden, generator=g)
    with torch.no_grad():
        h_got, e_got = conv((src, dst, n), h, e)
        h_want, e_want = gg.gated_layer(sd, "", src.long(), dst.long(), n, h, e)
    assert (e_got - e_want).abs().max().item() < 1e-4 and (h_got - h_want).abs().max().item() < 1e-4
    # edge-id order: a permuted edge list gives the same rows, permuted the same way
    perm = torch.randperm(e_cnt, generator=g)
    with torch.no_grad():
        h_p, e_p = conv((src[perm], dst[perm], n), h, e[perm])
    assert (e_p - e_want[perm]).abs().max().item() < 1e-4 and (h_p - h_want).abs().max().item() < 1e-4


def test_doubled_views_on_the_device_are_built_once_and_hold_the_doubled_list():
    from gnnome_amd import engine_gated
    n, E = 40, 200
    src, dst, _, _ = gg.model_graph(n, E, seed=4)
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    dbl = engine_gated.doubled_for(views)
    assert engine_gated.doubled_for(views) is dbl and dbl.views.num_edges == 2 * E
    s2, d2 = engine_gated.edge_list_of(dbl.views)
    assert torch.equal(s2[:E].cpu(), src) and torch.equal(d2[:E].cpu(), dst)          # ids < E: the originals
    assert torch.equal(s2[E:].cpu(), dst) and torch.equal(d2[E:].cpu(), src)          # id E + k: the reverse copy of edge k
    assert torch.equal(dbl.enc_gather.long(), dbl.views.srt_eid.long() % E)
    assert torch.equal(dbl.views.srt_eid[dbl.score_gather.long()], views.srt_eid)     # exactly the ids < E, in the original sorted order
    rev = engine_gated.in_edge_views(views.reversed())                                # true views of the reversed graph, kept with the views
    assert engine_gated.in_edge_views(views.reversed()) is rev and not rev.transposed
    rs, rd = engine_gated.edge_list_of(rev)
    assert torch.equal(rs.cpu(), dst) and torch.equal(rd.cpu(), src)


def test_torch_operator_equals_the_ctypes_front_end():
    import gnnome_amd.torch_ops  # noqa: F401
    hidden = 128
    gr = gg.degree_graph(hidden)
    views = ops.GraphViews(gr["src"].to(dev()), gr["dst"].to(dev()), gr["n"])
    g = torch.Generator().manual_seed(3)
    P = torch.randn(gr["n"], 4 * hidden, generator=g).to(dev())
    e, h = torch.randn(views.num_edges, hidden, generator=g).to(dev()), torch.randn(gr["n"], hidden, generator=g).to(dev())
    scale, shift = torch.rand(hidden, generator=g).to(dev()) + 0.5, torch.randn(hidden, generator=g).to(dev())
    A1, A2 = P[:, :hidden], P[:, hidden:2 * hidden]
    for norm in (0, 1):
        got = torch.ops.gnnome_hip.node_aggregate_in(e, A1, A2, views.in_ptr, views.srt_src, h, scale, shift, norm)
        assert torch.equal(got, ops.node_aggregate_in(e, A1, A2, views, h, norm, scale, shift))
    meta = torch.ops.gnnome_hip.node_aggregate_in(*(t.to("meta") for t in (e, A1, A2, views.in_ptr, views.srt_src, h, scale, shift)), 0)
    assert meta.shape == h.shape and meta.device.type == "meta"


def test_refusals_on_the_device_path():
    with pytest.raises(ValueError, match="64, 128, 256"):
        GatedGCNModel(2, 2, 96, 16, 2, 64, "batch")
    m = GatedGCNModel(2, 2, 64, 16, 1, 64, "batch").eval()
    m.arithmetic = "reference"
    src, dst, x, e = gg.model_graph(10, 30, seed=1)
    with pytest.raises(ValueError, match="reference"):
        m((src, dst, 10), x, e)
