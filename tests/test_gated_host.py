"""The host side of GatedGCNModel: names, refusals, the doubled edge list of directed=False and the C ABI of the new entries.
Runs without a GPU."""
import ctypes
import re

import pytest
import torch

from gnnome_amd import _lib, engine_gated, layers
from gnnome_amd.models import GatedGCNModel

import gated_graphs as gg
import header_binding
from conftest import load_golden

# (gnnome_node_aggregate_in_raw_f32 is not built: the training route goes through the symmetric step and does not need it)
NEW_ENTRIES = ("gnnome_node_aggregate_in_f32", "gnnome_node_aggregate_in_range_f32")


@pytest.mark.parametrize("norm", ("batch", "layer"))
def test_state_dict_keys_equal_the_reference_key_list(norm):
    g = load_golden("g16_gated_h64.pt")
    m = GatedGCNModel(2, 2, g["hidden"], g["hidden_ne"], g["layers"], g["hs"], norm)
    assert list(m.state_dict()) == g["cases"][norm]["keys"]
    assert not any("A_3" in k for k in m.state_dict())
    m.load_state_dict(g["cases"][norm]["state_dict"], strict=True)
    prefixes = {k.split(".")[0] for k in m.state_dict()}
    assert prefixes == {"node_encoder", "edge_encoder", "gnn", "predictor"}


def test_constructor_refusals():
    with pytest.raises(ValueError, match=r"\(64, 128, 256\)"):
        GatedGCNModel(2, 2, 100, 16, 2, 64, "batch")
    with pytest.raises(ValueError, match=r"\(32, 64, 128\)"):
        GatedGCNModel(2, 2, 64, 16, 2, 48, "batch")
    with pytest.raises(ValueError, match="in_channels == out_channels"):
        layers.GatedGCN(64, 128, "batch")
    with pytest.raises(ValueError, match="residual"):
        layers.GatedGCN(64, 64, "batch", residual=False)
    with pytest.raises(ValueError, match="normalization"):
        layers.GatedGCN(64, 64, "none")
    with pytest.raises(ValueError):
        layers.NodeEncoder(2, 16, 64, bias=False)
    conv = layers.GatedGCN(64, 64, "layer", dropout=0.25)
    assert conv.dropout == 0.25 and not hasattr(conv, "A_3") and isinstance(conv.bn_e, torch.nn.LayerNorm)
    assert GatedGCNModel(2, 2, 64, 16, 2, 64, "batch").directed is True
    m = GatedGCNModel(2, 2, 64, 16, 1, 64, "batch")
    m.arithmetic = "reference"
    with pytest.raises(ValueError, match="reference"):
        engine_gated.check_arithmetic(m)


def test_doubled_edge_list_ids_and_row_maps():
    """engine_gated.doubled_edge_list / doubled_row_maps - what engine_gated.Doubled builds the directed=False graph from: edge E + k is the
    reverse copy of edge k, e is fed twice through enc_gather, and score_gather picks exactly the rows of the first E ids (e[:E], the
    originals) in the original views' sorted order."""
    src = torch.tensor([0, 2, 1, 2, 3], dtype=torch.int32)
    dst = torch.tensor([1, 1, 3, 0, 3], dtype=torch.int32)
    E = src.numel()
    s2, d2 = engine_gated.doubled_edge_list(src, dst)
    assert s2.tolist() == [0, 2, 1, 2, 3, 1, 1, 3, 0, 3] and d2.tolist() == [1, 1, 3, 0, 3, 0, 2, 1, 2, 3]
    assert torch.equal(s2[:E], src) and torch.equal(d2[:E], dst)          # ids < E are the originals
    assert torch.equal(s2[E:], dst) and torch.equal(d2[E:], src)          # id E + k is the reverse copy of edge k
    assert all(torch.equal(a, b) for a, b in zip((s2, d2), gg.doubled_edge_list(src, dst)))   # (the restatement's own doubling)
    # hand-made sorted orders (stable sort by destination): the original views' and the doubled views'
    srt_eid = torch.tensor([3, 0, 1, 2, 4], dtype=torch.int32)                                  # dst 0 | 1 1 | 3 3
    srt_eid2 = torch.tensor([3, 5, 0, 1, 7, 6, 8, 2, 4, 9], dtype=torch.int32)                  # dst 0 0 | 1 1 1 | 2 2 | 3 3 3
    assert torch.equal(torch.argsort(dst.long(), stable=True).int(), srt_eid) and torch.equal(torch.argsort(d2.long(), stable=True).int(), srt_eid2)
    enc_gather, score_gather = engine_gated.doubled_row_maps(srt_eid2, srt_eid, E)
    assert enc_gather.dtype == score_gather.dtype == torch.int32
    assert enc_gather.tolist() == [3, 0, 0, 1, 2, 1, 3, 2, 4, 4]          # every original row twice: once as itself, once as its reverse copy
    assert score_gather.tolist() == [0, 2, 3, 7, 8]
    assert torch.equal(srt_eid2[score_gather.long()], srt_eid)            # exactly the ids < E, in the original sorted order
    # rows of a per-edge tensor: fed twice, and back out as the originals
    feats = torch.arange(E, dtype=torch.float32).unsqueeze(1) * 10.0
    doubled_rows = feats[enc_gather.long()]                                # what the edge encoder's gather hands the stack
    assert torch.equal(doubled_rows, torch.cat([feats, feats])[srt_eid2.long()])
    assert torch.equal(doubled_rows[score_gather.long()], feats[srt_eid.long()])
    # any order of the doubled views serves: the maps follow the ids, not the positions
    g = torch.Generator().manual_seed(0)
    src_r, dst_r, _, _ = gg.model_graph(12, 30, seed=3)
    s2r, d2r = engine_gated.doubled_edge_list(src_r, dst_r)
    o1, o2 = torch.argsort(dst_r.long(), stable=True).int(), torch.randperm(60, generator=g).int()
    enc, sc = engine_gated.doubled_row_maps(o2, o1, 30)
    assert torch.equal(o2[sc.long()], o1) and torch.equal(enc.long(), o2.long() % 30)
    assert torch.equal(s2r[o2.long()][sc.long()], src_r[o1.long()]) and torch.equal(d2r[o2.long()][sc.long()], dst_r[o1.long()])


def test_training_adapter_shares_the_parameters_and_has_a_zero_a3():
    m = GatedGCNModel(2, 2, 64, 16, 2, 64, "batch", dropout=0.1)
    ad = engine_gated.SymAdapter(m)
    assert ad.linear1_node is m.node_encoder.linear1 and ad.linear2_edge is m.edge_encoder.linear2 and ad.predictor is m.predictor
    assert len(ad.names) == len(list(m.parameters())) and ad.names[0] == "linear1_node.weight" and "linear2_edge.bias" in ad.names
    assert not any("A_3" in n for n in ad.names)
    for conv, layer in zip(m.gnn.convs, ad.gnn.convs):
        assert layer.A_1 is conv.A_1 and layer.bn_e is conv.bn_e and layer.dropout == 0.1 and layer.bn_e_updates == 1
        assert not isinstance(layer.A_3.weight, torch.nn.Parameter) and not layer.A_3.weight.requires_grad
        assert not bool(layer.A_3.weight.any()) and not bool(layer.A_3.bias.any())


def test_header_and_ctypes_table_agree_on_the_new_entries():
    header = open(_lib.HEADER_PATH).read()
    parsed = header_binding.parse_header(_lib.HEADER_PATH)
    kind = lambda t: "ptr" if t in (ctypes.c_void_p,) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)) else t  # noqa: E731
    lib = header_binding.bind(_lib.LIB_PATH, _lib.HEADER_PATH)
    for name in NEW_ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert [kind(t) for t in parsed[name][1]] == [kind(t) for t in _lib.SIGNATURES[name]], name
        assert hasattr(lib, name)
    assert "gated_gcn_full.py:212-225" in header
    # argument validation runs before anything touches the device
    one = ctypes.c_void_p(16)
    assert lib.gnnome_node_aggregate_in_f32(None, 64, 0, None, None, 256, None, None, None, 64, None, 0, None, None, None) == 0   # no nodes: a no-op
    assert lib.gnnome_node_aggregate_in_f32(one, 96, 5, one, one, 96, one, one, one, 96, ctypes.c_void_p(32), 0, one, one, None) == -1
    assert b"hidden=96" in lib.gnnome_last_error()
    assert lib.gnnome_node_aggregate_in_f32(one, 64, 5, None, one, 256, one, one, one, 64, ctypes.c_void_p(32), 0, one, one, None) == -1
    assert b"null" in lib.gnnome_last_error()
    assert lib.gnnome_node_aggregate_in_range_f32(one, 64, 5, 3, 2, one, one, 256, one, one, one, 64, ctypes.c_void_p(32), 0, one, one, None) == -1
    assert b"range" in lib.gnnome_last_error()
    assert lib.gnnome_node_aggregate_in_f32(one, 64, 5, one, one, 256, one, one, one, 64, ctypes.c_void_p(32), 7, one, one, None) == -1
    assert b"norm_kind" in lib.gnnome_last_error()
