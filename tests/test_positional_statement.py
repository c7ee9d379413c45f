"""tests/positional_statement.py - the dense restatement of utils/data_utils.py:59-90 - pinned on cases computed by hand, and the host
logic of gnnome_amd.positional on CPU tensors (no kernel runs here: what reaches the device is replaced by the statement)."""
import copy
import logging
import os

import pytest
import torch

import positional_statement as st
from gnnome_amd import features, positional, trainer


# ---- the statement on hand-computed cases ------------------------------------------------------------------------------------------

def test_rw_on_a_directed_triangle_returns_at_step_three():
    assert st.rw(*st.triangle(), 3).tolist() == [[0.0, 0.0, 1.0]] * 3


def test_rw_on_a_two_cycle_returns_at_even_steps():
    assert st.rw(*st.two_cycle(), 4).tolist() == [[0.0, 1.0, 0.0, 1.0]] * 2


def test_rw_self_loop_with_in_degree_two_is_one_half():
    pe = st.rw(*st.self_loop_in_degree_two(), 1)
    assert pe[0, 0].item() == 0.5 and pe[1, 0].item() == 0.0
    # two steps: the only closed walk through 0 is the loop twice, 1/2 * 1/2
    assert st.rw(*st.self_loop_in_degree_two(), 2)[0, 1].item() == 0.25


def test_rw_in_degree_zero_is_clipped_to_one():
    # node 0 of the single edge 0 -> 1 has in-degree 0: 1 / max(0, 1) keeps the matrix finite, and nothing returns anywhere
    pe = st.rw(*st.one_edge(), 3)
    assert torch.isfinite(pe).all() and pe.abs().sum().item() == 0.0


def test_rw_parallel_edge_on_a_two_cycle():
    # 0 -> 1 twice, 1 -> 0 once: indeg(1) = 2, indeg(0) = 1; the closed walk 0 -> 1 -> 0 exists twice, each 1/2 * 1
    pe = st.rw(*st.parallel_two_cycle(), 4)
    assert pe.tolist() == [[0.0, 1.0, 0.0, 1.0]] * 2


def test_pr_on_two_nodes_and_one_edge_by_hand():
    # n = 2, edge 0 -> 1: dinv = [1 / (1 + 1e-9), 0]; c = (1 - 0.95) / 2
    dinv0, c = 1.0 / (1.0 + 1e-9), (1.0 - 0.95) / 2
    x1 = [c, 0.95 * (0.5 * dinv0) + c]
    x2 = [c, 0.95 * (x1[0] * dinv0) + c]
    pe = st.pr(*st.one_edge(), 2)
    assert pe.shape == (2, 2)
    assert pe[:, 0].tolist() == pytest.approx(x1, rel=1e-15, abs=0)
    assert pe[:, 1].tolist() == pytest.approx(x2, rel=1e-15, abs=0)


def test_pr_single_node_is_the_teleport_term():
    pe = st.pr(*st.single_node(), 3)
    assert pe.tolist() == [[1.0 - 0.95] * 3]


def test_a_dag_gives_all_zeros():
    pe = st.rw(*st.dag(), 6)
    assert pe.shape == (5, 6) and (pe == 0).all()


def test_the_diagonal_is_the_same_under_both_adjacency_conventions():
    src, dst, n = st.four_nodes()
    a = st.rw(src, dst, n, 6, sources_on_rows=True)
    b = st.rw(src, dst, n, 6, sources_on_rows=False)
    assert (a > 0).any() and not torch.equal(st.adjacency(src, dst, n, True), st.adjacency(src, dst, n, False))
    torch.testing.assert_close(a, b, rtol=1e-14, atol=0)
    assert torch.equal(a == 0, b == 0)


def test_expansion_sizes_count_out_edges_of_the_row():
    # triangle: the row is always one node with one out-edge; the hub's row: itself, node 1 (fans out to 70), the 70 leaves, itself
    assert st.rw_expansion_sizes(*st.triangle(), 3) == [[1, 1, 1]] * 3
    assert st.rw_expansion_sizes(*st.hub_three_cycle(), 4)[0] == [1, 70, 70, 1]


def test_the_banded_graph_fits_the_default_capacity():
    from gnnome_amd import ops
    src, dst, n = st.banded()
    assert n == 400
    sizes = st.rw_expansion_sizes(src, dst, n, 8)
    assert 64 < max(max(r) for r in sizes) <= ops.RW_DEFAULT_CAPACITY
    pe = st.rw(src, dst, n, 8)
    assert (pe > 0).any() and (pe.sum(dim=1) == 0).any()      # some reads lie on short cycles, some on none


# ---- host logic --------------------------------------------------------------------------------------------------------------------

def _graph_dict(src, dst, n):
    return {"src": torch.tensor(src, dtype=torch.int32), "dst": torch.tensor(dst, dtype=torch.int32), "num_nodes": n,
            "y": torch.zeros(len(src))}


@pytest.fixture
def on_the_host(monkeypatch):
    """Replace what reaches the device: views are the edge list itself, degrees and encodings come from the statement."""
    calls = []

    def stored_degrees(graph, device=None):
        ind, outd = st.degrees(*graph)
        return ind.float(), outd.float()

    def encode(graph, pe_dim, pe_type, device, dtype, capacity):
        calls.append((pe_dim, pe_type, dtype, capacity))
        src, dst, n = graph
        return (st.rw if pe_type == "RW" else st.pr)(src, dst, n, pe_dim).to(dtype)

    monkeypatch.setattr(positional, "_views_on", lambda graph, device: graph)
    monkeypatch.setattr(features, "stored_degrees", stored_degrees)
    monkeypatch.setattr(positional, "_encode", encode)
    return calls


def test_pe_dim_zero_returns_none_without_touching_the_graph(on_the_host):
    assert positional.positional_encoding(object(), 0, "RW") is None
    assert positional.positional_encoding(object(), 0, "PR") is None
    assert positional.positional_encoding(object(), 0, "none") is None
    assert on_the_host == []
    with pytest.raises(ValueError):
        positional.positional_encoding(object(), -1, "RW")


def test_unknown_type_sets_nothing_and_is_logged_once(on_the_host, caplog):
    positional._warned.discard("LapPE")
    with caplog.at_level(logging.WARNING, logger="gnnome_amd.positional"):
        assert positional.positional_encoding(st.triangle(), 4, "LapPE") is None
        assert positional.positional_encoding(st.triangle(), 4, "LapPE") is None
    assert on_the_host == []
    assert len([r for r in caplog.records if "LapPE" in r.getMessage()]) == 1


def test_known_types_reach_the_encoder_with_the_defaults(on_the_host):
    pe = positional.positional_encoding(st.triangle(), 3, "RW")
    assert pe.dtype == torch.float32 and pe.tolist() == [[0.0, 0.0, 1.0]] * 3
    pe = positional.positional_encoding(st.one_edge(), 2, "PR", dtype=torch.float64, capacity=77)
    assert pe.dtype == torch.float64 and pe.shape == (2, 2)
    assert on_the_host == [(3, "RW", torch.float32, None), (2, "PR", torch.float64, 77)]


def test_add_positional_encoding_sets_exactly_the_reference_keys(on_the_host):
    base = _graph_dict(*st.four_nodes())
    before = set(base)
    g = positional.add_positional_encoding(base)                       # the defaults: nb_pos_enc = 0
    assert g is base and set(g) - before == {"in_deg", "out_deg"}
    assert g["in_deg"].dtype == g["out_deg"].dtype == torch.float32
    assert g["in_deg"].tolist() == [4.0, 1.0, 3.0, 0.0] and g["out_deg"].tolist() == [2.0, 2.0, 2.0, 2.0]
    g = positional.add_positional_encoding(_graph_dict(*st.four_nodes()), 5, "RW")
    assert set(g) - before == {"in_deg", "out_deg", "pe"} and g["pe"].shape == (4, 5) and g["pe"].dtype == torch.float32
    assert torch.equal(g["pe"], st.rw(*st.four_nodes(), 5).float())
    g = positional.add_positional_encoding(_graph_dict(*st.four_nodes()), 2, "PR")
    assert torch.equal(g["pe"], st.pr(*st.four_nodes(), 2).float())
    g = positional.add_positional_encoding(_graph_dict(*st.four_nodes()), 5, "none")     # the reference's default type with a width
    assert set(g) - before == {"in_deg", "out_deg"}


def test_hyperparameters_carry_the_reference_switches_off():
    hp = trainer.hyperparameters_with()
    assert hp["nb_pos_enc"] == 0 and hp["type_pos_enc"] == "none"
    assert trainer.hyperparameters_with({"nb_pos_enc": 8, "type_pos_enc": "PR"})["nb_pos_enc"] == 8


def test_load_dataset_with_the_defaults_leaves_the_graphs_as_they_were(tmp_path, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("nothing is computed at nb_pos_enc = 0")

    monkeypatch.setattr(positional, "add_positional_encoding", refuse)
    graphs = [_graph_dict(*st.triangle()), _graph_dict(*st.four_nodes())]
    want = copy.deepcopy(graphs)
    for loaded in (trainer.load_dataset(graphs), trainer.load_dataset(graphs, trainer.hyperparameters_with()),
                   trainer.load_dataset(graphs, {"lr": 1e-3}, torch.device("cpu"))):
        assert [n for n, _ in loaded] == ["graph 0", "graph 1"]
        for (_, g), orig, w in zip(loaded, graphs, want):
            assert g is orig and set(g) == set(w)
            assert all(torch.equal(g[k], w[k]) if torch.is_tensor(w[k]) else g[k] == w[k] for k in w)
    for idx, g in enumerate(graphs):
        torch.save(g, os.path.join(tmp_path, f"{idx}.pt"))
    from_disk = trainer.load_dataset(str(tmp_path))
    assert [set(g) for _, g in from_disk] == [set(w) for w in want]


def test_load_dataset_hands_the_switches_to_add_positional_encoding(monkeypatch):
    seen = []

    def record(g, nb_pos_enc=0, type_pos_enc="none", device=None):
        seen.append((g["num_nodes"], nb_pos_enc, type_pos_enc, device))
        g["pe"] = "set"
        return g

    monkeypatch.setattr(positional, "add_positional_encoding", record)
    loaded = trainer.load_dataset([_graph_dict(*st.triangle())], {"nb_pos_enc": 4, "type_pos_enc": "RW"}, "dev")
    assert seen == [(3, 4, "RW", "dev")] and loaded[0][1]["pe"] == "set"
