"""CPU tests of tests/aggregate_graphs.py: the graphs have the degrees they claim and reach the places they are for, and the exact input
recipe is what its name says - integer sums below 2^24, the same fp32 bits whatever the order of the additions."""
import pytest
import torch

import aggregate_graphs as ag
import cpu_ops


def _degrees(g):
    n = g["n"]
    return torch.bincount(g["dst"].long(), minlength=n), torch.bincount(g["src"].long(), minlength=n)


@pytest.mark.parametrize("name", list(ag.FAMILIES))
def test_family_has_the_degrees_it_claims(name):
    g = ag.graph(name)
    din, dout = _degrees(g)
    assert torch.equal(din, g["in_degree"]) and torch.equal(dout, g["out_degree"])
    for node, (a, b) in g["spec"].items():
        assert (int(din[node]), int(dout[node])) == (a, b), node
    assert g["hubs"] == torch.nonzero(din + dout > ag.HUB_THRESHOLD).flatten().tolist()
    assert int(g["src"].min()) >= 0 and int(g["dst"].min()) >= 0 and max(int(g["src"].max()), int(g["dst"].max())) < g["n"]
    # the probes: one in-edge each, from a node that has no other edge
    assert sorted(g["dst"][g["src"] == g["probe_src"]].tolist()) == sorted([g["probe_on"], g["probe_off"]])
    assert (int(din[g["probe_src"]]), int(dout[g["probe_on"]]), int(dout[g["probe_off"]])) == (0, 0, 0)


def test_lists_family_covers_every_pair_of_lengths_and_the_special_nodes():
    g = ag.graph("lists")
    n = g["n"]
    pairs = sorted(g["spec"].values())
    for a in ag.LIST_LENGTHS:
        for b in ag.LIST_LENGTHS:
            assert (a, b) in pairs
    assert g["spec"][0] == (0, 0) and g["spec"][n - 1] == (0, 0) and not g["hubs"]
    edges = list(zip(g["src"].tolist(), g["dst"].tolist()))
    loops = {}
    for s, d in edges:
        if s == d:
            loops[s] = loops.get(s, 0) + 1
    assert sorted(loops.values()) == [1, 1, 2]
    count = {}
    for sd in edges:
        count[sd] = count.get(sd, 0) + 1
    assert sum(1 for sd, c in count.items() if c == 3 and sd[0] != sd[1]) == 1
    # the pool the neighbours come from stays low-degree
    special = torch.zeros(n, dtype=torch.bool)
    special[list(g["spec"])] = True
    assert int((g["in_degree"] + g["out_degree"])[~special].max()) < 64


def test_hub_edges_family_sits_on_the_threshold_and_the_range_ends():
    g = ag.graph("hub_edges")
    n, items = g["n"], g["in_degree"] + g["out_degree"]
    by_spec = {v: k for k, v in g["spec"].items()}
    assert by_spec[(2048, 2047)] not in g["hubs"] and by_spec[(2048, 2048)] not in g["hubs"] and by_spec[(2049, 2048)] in g["hubs"]
    assert int(items[by_spec[(2048, 2048)]]) == ag.HUB_THRESHOLD and int(items[by_spec[(2049, 2048)]]) == ag.HUB_THRESHOLD + 1
    assert by_spec[(4097, 0)] == 0 and by_spec[(0, 4097)] == n - 1 and 0 in g["hubs"] and n - 1 in g["hubs"]
    assert len(g["hubs"]) == 7 and g["src"].numel() < 60_000
    # (4130, 37): chunks of one 64-item batch, the in / out boundary inside one, empty chunks behind
    cnt = 4130 + 37
    per = ((cnt + ag.HUB_CHUNKS - 1) // ag.HUB_CHUNKS + ag.BATCH - 1) // ag.BATCH * ag.BATCH
    assert per == ag.BATCH and 4130 % ag.BATCH != 0 and -(-cnt // per) < ag.HUB_CHUNKS
    loop_hub = by_spec[(2150, 2150)]
    assert sum(1 for s, d in zip(g["src"].tolist(), g["dst"].tolist()) if s == d == loop_hub) == 50
    non_hub = torch.ones(n, dtype=torch.bool)
    non_hub[list(g["spec"])] = False
    assert int(items[non_hub].max()) < 64


@pytest.mark.parametrize("k", ag.MANY_HUBS)
def test_many_hubs_family(k):
    g = ag.graph(f"many_hubs{k}")
    items = g["in_degree"] + g["out_degree"]
    hubs = g["hubs"]
    assert len(hubs) == k and hubs == [5 + ag.MANY_HUBS_STRIDE * j for j in range(k)]
    assert all(ag.HUB_THRESHOLD + 4 <= int(items[h]) <= 4400 for h in hubs)
    assert hubs[-1] > g["n"] - 2 * ag.MANY_HUBS_STRIDE and g["src"].numel() <= 310_000      # spread over the whole range
    is_hub = torch.zeros(g["n"], dtype=torch.bool)
    is_hub[hubs] = True
    s_hub, d_hub = is_hub[g["src"].long()], is_hub[g["dst"].long()]
    probe = g["src"] == g["probe_src"]
    assert bool(((s_hub ^ d_hub) | probe).all())                                            # every hub edge joins a hub to a non-hub node
    # written in shuffled order: the first edge of each hub, in edge order, is neither ascending nor descending in id
    hub_end = torch.where(s_hub, g["src"], g["dst"]).long()[s_hub | d_hub]      # the hub of every hub edge, in edge order
    first = {h: int(torch.nonzero(hub_end == h)[0]) for h in hubs}
    order = sorted(first, key=first.get)
    assert order != sorted(order) and order != sorted(order, reverse=True)


@pytest.mark.parametrize("name", list(ag.FAMILIES))
def test_exact_recipe_is_order_independent_in_fp32(name):
    g = ag.graph(name)
    n, hidden = g["n"], 64
    cv = cpu_ops.CpuViews(g["src"], g["dst"], n)
    s, d = cv.srt_src, cv.srt_dst
    gates, A2, A3, X = ag.exact_inputs(s.numel(), n, hidden, seed=5)
    assert set(gates.unique().tolist()) == {ag.GATE_ON, ag.GATE_OFF}
    assert float(torch.sigmoid(torch.tensor(ag.GATE_ON))) == 1.0 and float(torch.sigmoid(torch.tensor(ag.GATE_OFF))) == 0.0
    want = ag.exact_sums(s, d, gates, A2, A3, n)
    as_f32 = ag.exact_sums(s, d, gates, A2, A3, n, dtype=torch.float32)
    perm = torch.randperm(s.numel(), generator=torch.Generator().manual_seed(1))
    shuffled = ag.exact_sums(s[perm], d[perm], gates[perm], A2, A3, n, dtype=torch.float32)
    for key, w in want.items():
        assert torch.equal(as_f32[key], w.float()) and torch.equal(shuffled[key], w.float()), key
    # no sum - nor any partial sum of it, in any order - reaches 2^24: the sums of the absolute values stay below it
    bound = ag.exact_sums(s, d, gates, A2.abs(), A3.abs(), n)
    assert max(int(v.max()) for v in bound.values()) < ag.EXACT_LIMIT
    want_seg = ag.exact_segment_sums(s, d, X, n)
    seg_f32 = ag.exact_segment_sums(s, d, X, n, dtype=torch.float32)
    assert all(torch.equal(a, b.float()) for a, b in zip(seg_f32, want_seg))
    assert max(int(v.max()) for v in ag.exact_segment_sums(s, d, X.abs(), n)) < ag.EXACT_LIMIT
    # ... and the checker's own float32 statement of mode 2 (sigmoid and all) gives the same integers
    chk_in, chk_out = cpu_ops.node_aggregate_raw(gates, None, A2, A3, cv, 2, n)
    assert torch.equal(chk_in, want["sum_in"].float()) and torch.equal(chk_out, want["sum_out"].float())
