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


# ---------------------------------------------------------------------------------------------- the halves recipe

BACKWARD_GRAPHS = ("lists", "hub_edges")          # what tests/test_aggregate_adversarial.py runs the halves recipe on, at these widths
BACKWARD_WIDTHS = (64, 128, 256)
_SORTED = {}


def _sorted(name):
    """(s, d, n) of the named graph: the destination-sorted endpoint arrays, built once."""
    if name not in _SORTED:
        g = ag.graph(name)
        cv = cpu_ops.CpuViews(g["src"], g["dst"], g["n"])
        _SORTED[name] = (cv.srt_src.long(), cv.srt_dst.long(), g["n"], cv)
    return _SORTED[name]


def _assert_halves_condition(s, d, t, n, what):
    bound = ag.exact_backward_bound(s, d, t, n)
    assert max(bound.values()) < ag.EXACT_LIMIT, (what, bound)
    return bound


@pytest.mark.parametrize("hidden", BACKWARD_WIDTHS)
@pytest.mark.parametrize("name", BACKWARD_GRAPHS)
def test_halves_recipe_stays_below_2_to_24_quarters(name, hidden):
    """The CONDITION of the recipe, on the graphs and widths the device tests use, in both roles of the endpoint arrays (reversed views) -
    renumbering the nodes permutes the sums and changes none: per output the sum of the absolute values of the terms, in quarters, is
    below 2^24, so every partial sum is an fp32 value."""
    s, d, n, _ = _sorted(name)
    t = ag.exact_backward_inputs(s.numel(), n, hidden, seed=hidden + len(name))
    kinds = {v: int((t["gates"] == v).sum()) for v in (ag.GATE_ON, ag.GATE_OFF, ag.GATE_HALF)}
    assert sum(kinds.values()) == t["gates"].numel() and 0.45 < kinds[ag.GATE_HALF] / t["gates"].numel() < 0.55
    assert bool(((t["gates"] == ag.GATE_HALF).any(1) & (t["gates"] != ag.GATE_HALF).any(1)).all())         # mixed within every row
    for k in ag.NODE_TABLES + ("de0", "xe", "mean"):
        assert torch.equal(t[k], t[k].round()) and float(t[k].abs().max()) <= ag.BACKWARD_MAX, k
    assert torch.equal(t["xe"].to(torch.bfloat16).float(), t["xe"])                                         # xe is its own bf16 copy
    assert set(t["scale"].tolist()) <= {1.0, 2.0} and bool(((2 * t["shift"]) % 2 == 1).all())
    act = t["xe"] * t["scale"] + t["shift"]
    assert bool((act != 0).all()) and torch.equal(act.double(), t["xe"].double() * t["scale"].double() + t["shift"].double())
    for ss, dd in ((s, d), (d, s)):
        bound = _assert_halves_condition(ss, dd, t, n, name)
        print(f"{name} H={hidden}: sums of |terms| in quarters {bound} (limit {ag.EXACT_LIMIT})")


@pytest.mark.parametrize("n,e,last", ag.TAILS)
def test_tails_graphs_sit_on_the_clamp(n, e, last):
    g = ag.tails(n, e, last)
    cv = cpu_ops.CpuViews(g["src"], g["dst"], n)
    active = g["active"]
    assert n % 4 != 0 and g["src"].numel() == e
    assert (n == 1 or active < n) and not bool((g["in_degree"] + g["out_degree"])[active:].any())          # the highest nodes: no edge at all
    assert bool((cv.in_ptr[active:] == e).all()) and bool((cv.out_ptr[active:].long() >= int(cv.out_ptr[active])).all())
    assert int(cv.in_ptr[active]) == e and int(cv.in_ptr[active]) - int(cv.in_ptr[active - 1]) == last     # ... and the last in-list ends at position E - 1
    for hidden in BACKWARD_WIDTHS:
        t = ag.exact_backward_inputs(e, n, hidden, seed=n + e)
        _assert_halves_condition(cv.srt_src.long(), cv.srt_dst.long(), t, n, (n, e))


def test_halves_statement_is_the_checkers_and_order_independent_in_fp32():
    """The int64 statement against the checker's torch restatement of the fused backward (sigmoid and all) in float32, and over shuffled
    edges: the same numbers, bit for bit."""
    s, d, n, cv = _sorted("lists")
    t = ag.exact_backward_inputs(s.numel(), n, 64, seed=2)
    want = ag.exact_backward(s, d, t, n)
    assert float(torch.sigmoid(torch.tensor(ag.GATE_HALF))) == 0.5
    for dtype in (torch.float32,):      # (in float64 sigmoid(GATE_OFF) = 2.6e-56 is not zero: the checker's own statement is exact in float32 only)
        c = {k: v.to(dtype) for k, v in t.items()}
        got = cpu_ops.agg_bwd_fused(c["gates"], c["Tf"], c["Uf"], c["Tb"], c["Ub"], c["A2"], c["A3"], cv, c["de0"].clone(), c["xe"], c["scale"],
                                    c["shift"], c["mean"], n)
        for key, g_ in zip(("sum_in", "sum_out", "de", "s1", "s2"), got):
            assert torch.equal(g_.double(), want[key]), (dtype, key)
    perm = torch.randperm(s.numel(), generator=torch.Generator().manual_seed(1))
    tp = dict(t, gates=t["gates"][perm], de0=t["de0"][perm], xe=t["xe"][perm])
    shuffled = ag.exact_backward(s[perm], d[perm], tp, n)
    assert all(torch.equal(shuffled[k], want[k]) for k in ("sum_in", "sum_out", "s1", "s2")) and torch.equal(shuffled["de"], want["de"][perm])


def _without(t, p):
    keep = torch.ones(t["gates"].shape[0], dtype=torch.bool)
    keep[p] = False
    return dict(t, gates=t["gates"][keep], de0=t["de0"][keep], xe=t["xe"][keep]), keep


def _mutants(s, d, t, n, want, p):
    """What a kernel with one of the faults the device tests are for would return, restated on the statement at sorted position p
    -> {name: outputs}; `de` always has the E rows of the unmutated statement."""
    out = {}
    tw, keep = _without(t, p)
    m = ag.exact_backward(s[keep], d[keep], tw, n)
    out["one list item dropped"] = dict(want, sum_in=m["sum_in"], sum_out=m["sum_out"])            # (the node sums walk lists, de' and s1 / s2 rows)
    idx = torch.cat([torch.arange(s.numel()), torch.tensor([p])])
    m2 = ag.exact_backward(s[idx], d[idx], dict(t, gates=t["gates"][idx], de0=t["de0"][idx], xe=t["xe"][idx]), n)
    out["one item doubled"] = dict(want, sum_in=m2["sum_in"], sum_out=m2["sum_out"])
    # the neighbour of item p replaced by the first item's of its 64-item batch of d[p]'s in-list
    first = int(torch.searchsorted(d, d[p]))
    head = first + (p - first) // ag.BATCH * ag.BATCH
    s_first = s.clone()
    s_first[p] = s[head]
    mf = ag.exact_backward(s_first, d, t, n)
    out["neighbour of the batch's first item"] = dict(mf, sum_out=want["sum_out"])                  # (the in-edge walk's neighbour: sum_in, de', s1, s2)
    de = want["de"].clone()
    de[p] = t["de0"][p].double()
    out["one de row left unwritten"] = dict(want, de=de)
    out["one row dropped from the statistics"] = dict(want, s1=m["s1"], s2=m["s2"])
    return out


def test_every_mutant_changes_an_output_of_the_halves_statement():
    """A lost, doubled or misrouted item, an unwritten de' row and a row missing from the statistics each change at least one of the five
    outputs on the `lists` graph - at EVERY sampled position: the recipe has no blind rows.  (The only positions left out of the
    misrouted-neighbour mutation are the ones where it changes nothing by construction: the first item of a batch, and a parallel edge of it.)"""
    s, d, n, _ = _sorted("lists")
    hidden = 64
    t = ag.exact_backward_inputs(s.numel(), n, hidden, seed=hidden + len("lists"))
    want = ag.exact_backward(s, d, t, n)
    e = s.numel()
    rng = torch.Generator().manual_seed(4)
    positions = sorted({0, e - 1, *torch.randint(0, e, (24,), generator=rng).tolist()})
    table, misrouted = {}, 0
    for p in positions:
        for name, got in _mutants(s, d, t, n, want, p).items():
            changed = [k for k in want if not torch.equal(got[k], want[k])]
            if name.startswith("neighbour"):
                first = int(torch.searchsorted(d, d[p]))
                if int(s[first + (p - first) // ag.BATCH * ag.BATCH]) == int(s[p]):
                    assert not changed
                    continue
                misrouted += 1
            table.setdefault(name, set()).update(changed)
            assert changed, (name, p)
    assert misrouted >= 10 and len(table) == 5
    print()
    for name, changed in table.items():
        print(f"{name:40s} changes {' '.join(sorted(changed))}")
    assert {"sum_in", "sum_out"} <= table["one list item dropped"] and "de" in table["one de row left unwritten"]
    assert {"s1", "s2"} <= table["one row dropped from the statistics"] and {"sum_in", "de"} <= table["neighbour of the batch's first item"]
