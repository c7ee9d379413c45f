"""gnnome_amd.bubbles (csrc/bubbles.hip) against tests/bubble_statement.py, bit for bit and dtype for dtype: bubble_arms, bubble_nodes,
pop_bubbles and simplify_graph(bubbles=True), on the diploid graphs, on every hand-made graph of tests/bubble_cases.py and on shapes that
sit on the wavefront, the LDS tile of the judgement kernel and the round count of the ranking.  Everything is an integer, so every
comparison is exact; a second call, and calls with other grids, must give the same bytes."""
import math

import numpy as np
import pytest
import torch

import bubble_cases as bc
import bubble_statement as bs
import graph_simplify_statement as gs
import overlap_graph_statement as st
from gnnome_amd import bubbles, overlapper, simplify
from test_graph_simplify_device import as_device, same
from test_graph_simplify_statement import KW

gpu = pytest.mark.gpu
WAVE = 64


def same_dict(got, want, other=None):
    for f, w in want.items():
        if isinstance(w, np.ndarray):
            same(got[f], w, f)
            assert other is None or torch.equal(other[f], got[f]), f
        elif f == "reads":
            same(got[f][0], w[0], "reads data")
            same(got[f][1], w[1], "reads off")
    assert got["num_nodes"] == want["num_nodes"] and got["removed"] == want["removed"]


def check(g, keep=None, pop=True, **kw):
    """Every output of the module on the numpy graph `g` equals the statement's -> (the mark as a numpy array, stats)."""
    dev = as_device(g)
    dkeep = None if keep is None else torch.from_numpy(keep).cuda()
    dkw = dict(kw, weight=torch.from_numpy(kw["weight"]).cuda()) if kw.get("weight") is not None else kw
    want_arms = bs.bubble_arms(g, keep, kw.get("weight"))
    arms = bubbles.bubble_arms(dev, dkeep, dkw.get("weight"))
    assert sorted(arms) == sorted(bs.ARM_KEYS)
    for f in bs.ARM_KEYS:
        assert arms[f].is_cuda
        same(arms[f], want_arms[f], f)
    want, stats = bs.bubble_nodes(g, keep, **kw), {}
    mark = bubbles.bubble_nodes(dev, dkeep, stats=stats, **dkw)
    assert mark.is_cuda and mark.dtype == torch.bool
    same(mark, want, "bubble_nodes")
    assert torch.equal(mark[0::2], mark[1::2])                                               # a node and its complement
    for grid in (0, 1, 3):                                                                    # equal bytes on every launch, for every grid
        assert torch.equal(bubbles.bubble_nodes(dev, dkeep, grid=grid, **dkw), mark), grid
    for f in ("unitig_rank_ms", "bubble_lists_ms", "bubble_arms_ms"):
        assert stats[f] >= 0
    if pop:
        for compact in (True, False):
            want_g = bs.pop_bubbles(g, keep=keep, compact=compact, **kw)
            runs = [bubbles.pop_bubbles(dev, keep=dkeep, compact=compact, **dkw) for _ in range(2)]
            same_dict(runs[0], want_g, runs[1])
            assert gs.mate_closed(runs[0]["src"].cpu().numpy(), runs[0]["dst"].cpu().numpy())
        if keep is None:
            sg_kw = dict(fuzz=0, bubbles=dkw or True)
            same_dict(simplify.simplify_graph(dev, **sg_kw), bs.simplify_graph(g, fuzz=0, bubbles=kw or True))
    return want, stats


@pytest.fixture(scope="module")
def sim():
    return st.simulate()


# ---- the diploid graphs ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("seed", bc.DIPLOID_SEEDS)
def test_diploid_graph(seed):
    raw = bc.diploid_graph(seed)
    g = gs.simplify_graph(raw, fuzz=0)
    mark, stats = check(g)
    assert mark.any() and stats["bubble_judge_ms"] >= 0 and stats["bubble_mark_ms"] >= 0
    got = simplify.simplify_graph(as_device(raw), fuzz=0, bubbles=True)                       # from the raw graph: one line per strand
    same_dict(got, bs.simplify_graph(raw, fuzz=0))
    assert int(torch.bincount(got["src"]).max()) == 1 and int(torch.bincount(got["dst"]).max()) == 1
    assert got["removed"]["bubble_nodes"] == int(mark.sum()) and got["removed"]["bubble_rounds"] == 1


# ---- the hand-made graphs -------------------------------------------------------------------------------------------------------

@gpu
def test_the_choice_of_the_winner():
    g, a1, a3 = bc.two_arms(1, 3)
    assert np.nonzero(check(g)[0])[0].tolist() == [8, 9]
    weight = np.ones(g["num_nodes"], dtype=np.int64)
    weight[[8, 9]] = 4
    assert np.nonzero(check(g, weight=weight)[0])[0].tolist() == [10, 11, 12, 13, 14, 15]
    assert np.nonzero(check(bc.two_arms(2, 2, ol1=[500, 500, 500], ol2=[500, 501, 500])[0])[0])[0].tolist() == [8, 9, 10, 11]
    for flip in (False, True):
        assert np.nonzero(check(bc.two_arms(2, 2, flip=flip)[0])[0])[0].tolist() == [12, 13, 14, 15]


@gpu
def test_the_two_bounds_and_one_beyond():
    g = bc.two_arms(1, 3, ol2=675)[0]                                                       # dist 0 and 300, the winner is the far one
    for kw, pops in ((dict(max_diff=300), True), (dict(max_diff=299), False), (dict(max_dist=300), True), (dict(max_dist=299), False)):
        assert bool(check(g, **kw)[0].any()) == pops, kw
    g = bc.two_arms(1, 3, ol1=300, ol2=750)[0]                                              # dist 400 and 0, the loser is the far one
    for kw, pops in ((dict(max_dist=400), True), (dict(max_dist=399), False)):
        assert bool(check(g, **kw)[0].any()) == pops, kw
    assert check(bc.two_arms(1, 3, ol1=600, ol2=800)[0], max_diff=0)[0].any()               # both at -200


@gpu
def test_shapes_that_are_no_bubble():
    for name, g in bc.no_bubble_graphs().items():
        assert not check(g)[0].any(), name
    g = bc.two_arms(1, 3)[0]
    dev = as_device(g)
    weight = torch.ones(g["num_nodes"], dtype=torch.int64)
    weight[8] = 2
    for fn in (bubbles.bubble_nodes, bubbles.bubble_arms, bubbles.pop_bubbles):
        with pytest.raises(ValueError, match="weight"):
            fn(dev, weight=weight)
        with pytest.raises(ValueError, match="weight"):
            fn(dev, weight=torch.ones(g["num_nodes"]))
        with pytest.raises(ValueError, match="mates"):
            fn(dev, keep=torch.arange(len(g["src"])) > 0)
        with pytest.raises(ValueError, match="prefix_length"):
            fn(dict(dev, prefix_length=dev["prefix_length"] + 1))
    with pytest.raises(ValueError, match="weight"):
        simplify.simplify_graph(dev, bubbles={"weight": weight})
    with pytest.raises(ValueError, match="max_diff"):
        bubbles.bubble_nodes(dev, max_diff=-1)
    with pytest.raises(ValueError, match="rounds"):
        bubbles.pop_bubbles(dev, rounds=0)
    for bad in ("yes", 1, False):
        with pytest.raises(ValueError, match="bubbles"):
            simplify.simplify_graph(dev, bubbles=bad)
    with pytest.raises(ValueError, match="bubbles"):
        simplify.simplify_graph(dev, bubbles={"max_tip": 3})


@gpu
def test_two_bubbles_at_one_source_a_nested_bubble_and_a_keep_mask():
    assert np.nonzero(check(bc.two_bubbles_at_one_source())[0])[0].tolist() == [8, 9, 12, 13, 14, 15]
    g = bc.nested_bubble()
    assert np.nonzero(check(g)[0])[0].tolist() == [12, 13]
    dev, stats = as_device(g), {}
    assert bubbles.pop_bubbles(dev, rounds=1)["removed"] == {"bubble_nodes": 2, "bubble_rounds": 1, "reads": 1}
    assert bubbles.pop_bubbles(dev, stats=stats)["removed"] == {"bubble_nodes": 4, "bubble_rounds": 2, "reads": 2}
    assert stats["bubble_rounds"] == 2 and stats["bubble_judge_ms"] >= 0 and stats["compact_ms"] >= 0
    same_dict(simplify.simplify_graph(dev, fuzz=0, bubbles={"rounds": 1}), bs.simplify_graph(g, fuzz=0, bubbles={"rounds": 1}))
    g = bc.two_arms(1, 3)[0]
    keep = np.array([e not in {(10, 12), (13, 11)} for e in zip(g["src"].tolist(), g["dst"].tolist())])
    assert not check(g, keep=keep)[0].any()


# ---- a wavefront, the LDS tile, the ranking ----------------------------------------------------------------------------------------

@gpu
def test_more_arms_at_one_source_than_a_wavefront_has_lanes():
    g, arm = bc.hub_bubbles(0)
    mark, _ = check(g)
    assert len(arm) == 70 > WAVE and int(mark.sum()) == 2 * (70 - 3)                          # the last arm of every sink stays


@gpu
@pytest.mark.parametrize("place", ("first", "middle", "last"))
def test_a_source_row_longer_than_the_lds_tile(place):
    tile = bubbles.bubble_tile_size()
    arms = tile + 72
    reads = arms + 4
    hub = {"first": 0, "middle": reads - 1, "last": 2 * reads - 1}[place]
    g, arm = bc.hub_bubbles(hub, arms=arms, step=3)
    assert int((g["src"] == hub).sum()) == arms > tile > WAVE
    assert (g["src"].min() == hub) == (place == "first") and (g["src"].max() == hub) == (place == "last")
    mark, _ = check(g, pop=place == "middle")
    marked = [bool(mark[a]) for a in arm]
    assert not any(marked[-3:]) and all(marked[-150:-3]) and not any(marked[:10])            # winners; losers; further off than max_diff


@gpu
def test_an_arm_longer_than_any_lane_could_walk():
    g, long, short = bc.two_arms(300, 2, ol1=995)                                           # dist 300 000 - 301 * 995 = 505 beside 500
    mark, stats = check(g)
    assert np.nonzero(mark)[0].tolist() == sorted(short + [v ^ 1 for v in short])
    assert stats["rank_rounds"] == math.ceil(math.log2(300 - 1))                            # O(log n) launches, no walk


@gpu
def test_empty_graphs_and_graphs_without_a_fork():
    empty = {"src": np.zeros(0, dtype=np.int64), "dst": np.zeros(0, dtype=np.int64), "num_nodes": 0,
             "prefix_length": np.zeros(0, dtype=np.int64), "overlap_length": np.zeros(0, dtype=np.int64),
             "read_length": np.zeros(0, dtype=np.int64)}
    assert check(empty)[0].size == 0
    assert not check(dict(empty, num_nodes=10, read_length=np.full(10, 500, dtype=np.int64)))[0].any()
    line = gs.build([1000] * 70, bc.chain(list(range(0, 140, 2))))
    assert not check(line)[0].any()                                                          # no source of out-degree >= 2
    g = bc.two_arms(1, 3)[0]
    assert not check(g, keep=np.zeros(len(g["src"]), dtype=bool))[0].any()                   # keep all false


# ---- the wiring -----------------------------------------------------------------------------------------------------------------

@gpu
def test_a_haploid_line_has_no_bubble(sim):
    plain = overlapper.overlap_graph(sim[1], simplify=dict(fuzz=0), unitigs=True, **KW)
    popped = overlapper.overlap_graph(sim[1], simplify=dict(fuzz=0, bubbles=True), unitigs=True, **KW)
    assert sorted(plain) == sorted(popped) and popped["num_nodes"] == 2
    for f, v in plain.items():
        if torch.is_tensor(v):
            assert torch.equal(popped[f], v), f
        elif f == "reads":
            assert torch.equal(popped[f][0], v[0]) and torch.equal(popped[f][1], v[1])
        else:
            assert popped[f] == v, f
    g = overlapper.overlap_graph(sim[1], simplify=dict(fuzz=0, bubbles=True), **KW)
    assert g["removed"] == {"transitive_edges": 156, "tip_nodes": 0, "bubble_nodes": 0, "bubble_rounds": 0, "reads": 78}


@gpu
def test_without_the_keyword_removed_has_its_three_keys():
    g = bc.two_arms(1, 3)[0]
    assert simplify.simplify_graph(as_device(g), fuzz=0)["removed"] == {"transitive_edges": 0, "tip_nodes": 0, "reads": 0}
    assert sorted(simplify.simplify_graph(as_device(g))["removed"]) == ["reads", "tip_nodes", "transitive_edges"]
