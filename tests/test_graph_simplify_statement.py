"""tests/graph_simplify_statement.py against properties that do not come from it (no GPU): on the simulated reads the transitive rule must
leave one line per strand, on both strands alike; on hand-made graphs the rule's exclusions and the tip rule's cases are spelled out."""
import numpy as np
import pytest

import graph_simplify_statement as gs
import overlap_graph_statement as st

KW = dict(k=15, w=5, max_occ=64, min_overlap=300)


def mutate(reads, seed, sub=0.01, indel=0.005):
    """The mutate of tests/test_overlap_graph_device.py."""
    rng = np.random.default_rng(seed)
    out = []
    for r in reads:
        s = bytearray()
        for c in r:
            x = rng.random()
            if x < indel / 2:
                continue                                   # a deletion
            if x < indel:
                s.append(b"ACGT"[rng.integers(4)])         # an insertion in front of the base
            s.append(b"ACGT"[(b"ACGT".index(c) + rng.integers(1, 4)) % 4] if rng.random() < sub else c)
        out.append(bytes(s))
    return out


@pytest.fixture(scope="module")
def sim():
    return st.simulate()


@pytest.fixture(scope="module")
def clean(sim):
    ov = st.overlaps(sim[1], **KW)
    return ov, st.graph(ov)


@pytest.fixture(scope="module")
def noisy(sim):
    ov = st.overlaps(mutate(sim[1], seed=3), **KW)
    return ov, st.graph(ov)


def degrees(g, keep):
    return (np.bincount(g["src"][keep], minlength=g["num_nodes"]), np.bincount(g["dst"][keep], minlength=g["num_nodes"]))


def is_one_line_per_strand(g, keep, reads_left):
    out_deg, in_deg = degrees(g, keep)
    return (out_deg.max() <= 1 and in_deg.max() <= 1 and int(keep.sum()) == 2 * (reads_left - 1)
            and gs.mate_closed(g["src"][keep], g["dst"][keep]))


def test_error_free_reads_reduce_to_one_line_per_strand(clean):
    ov, g = clean
    assert len(g["src"]) == 238 and int(np.bincount(g["src"]).max()) == 7 and int((~ov["contained"]).sum()) == 42
    mark = gs.transitive_edges(g, fuzz=0)
    assert int(mark.sum()) == 156 and int((~mark).sum()) == 82
    assert is_one_line_per_strand(g, ~mark, 42)
    mates = {(u, v): e for e, (u, v) in enumerate(zip(g["src"].tolist(), g["dst"].tolist()))}
    assert all(mark[e] == mark[mates[(v ^ 1, u ^ 1)]] for (u, v), e in mates.items())       # an edge is transitive iff its mate is
    assert not gs.tip_nodes(g, ~mark).any()                                                  # a line has no junction
    s = gs.simplify_graph(g, fuzz=0)
    assert s["num_nodes"] == 2 * 42 and len(s["src"]) == 82 and s["removed"] == {"transitive_edges": 156, "tip_nodes": 0, "reads": 78}
    assert np.array_equal(s["kept_reads"], np.nonzero(~ov["contained"])[0])                  # here the reads that are left are the line
    assert (s["read_length"][s["src"]] - s["overlap_length"] == s["prefix_length"]).all()


def test_mutated_reads_need_the_fuzz(noisy):
    ov, g = noisy
    mark = gs.transitive_edges(g, fuzz=0)
    assert degrees(g, ~mark)[0].max() == 5 and gs.mate_closed(g["src"][~mark], g["dst"][~mark])
    for fuzz in (5, 20, 50):
        mark = gs.transitive_edges(g, fuzz=fuzz)
        assert int(mark.sum()) == 156 and is_one_line_per_strand(g, ~mark, int((~ov["contained"]).sum())), fuzz


def test_the_rule_is_simultaneous_and_absolute():
    # reads 0 -> 1 -> 2 and 0 -> 2; lengths 1000: p(0->1) = 300, p(1->2) = 400, p(0->2) = 1000 - ol
    for ol, fuzz, want in ((300, 0, True), (310, 10, True), (311, 10, False), (289, 10, False), (290, 10, True)):
        g = gs.build([1000] * 3, [(0, 2, 700), (2, 4, 600), (0, 4, ol)])
        mark = gs.transitive_edges(g, fuzz)
        edges = list(zip(g["src"].tolist(), g["dst"].tolist()))
        assert mark[edges.index((0, 4))] == mark[edges.index((5, 1))] == want, (ol, fuzz)
        assert int(mark.sum()) == 2 * want
    # four reads 100 bases apart, every pair overlapping: 0 -> 3 is explained by 0 -> 1 and 1 -> 3, although 1 -> 3 goes as well
    g = gs.build([1000] * 4, [(2 * i, 2 * j, 1000 - 100 * (j - i)) for i in range(4) for j in range(i + 1, 4)])
    mark = gs.transitive_edges(g, 0)
    kept = sorted(zip(g["src"][~mark].tolist(), g["dst"][~mark].tolist()))
    assert kept == [(0, 2), (2, 4), (3, 1), (4, 6), (5, 3), (7, 5)]


def test_the_rule_excludes_w_equal_to_v_or_x():
    two_cycle = gs.build([1000] * 2, [(0, 2, 500), (2, 0, 500)])
    to_own_complement = gs.build([1000] * 2, [(0, 1, 500), (0, 2, 500)])
    loop_at_x = gs.build([1000] * 2, [(0, 2, 500), (2, 2, 1000)])           # the only two-hop path to x = 2 passes through x itself
    loop_at_v = gs.build([1000] * 2, [(0, 2, 500), (0, 0, 1000)])
    for g in (two_cycle, to_own_complement, loop_at_x, loop_at_v):
        assert not gs.transitive_edges(g, fuzz=10 ** 6).any()


def line(n, length=1000, ol=600):
    return [(2 * r, 2 * r + 2, ol) for r in range(n - 1)]


def tips_on_a_line():
    """Reads 0 .. 11 are the line; chains of 1, 4 and 5 reads (reads 12, 13 .. 16, 17 .. 21) run into read 7, node 14."""
    ov = line(12)
    ov += [(24, 14, 500)]
    ov += [(26, 28, 500), (28, 30, 500), (30, 32, 500), (32, 14, 500)]
    ov += [(34, 36, 500), (36, 38, 500), (38, 40, 500), (40, 42, 500), (42, 14, 500)]
    return gs.build([1000] * 22, ov)


def test_tips_of_length_one_max_tip_and_one_more():
    g = tips_on_a_line()
    node = np.arange(44)
    assert np.array_equal(gs.tip_nodes(g, max_tip=4), (node >= 24) & (node < 34))           # the complements 25, 27, .. included
    assert np.array_equal(gs.tip_nodes(g, max_tip=5), node >= 24)
    assert np.array_equal(gs.tip_nodes(g, max_tip=1), (node == 24) | (node == 25))
    s = gs.simplify_graph(g, fuzz=0, max_tip=4)
    assert s["removed"] == {"transitive_edges": 0, "tip_nodes": 10, "reads": 5} and s["num_nodes"] == 34
    assert gs.mate_closed(s["src"], s["dst"])


def test_a_junction_fed_by_tips_only_keeps_the_heaviest():
    # three dead ends meet in read 3, which leads on: the one with the largest summed p stays, the smallest last node on a tie
    tail = [(6, 8, 600), (8, 10, 600)]
    g = gs.build([1000] * 6, [(0, 6, 700), (2, 6, 500), (4, 6, 600)] + tail)
    assert np.nonzero(gs.tip_nodes(g))[0].tolist() == [0, 1, 4, 5]                          # p = 300, 500, 400: read 1 survives
    g = gs.build([1000] * 6, [(0, 6, 500), (2, 6, 500), (4, 6, 600)] + tail)
    assert np.nonzero(gs.tip_nodes(g))[0].tolist() == [2, 3, 4, 5]                          # 500, 500, 400: the tie goes to node 0
    g = gs.build([1000] * 7, [(12, 0, 600), (0, 6, 700), (2, 6, 500), (4, 6, 600)] + tail)
    assert np.nonzero(gs.tip_nodes(g))[0].tolist() == [2, 3, 4, 5]                          # 400 + 300 > 500: the sum over the chain counts


def test_chains_that_are_no_tips():
    isolated = gs.build([1000] * 3, line(3))                                                # ends in out-degree 0: a piece, not a tip
    assert not gs.tip_nodes(isolated).any()
    # read 0 -> read 1, which forks to reads 2 and 3 before any junction; 2 and 3 join again in read 4
    fork = gs.build([1000] * 6, [(0, 2, 500), (2, 4, 500), (2, 6, 400), (4, 8, 500), (6, 8, 500), (8, 10, 500)])
    assert not gs.tip_nodes(fork).any()
    # with keep: the edge 2 -> 6 and its mate masked out, read 3 becomes a start of a one-node chain into the junction read 4
    keep = np.array([(u, v) not in ((2, 6), (7, 3)) for u, v in zip(fork["src"].tolist(), fork["dst"].tolist())])
    assert np.nonzero(gs.tip_nodes(fork, keep))[0].tolist() == [6, 7]
