"""tests/unitig_statement.py against properties that do not come from it (no GPU): the simulated reads reduce to one unitig pair that spells
the covered genome; on random mate-closed graphs the chains partition the nodes, never meet their complements and leave a graph on which
compaction changes nothing; hand-made graphs spell out the link rule's exclusions, the cut of a cycle and the refusals."""
import numpy as np
import pytest

import graph_simplify_statement as gs
import overlap_graph_statement as st
import unitig_statement as us
from test_graph_simplify_statement import KW


def pack(reads):
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), off


def with_reads(g, seed=0):
    """g with random sequences of its read lengths: spelling only cuts and joins them."""
    rng = np.random.default_rng(seed)
    base = np.frombuffer(b"ACGT", dtype=np.uint8)
    return dict(g, reads=pack([bytes(base[rng.integers(0, 4, n)]) for n in g["read_length"][0::2].tolist()]))


def random_graph(seed, reads=300):
    """`reads` reads of 50 .. 150 bases in random orientations: a line through a third of them, so that long chains exist, cycles of
    2, 2, 3, 3, 5 and 9 others, and 0.2 random overlaps per read on top, which break some of both and add forks, joins, hairpins,
    self-loops and parallel pairs as they fall."""
    rng = np.random.default_rng(seed)
    length = rng.integers(50, 151, reads)
    node = [2 * int(r) + int(s) for r, s in zip(rng.permutation(reads), rng.integers(0, 2, reads))]
    walk, at = node[:reads // 3], reads // 3
    ov = [(u, v, int(rng.integers(10, 41))) for u, v in zip(walk, walk[1:])]
    for n in (2, 2, 3, 3, 5, 9):
        ring, at = node[at:at + n], at + n
        ov += [(u, v, int(rng.integers(10, 41))) for u, v in zip(ring, ring[1:] + ring[:1])]
    ov += [(int(u), int(v), int(rng.integers(10, 41))) for u, v in rng.integers(0, 2 * reads, (int(0.2 * reads), 2))]
    return with_reads(gs.build(length, ov), seed)


def line_graph(n, first=0, flip=()):
    """n reads first .. first + n - 1 in a line (those in `flip` reverse-complemented) -> overlaps for gs.build."""
    node = [2 * (first + i) + (i in flip) for i in range(n)]
    return [(u, v, 400 + 7 * (i % 5)) for i, (u, v) in enumerate(zip(node, node[1:]))]


def cycle_graph(n, first=0, flip=()):
    node = [2 * (first + i) + (i in flip) for i in range(n)]
    return [(u, v, 400 + 7 * (i % 5)) for i, (u, v) in enumerate(zip(node, node[1:] + node[:1]))]


def chains_of(c):
    off, nodes = c["chain_off"].tolist(), c["chain_nodes"].tolist()
    return [nodes[a:b] for a, b in zip(off, off[1:])]


def properties(g):
    """What the issue asks of every compaction -> (chains dict, unitig graph)."""
    N, E = g["num_nodes"], len(g["src"])
    c, u = us.unitig_chains(g), us.compact_unitigs(g)
    chains = chains_of(c)
    U = len(chains)
    assert U % 2 == 0 and u["num_nodes"] == U
    assert sorted(c["chain_nodes"].tolist()) == list(range(N))                               # every node is in one chain
    for j, chain in enumerate(chains):
        assert all(c["unitig"][v] == j and c["rank"][v] == i for i, v in enumerate(chain))
        assert not {v ^ 1 for v in chain} & set(chain)                                        # no chain meets its complement
        assert chains[j ^ 1] == [v ^ 1 for v in reversed(chain)]                              # which is the other chain of the pair
    heads = [chain[0] for chain in chains]
    assert all(heads[j] < heads[j + 1] for j in range(0, U, 2)) and heads[0::2] == sorted(heads[0::2])
    assert int(c["link"].sum()) + len(u["src"]) == E
    src, dst = np.asarray(g["src"]), np.asarray(g["dst"])
    last = np.diff(c["chain_off"])[c["unitig"]] - 1
    kept = ~c["link"]
    assert (c["rank"][src[kept]] == last[src[kept]]).all() and (c["rank"][dst[kept]] == 0).all()   # every kept edge runs tail to head
    internal = c["link"]
    assert (c["unitig"][src[internal]] == c["unitig"][dst[internal]]).all() and (c["rank"][dst[internal]] == c["rank"][src[internal]] + 1).all()
    assert np.array_equal(c["length"][0::2], c["length"][1::2])
    assert gs.mate_closed(u["src"], u["dst"])
    again = us.compact_unitigs(u)                                                             # idempotent
    assert np.array_equal(again["chain_off"], np.arange(U + 1)) and np.array_equal(again["chain_nodes"], np.arange(U))
    for f in ("src", "dst", "overlap_length", "prefix_length", "read_length"):
        assert np.array_equal(again[f], u[f]), f
    if "reads" in u:
        assert np.array_equal(np.diff(u["reads"][1]), c["length"][0::2]) and np.array_equal(again["reads"][0], u["reads"][0])
    return c, u


@pytest.fixture(scope="module")
def sim():
    return st.simulate()


@pytest.fixture(scope="module")
def simplified(sim):
    g = st.graph(st.overlaps(sim[1], **KW))
    g["reads"] = pack(sim[1])
    return gs.simplify_graph(g, fuzz=0)


def test_the_simulated_reads_are_one_unitig_that_spells_the_covered_genome(sim, simplified):
    genome, reads, strand, start, end = sim
    c, u = properties(simplified)
    assert u["num_nodes"] == 2 and len(u["src"]) == 0 and int(c["link"].sum()) == 82
    chains = chains_of(c)
    assert len(chains[0]) == 42 and chains[1] == [v ^ 1 for v in reversed(chains[0])] and not c["circular"].any()
    covered = genome[int(start.min()):int(end.max())]
    data, off = u["reads"]
    assert off.tolist() == [0, len(covered)] and data.tobytes() in (covered, st.revcomp(covered))
    assert us.spell(simplified, chains[1]) == st.revcomp(data.tobytes())


@pytest.mark.parametrize("seed", range(6))
def test_random_mate_closed_graphs(seed):
    g = random_graph(seed)
    c, u = properties(g)
    sizes = np.diff(c["chain_off"])
    assert sizes.max() >= 4 and (sizes == 1).any() and 0 < len(u["src"]) < len(g["src"])


def test_the_random_graphs_keep_cycles_and_break_cycles():
    circular = [int(us.unitig_chains(random_graph(seed))["circular"].sum()) for seed in range(6)]
    assert min(circular) >= 2 and max(circular) <= 10 and len(set(circular)) > 1


def test_hairpin_self_loop_and_parallel_pair_are_no_links():
    hairpin = gs.build([1000] * 2, [(0, 2, 500), (2, 3, 400)])                               # 2 -> 3 is 2 -> 2 ^ 1, its own mate
    c, u = properties(hairpin)
    assert chains_of(c) == [[0, 2], [3, 1]] and c["link"].tolist() == [True, False, True]
    assert (u["src"].tolist(), u["dst"].tolist(), u["overlap_length"].tolist(), u["prefix_length"].tolist()) == ([0], [1], [400], [1100])
    loop = gs.build([1000] * 2, [(0, 0, 300), (2, 0, 500)])                                  # node 0: in-degree 2; 1 -> 1 and 1 -> 3 likewise
    c, u = properties(loop)
    assert not c["link"].any() and len(u["src"]) == 4 and np.array_equal(c["chain_off"], np.arange(5))
    only_loop = gs.build([1000], [(0, 0, 300)])                                              # degrees 1 and 1, and still no link
    c, u = properties(only_loop)
    assert not c["link"].any() and not c["circular"].any() and u["src"].tolist() == [0, 1] and u["dst"].tolist() == [0, 1]
    parallel = gs.build([1000] * 2, [(0, 2, 500), (0, 2, 400)])
    c, u = properties(parallel)
    assert not c["link"].any() and len(u["src"]) == 4


def test_a_fork_and_a_join():
    g = gs.build([1000] * 6, [(0, 2, 500), (2, 4, 500), (2, 6, 400), (4, 8, 500), (6, 8, 500), (8, 10, 500)])
    c, u = properties(g)
    assert chains_of(c) == [[0, 2], [3, 1], [4], [5], [6], [7], [8, 10], [11, 9]]
    assert int(c["link"].sum()) == 4 and len(u["src"]) == 8
    assert c["length"].tolist() == [1500, 1500, 1000, 1000, 1000, 1000, 1500, 1500] and c["offset"][[2, 1, 10, 9]].tolist() == [500] * 4
    assert sorted(zip(u["src"].tolist(), u["dst"].tolist())) == [(0, 2), (0, 4), (2, 6), (3, 1), (4, 6), (5, 1), (7, 3), (7, 5)]


def test_cycles_are_cut_at_their_smallest_read():
    two = gs.build([1000, 800], cycle_graph(2))                                              # 0 -> 2 -> 0 and 1 -> 3 -> 1
    c, u = properties(two)
    assert chains_of(c) == [[0, 2], [3, 1]] and c["circular"].all() and c["link"].tolist() == [True, False, False, True]
    assert (u["src"].tolist(), u["dst"].tolist()) == ([1, 0], [1, 0])                        # the cut links 1 -> 3 and 2 -> 0 as self-edges
    assert c["length"].tolist() == [1000 - 400 + 800] * 2 and u["prefix_length"].tolist() == [1400 - 407, 1400 - 407]
    three = gs.build([1000] * 4, cycle_graph(3, first=1))                                    # read 0 alone; 2 -> 4 -> 6 -> 2
    c, u = properties(three)
    assert chains_of(c) == [[0], [1], [2, 4, 6], [7, 5, 3]] and c["circular"].tolist() == [False, False, True, True]
    assert sorted(zip(u["src"].tolist(), u["dst"].tolist())) == [(2, 2), (3, 3)]
    flipped = gs.build([1000] * 4, cycle_graph(3, first=1, flip=(0,)))                       # 3 -> 4 -> 6 -> 3: the cycle ends at 3 = 2r + 1
    c, u = properties(flipped)
    assert chains_of(c) == [[0], [1], [2, 7, 5], [4, 6, 3]] and c["circular"].tolist() == [False, False, True, True]
    src, dst = flipped["src"].tolist(), flipped["dst"].tolist()
    cut = sorted((src[e], dst[e]) for e in np.nonzero(~c["link"])[0])
    assert cut == [(3, 4), (5, 2)]
    beside = gs.build([1000] * 9, line_graph(4) + cycle_graph(3, first=4) + line_graph(2, first=7))
    c, u = properties(beside)
    assert chains_of(c)[0::2] == [[0, 2, 4, 6], [8, 10, 12], [14, 16]] and c["circular"].tolist() == [False, False, True, True, False, False]


def test_a_line_with_flipped_reads_is_one_pair():
    g = with_reads(gs.build(np.arange(900, 910), line_graph(10, flip=(0, 3, 4, 9))))
    c, u = properties(g)
    assert len(chains_of(c)) == 2 and len(u["src"]) == 0
    assert chains_of(c)[0] == [1, 2, 4, 7, 9, 10, 12, 14, 16, 19] and c["offset"][19] == sum(g["prefix_length"][g["src"] == v][0] for v in chains_of(c)[0][:-1])


def test_refusals():
    g = gs.build([1000] * 3, [(0, 2, 500), (2, 4, 500)])
    cut = {f: (v[:-1] if isinstance(v, np.ndarray) and len(v) == 4 else v) for f, v in g.items()}
    with pytest.raises(ValueError, match="mates"):
        us.unitig_chains(cut)
    with pytest.raises(ValueError, match="prefix_length"):
        us.unitig_chains(dict(g, prefix_length=g["prefix_length"] + np.array([0, 1, 0, 0])))
    with pytest.raises(ValueError, match="prefix_length"):
        us.compact_unitigs(dict(g, overlap_length=g["overlap_length"] - 1))
