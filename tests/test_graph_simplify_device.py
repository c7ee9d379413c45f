"""gnnome_amd.simplify (csrc/graph_simplify.hip) against tests/graph_simplify_statement.py, bit for bit: transitive_edges, tip_nodes and
every tensor of simplify_graph's dict, on the simulated overlap graph and on hand-made graphs that sit on the rule's edges.  Everything
is an integer, so every comparison is exact.  On every graph the kept edge set must be closed under mates and a second launch must give
the same bytes."""
import numpy as np
import pytest
import torch

import graph_simplify_statement as gs
import overlap_graph_statement as st
from gnnome_amd import labels, overlapper, pipeline, simplify
from test_graph_simplify_statement import KW, line, mutate, tips_on_a_line

gpu = pytest.mark.gpu
TILE = 256          # out-edges of one node per LDS tile of the mark kernel (simplify.transitive_tile_size()); a wavefront is 64 lanes


def as_host(g):
    """The statement's view of a device graph dict."""
    out = {}
    for f, v in g.items():
        if torch.is_tensor(v):
            out[f] = v.cpu().numpy()
        elif f == "reads" and v is not None:
            out[f] = tuple(t.cpu().numpy() for t in v)
        elif f == "num_nodes":
            out[f] = v
    return out


def as_device(g):
    return {f: torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v for f, v in g.items()}


def same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and np.array_equal(got, want), what


def check(g, fuzz=10, max_tip=4, closed=True):
    """Every output of the module on the graph `g` (numpy or device dict) equals the statement's -> (device simplify_graph dict, the
    statement's), both with compact=True."""
    host = as_host(g) if torch.is_tensor(g["src"]) else g
    dev = g if torch.is_tensor(g["src"]) else as_device(g)
    want_mark = gs.transitive_edges(host, fuzz)
    mark = simplify.transitive_edges(dev, fuzz)
    assert mark.is_cuda and mark.dtype == torch.bool
    same(mark, want_mark, "transitive_edges")
    assert torch.equal(simplify.transitive_edges(dev, fuzz), mark)                          # two launches, equal bytes
    for keep in (None, ~want_mark):
        tip = simplify.tip_nodes(dev, None if keep is None else torch.from_numpy(keep).cuda(), max_tip)
        assert tip.is_cuda and tip.dtype == torch.bool
        same(tip, gs.tip_nodes(host, keep, max_tip), "tip_nodes")
        assert torch.equal(tip[0::2], tip[1::2])                                             # a node and its complement
    for compact in (False, True):
        want = gs.simplify_graph(host, fuzz, max_tip, compact=compact)
        runs = [simplify.simplify_graph(dev, fuzz, max_tip, compact=compact, check_mates=closed) for _ in range(2)]
        got = runs[0]
        assert got["num_nodes"] == want["num_nodes"] and got["removed"] == want["removed"]
        assert compact or got["num_nodes"] == host["num_nodes"]
        for f, w in want.items():
            if isinstance(w, np.ndarray):
                same(got[f], w, f)
                assert torch.equal(runs[1][f], got[f]), f
            elif f == "reads":
                same(got[f][0], w[0], "reads data")
                same(got[f][1], w[1], "reads off")
        if closed:
            assert gs.mate_closed(got["src"].cpu().numpy(), got["dst"].cpu().numpy())
        # the new dict indexes back into the input exactly; node pairing survives the renumbering
        origin, reads = got["edge_origin"].cpu().numpy(), got["kept_reads"].cpu().numpy()
        src, dst = got["src"].cpu().numpy(), got["dst"].cpu().numpy()
        assert np.array_equal(2 * reads[src >> 1] + (src & 1), host["src"][origin])
        assert np.array_equal(2 * reads[dst >> 1] + (dst & 1), host["dst"][origin])
        assert np.array_equal(got["prefix_length"].cpu().numpy(), host["prefix_length"][origin])
        assert (np.diff(origin) > 0).all() and (np.diff(reads) > 0).all()
        assert np.array_equal(got["read_length"].cpu().numpy(), host["read_length"].reshape(-1, 2)[reads].reshape(-1))
    return got, want


@pytest.fixture(scope="module")
def sim():
    return st.simulate()


def annotations(strand, start, end):
    node = lambda x, flip=False: torch.from_numpy(np.stack([x, -x if flip else x], 1).reshape(-1).astype(np.int64))   # noqa: E731
    return [node(strand, True), node(start), node(end), torch.ones(2 * len(start), dtype=torch.int64)]


# ---- the simulated graph ---------------------------------------------------------------------------------------------------------

@gpu
def test_simulated_graph_clean(sim):
    g = overlapper.overlap_graph(sim[1], annotations=annotations(*sim[2:]), **KW)
    g.pop("overlaps")
    got, want = check(g, fuzz=0)
    assert got["removed"] == {"transitive_edges": 156, "tip_nodes": 0, "reads": 78} and got["src"].numel() == 82
    assert int(torch.bincount(got["src"]).max()) == 1 and bool((got["overlap_similarity"] == 1.0).all())
    # the packed reads of the new dict are the old ones of kept_reads, byte for byte
    data, off = (t.cpu().numpy() for t in g["reads"])
    new_data, new_off = (t.cpu().numpy() for t in got["reads"])
    for i, r in enumerate(got["kept_reads"].tolist()):
        assert new_data[new_off[i]:new_off[i + 1]].tobytes() == data[off[r]:off[r + 1]].tobytes() == sim[1][r]
    for f in ("read_strand", "read_start", "read_end", "read_chr", "contained"):
        assert f in want and f in got


@gpu
def test_simulated_graph_mutated(sim):
    g = overlapper.overlap_graph(mutate(sim[1], seed=3), similarity=False, **KW)
    g.pop("overlaps")
    got, _ = check(g, fuzz=0)
    assert int(torch.bincount(got["src"]).max()) > 1                                        # indels move the prefixes: fuzz = 0 is not enough
    for fuzz in (5, 50):
        got, _ = check(g, fuzz=fuzz)
        assert got["removed"]["transitive_edges"] == 156 and int(torch.bincount(got["src"]).max()) == 1


# ---- the transitive rule on its edges --------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("ol,marked", ((310, True), (311, False), (290, True), (289, False)))
def test_triangle_with_the_residual_at_fuzz_and_one_beyond(ol, marked):
    """p(v -> w) + p(w -> x) - p(v -> x) = 300 + 400 - (1000 - ol) = ol - 300: -10 and 10 are inside fuzz = 10, -11 and 11 are not."""
    got, _ = check(gs.build([1000] * 3, [(0, 2, 700), (2, 4, 600), (0, 4, ol)]), fuzz=10)
    assert got["removed"]["transitive_edges"] == 2 * marked


@gpu
def test_the_exclusions_of_the_rule():
    cases = {"a 2-cycle": ([(0, 2, 500), (2, 0, 500)], 0),
             "an edge to the own complement, which is its own mate": ([(0, 1, 500), (0, 2, 500)], 0),
             "the same with a path 0 -> 2 -> 1 around it: w = 2 is neither end": ([(0, 1, 500), (0, 2, 500), (2, 1, 500)], 1),
             "the only two-hop path passes through x": ([(0, 2, 500), (2, 2, 1000)], 0),
             "the only two-hop path passes through v": ([(0, 2, 500), (0, 0, 1000)], 0)}
    for name, (ov, marked) in cases.items():
        got, _ = check(gs.build([1000] * 2, ov), fuzz=10 ** 6)
        assert got["removed"]["transitive_edges"] == marked, name


def hub_graph(hub, reads=320, targets=300):
    """Node `hub` has `targets` out-edges among 2 * reads nodes - more than a wavefront's 64 lanes and more than one LDS tile of 256 -
    and the targets have edges among themselves, so that hub edges in every tile are marked.  All reads are 10 000 long; hub -> t_i has
    p = 100 + 10 i; t_i -> t_(i+1) has p = 10 for even i and 11 (one base off) for odd i; t_i -> t_(i+2) has p = 20 where i % 4 == 0.
    At fuzz = 0 the odd targets and t_2, t_6, .. are explained, at fuzz = 1 every target but t_0."""
    rng = np.random.default_rng(5)
    others = np.array([r for r in range(reads) if r != hub >> 1])
    order = [2 * int(r) + int(s) for r, s in zip(rng.permutation(others)[:targets], rng.integers(0, 2, targets))]
    assert len(order) == targets
    ov = [(hub, t, 10000 - (100 + 10 * i)) for i, t in enumerate(order)]
    ov += [(order[i], order[i + 1], 10000 - (10 + i % 2)) for i in range(targets - 1)]
    ov += [(order[i], order[i + 2], 10000 - 20) for i in range(0, targets - 2, 4)]
    return gs.build([10000] * reads, ov)


@gpu
@pytest.mark.parametrize("hub", (0, 155, 639))
def test_a_hub_row_longer_than_a_wavefront_and_an_lds_tile(hub):
    """The hub's row is the first row, a middle one and the last one of the 640."""
    assert simplify.transitive_tile_size() == TILE
    g = hub_graph(hub)
    row = np.nonzero(g["src"] == hub)[0]
    assert len(row) == 300 > TILE > 64 and g["num_nodes"] == 640
    assert (g["src"].min() == hub) == (hub == 0) and (g["src"].max() == hub) == (hub == 639)
    by_dst = row[np.argsort(g["dst"][row], kind="stable")]                                  # the order the kernel tiles the row in
    marked = []
    for fuzz in (0, 1):
        want = gs.transitive_edges(g, fuzz)
        assert want[by_dst[:TILE]].any() and want[by_dst[TILE:]].any() and not want[by_dst].all()
        assert not want[by_dst[:TILE]].all() and not want[~np.isin(np.arange(len(want)), row)].all()
        marked.append(int(want[row].sum()))
        check(g, fuzz=fuzz)
    assert marked == [150 + 75, 299]


@gpu
def test_empty_graphs():
    empty = {"src": np.zeros(0, dtype=np.int64), "dst": np.zeros(0, dtype=np.int64), "num_nodes": 0,
             "prefix_length": np.zeros(0, dtype=np.int64), "overlap_length": np.zeros(0, dtype=np.int64),
             "read_length": np.zeros(0, dtype=np.int64)}
    got, _ = check(empty)
    assert got["num_nodes"] == 0 and got["src"].numel() == 0
    no_edges = dict(empty, num_nodes=10, read_length=np.full(10, 500, dtype=np.int64))
    got, _ = check(no_edges)
    assert got["num_nodes"] == 0 and got["removed"]["reads"] == 5
    assert simplify.simplify_graph(as_device(no_edges), compact=False)["num_nodes"] == 10


# ---- tips -----------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("max_tip,tip_reads", ((1, 1), (4, 5), (5, 10)))
def test_tips_of_length_one_max_tip_and_one_more_on_one_junction(max_tip, tip_reads):
    g = tips_on_a_line()
    got, want = check(g, fuzz=0, max_tip=max_tip)
    tip = simplify.tip_nodes(as_device(g), max_tip=max_tip).cpu().numpy()
    assert int(tip.sum()) == 2 * tip_reads and np.array_equal(tip[0::2], tip[1::2]) and tip[24] and tip[25]   # the complements too
    assert got["removed"]["reads"] == tip_reads and got["num_nodes"] == 44 - 2 * tip_reads


@gpu
def test_a_junction_fed_by_tips_only_keeps_the_heaviest_ties_to_the_smallest_node():
    tail = [(6, 8, 600), (8, 10, 600)]
    for ov, reads, tips in (([(0, 6, 700), (2, 6, 500), (4, 6, 600)], 6, [0, 1, 4, 5]),
                            ([(0, 6, 500), (2, 6, 500), (4, 6, 600)], 6, [2, 3, 4, 5]),
                            ([(12, 0, 600), (0, 6, 700), (2, 6, 500), (4, 6, 600)], 7, [2, 3, 4, 5])):
        g = gs.build([1000] * reads, ov + tail)
        check(g, fuzz=0)
        assert np.nonzero(simplify.tip_nodes(as_device(g)).cpu().numpy())[0].tolist() == tips


@gpu
def test_chains_that_are_no_tips():
    isolated = gs.build([1000] * 3, line(3))
    fork = gs.build([1000] * 6, [(0, 2, 500), (2, 4, 500), (2, 6, 400), (4, 8, 500), (6, 8, 500), (8, 10, 500)])
    for g in (isolated, fork):
        got, _ = check(g, fuzz=0)
        assert got["removed"]["tip_nodes"] == 0 and not simplify.tip_nodes(as_device(g)).any()
    keep = np.array([(u, v) not in ((2, 6), (7, 3)) for u, v in zip(fork["src"].tolist(), fork["dst"].tolist())])
    tip = simplify.tip_nodes(as_device(fork), torch.from_numpy(keep).cuda())
    same(tip, gs.tip_nodes(fork, keep), "tip_nodes with keep")
    assert np.nonzero(tip.cpu().numpy())[0].tolist() == [6, 7]


# ---- end to end -----------------------------------------------------------------------------------------------------------------

@gpu
def test_overlap_graph_simplify_keeps_true_edges_only(sim):
    genome, reads, strand, start, end = sim
    raw = overlapper.overlap_graph(reads, annotations=annotations(strand, start, end), **KW)
    g = overlapper.overlap_graph(reads, annotations=annotations(strand, start, end), simplify=True, **KW)
    assert raw["src"].numel() == 238 and "kept_reads" not in raw                            # the default is the raw graph, as before
    assert g["src"].numel() == 82 and g["num_nodes"] == 84
    ids, y = labels.process_graph(g)
    assert bool((y.cpu() == 1).all()) and ids.numel() == 82
    loose = overlapper.overlap_graph(reads, simplify={"compact": False, "fuzz": 0}, similarity=False, **KW)
    assert loose["num_nodes"] == 240 and torch.equal(loose["edge_origin"], g["edge_origin"])


@gpu
def test_assemble_reads_to_fasta_with_simplify_spells_the_covered_genome(sim, tmp_path):
    """The assertion of test_overlap_graph_device.py::test_assemble_reads_to_fasta_spells_the_covered_genome, on the simplified graph."""
    genome, reads, strand, start, end = sim
    path = tmp_path / "reads.fasta"
    with open(path, "w") as f:
        for i, (r, t, a, e) in enumerate(zip(reads, strand.tolist(), start.tolist(), end.tolist())):
            f.write(f">read_{i} strand={'+' if t == 1 else '-'} start={a} end={e} chr=1\n{r.decode()}\n")
    out = tmp_path / "asm.fasta"
    walks, contigs, stats, g = pipeline.assemble_reads_to_fasta(str(path), None, str(out), len_threshold=1000, use_labels=True,
                                                                simplify=True, **KW)
    covered = genome[int(start.min()):int(end.max())].decode()
    both = (genome.decode(), st.revcomp(genome).decode())
    assert len(contigs) >= 1 and contigs.sequence(0) in (covered, st.revcomp(covered.encode()).decode())
    assert all(any(contigs.sequence(i) in s for s in both) for i in range(len(contigs)))
    assert stats["longest_contig"] == len(covered) and out.read_text().count(">") == len(contigs)
    assert g["num_nodes"] == 84 and g["node_to_read"][0] == f"read_{int(g['kept_reads'][0])}"


def reads_with_a_tip():
    """Ten reads of 1500 bases every 500 bases of a random genome, every other one reverse-complemented, and read 10: 900 bases of the
    genome from 2100 on, then 400 random bases.  Its tail is longer than the max_hang = 200 of the test, so it dovetails with the reads
    that end inside its genome part (those from 1000 and 1500) and is an internal match for the reads that go on (from 2000, 2500)."""
    rng = np.random.default_rng(77)
    base = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = bytes(base[rng.integers(0, 4, 6000)])
    reads = [genome[s:s + 1500] if i % 2 == 0 else st.revcomp(genome[s:s + 1500]) for i, s in enumerate(range(0, 5000, 500))]
    return genome, reads + [genome[2100:3000] + bytes(base[rng.integers(0, 4, 400)])]


@gpu
def test_a_tip_built_from_sequence_is_removed_and_the_line_stays():
    genome, reads = reads_with_a_tip()
    kw = dict(KW, max_hang=200)
    host = st.graph(st.overlaps(reads, **kw))
    mark = gs.transitive_edges(host, 10)
    tip = gs.tip_nodes(host, ~mark, 4)
    out_deg = np.bincount(host["src"][~mark], minlength=22)
    assert np.nonzero(tip)[0].tolist() == [20, 21] and out_deg.max() == 2                   # the statement: one dead end of one read at a junction
    g = overlapper.overlap_graph(reads, similarity=False, **kw)
    g.pop("overlaps")
    got, want = check(g, fuzz=10)
    assert got["removed"]["tip_nodes"] == 2 and got["removed"]["reads"] == 1 and got["kept_reads"].tolist() == list(range(10))
    assert got["src"].numel() == 18 and int(torch.bincount(got["src"]).max()) == 1 and int(torch.bincount(got["dst"]).max()) == 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------

@gpu
def test_refusals():
    g = gs.build([1000] * 4, [(0, 2, 700), (2, 4, 600), (0, 4, 300)])                      # 6 edges, 8 nodes
    dev = as_device(g)
    one_missing = {f: (v[:-1] if torch.is_tensor(v) and v.numel() == 6 else v) for f, v in dev.items()}
    with pytest.raises(ValueError, match="mates"):
        simplify.simplify_graph(one_missing)
    assert simplify.simplify_graph(one_missing, tips=False, check_mates=False)["src"].numel() == 4   # 0 -> 4 went; 5 -> 1 lacks 5 -> 3
    with pytest.raises(ValueError, match="fuzz"):
        simplify.transitive_edges(dev, fuzz=-1)
    with pytest.raises(ValueError, match="fuzz"):
        simplify.simplify_graph(dev, fuzz=-1)
    with pytest.raises(ValueError, match="max_tip"):
        simplify.tip_nodes(dev, max_tip=0)
    with pytest.raises(ValueError, match="max_tip"):
        simplify.simplify_graph(dev, max_tip=0)
    with pytest.raises(ValueError, match="prefix_length"):
        simplify.simplify_graph({f: v for f, v in dev.items() if f != "prefix_length"})
    with pytest.raises(ValueError, match="simplify"):
        overlapper.overlap_graph([b"ACGT" * 100], simplify="yes")
