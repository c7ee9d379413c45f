"""gnnome_amd.unitigs (csrc/unitigs.hip) against tests/unitig_statement.py, bit for bit and dtype for dtype: unitig_chains and every tensor of
compact_unitigs, on the simulated overlap graph, on random mate-closed graphs and on lines and cycles whose sizes sit on the wavefront, the
workgroup and the round count of the ranking.  Everything is an integer, so every comparison is exact; a second call, and calls with
other grids, must give the same bytes.  Then the GFA round trip through gfa.read_gfa and the pipeline on the unitig graph."""
import math

import numpy as np
import pytest
import torch

import graph_simplify_statement as gs
import overlap_graph_statement as st
import unitig_statement as us
from gnnome_amd import gfa, overlapper, pipeline, unitigs
from test_graph_simplify_device import as_host, hub_graph, same
from test_graph_simplify_statement import KW, mutate
from test_unitig_statement import cycle_graph, line_graph, random_graph, with_reads

gpu = pytest.mark.gpu
CHAIN_KEYS = ("unitig", "rank", "offset", "chain_off", "chain_nodes", "length", "circular", "link")


def as_device(g):
    out = {}
    for f, v in g.items():
        out[f] = torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else tuple(torch.from_numpy(t).cuda() for t in v) if f == "reads" else v
    return out


def check(g):
    """Every output of the module on the graph `g` (numpy or device dict) equals the statement's -> (chains, unitig graph, stats)."""
    host = as_host(g) if torch.is_tensor(g["src"]) else g
    dev = g if torch.is_tensor(g["src"]) else as_device(g)
    want, stats = us.unitig_chains(host), {}
    got = unitigs.unitig_chains(dev, stats=stats)
    assert sorted(got) == sorted(CHAIN_KEYS)
    for f in CHAIN_KEYS:
        assert got[f].is_cuda
        same(got[f], want[f], f)
    for grid in (0, 1, 3):                                                                    # equal bytes on every launch, for every grid
        again = unitigs.unitig_chains(dev, grid=grid)
        assert all(torch.equal(again[f], got[f]) for f in CHAIN_KEYS), grid
    want_u = us.compact_unitigs(host)
    runs = [unitigs.compact_unitigs(dev) for _ in range(2)]
    got_u = runs[0]
    assert got_u["num_nodes"] == want_u["num_nodes"]
    for f, w in want_u.items():
        if isinstance(w, np.ndarray):
            same(got_u[f], w, f)
            assert torch.equal(runs[1][f], got_u[f]), f
        elif f == "reads":
            same(got_u[f][0], w[0], "reads data")
            same(got_u[f][1], w[1], "reads off")
            assert torch.equal(runs[1][f][0], got_u[f][0])
    assert (stats["cycle_nodes"] > 0) == bool(want["circular"].any())
    if not want["circular"].any():                                                            # no cycle: the cycle phase is not paid for
        assert stats["cycle_min_rounds"] == 0 and stats["cycle_rank_rounds"] == 0
    for f in ("unitig_lists_ms", "unitig_links_ms", "unitig_rank_ms", "unitig_number_ms", "unitig_scatter_ms"):
        assert stats[f] >= 0
    return got, got_u, stats


def path(nodes, closed=False):
    nxt = nodes[1:] + (nodes[:1] if closed else [])
    return [(u, v, 300 + 11 * (i % 7)) for i, (u, v) in enumerate(zip(nodes, nxt))]


@pytest.fixture(scope="module")
def sim():
    return st.simulate()


# ---- the simulated graph ---------------------------------------------------------------------------------------------------------

@gpu
def test_simulated_graph_clean(sim):
    genome, reads, strand, start, end = sim
    g = overlapper.overlap_graph(reads, simplify={"fuzz": 0}, **KW)
    g.pop("overlaps")
    c, u, stats = check(g)
    assert u["num_nodes"] == 2 and u["src"].numel() == 0 and c["chain_off"].tolist() == [0, 42, 84] and stats["rank_rounds"] == 6
    covered = genome[int(start.min()):int(end.max())]
    assert u["reads"][0].cpu().numpy().tobytes() in (covered, st.revcomp(covered))
    direct = overlapper.overlap_graph(reads, simplify={"fuzz": 0}, unitigs=True, **KW)
    assert direct["num_nodes"] == 2 and torch.equal(direct["reads"][0], u["reads"][0]) and "overlaps" not in direct
    assert "chain_nodes" not in overlapper.overlap_graph(reads, simplify={"fuzz": 0}, similarity=False, **KW)   # the default: no unitigs


@gpu
def test_simulated_graph_mutated(sim):
    g = overlapper.overlap_graph(mutate(sim[1], seed=3), simplify={"fuzz": 0}, **KW)          # fuzz = 0 leaves forks and joins
    g.pop("overlaps")
    c, u, _ = check(g)
    assert 2 < u["num_nodes"] < g["num_nodes"] and 0 < u["src"].numel() < g["src"].numel()
    assert torch.equal(u["overlap_similarity"], g["overlap_similarity"][u["edge_origin"]])


@gpu
@pytest.mark.parametrize("seed", range(6))
def test_random_graphs(seed):
    c, u, stats = check(random_graph(seed))
    assert stats["cycle_nodes"] > 0 and bool(c["circular"].any())


# ---- lines and cycles on the edges of a wavefront, a workgroup and the round count ---------------------------------------------------

@gpu
@pytest.mark.parametrize("n", (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 5000))
def test_a_line(n):
    g = gs.build(1000 + np.arange(n) % 13, line_graph(n, flip=(0, 2, n // 2, n - 1)))
    c, u, stats = check(g if n > 300 else with_reads(g))
    assert u["num_nodes"] == 2 and u["src"].numel() == 0 and c["chain_off"].tolist() == [0, n, 2 * n]
    assert stats["rank_rounds"] == (math.ceil(math.log2(n - 1)) if n > 2 else 0)             # a chain of n nodes: O(log n) launches


@gpu
def test_several_lines_with_interleaved_heads():
    rng = np.random.default_rng(11)
    sizes = (700, 130, 65, 64, 7, 1)
    reads = rng.permutation(sum(sizes)).tolist()
    ov, at = [], 0
    for n in sizes:
        ov += path([2 * r + int(s) for r, s in zip(reads[at:at + n], rng.integers(0, 2, n))])
        at += n
    c, u, stats = check(gs.build(900 + rng.integers(0, 200, sum(sizes)), ov))
    assert u["num_nodes"] == 2 * len(sizes) and sorted(torch.diff(c["chain_off"]).tolist()) == sorted(2 * sizes)
    assert stats["rank_rounds"] == 10 and stats["cycle_nodes"] == 0


@gpu
@pytest.mark.parametrize("n", (2, 3, 64, 65, 1000))
def test_cycles_alone_and_beside_lines(n):
    c, u, stats = check(gs.build([1000] * n, cycle_graph(n)))
    assert u["num_nodes"] == 2 and c["circular"].tolist() == [True, True] and c["chain_nodes"][0] == 0 and stats["cycle_nodes"] == 2 * n
    assert (u["src"].tolist(), u["dst"].tolist()) in (([0, 1], [0, 1]), ([1, 0], [1, 0]))     # the cut links as self-edges
    assert stats["cycle_min_rounds"] == math.ceil(math.log2(2 * n))
    rng = np.random.default_rng(n)
    total = 10 + n + 300 + 3
    reads = rng.permutation(total).tolist()
    node = [2 * r + int(s) for r, s in zip(reads, rng.integers(0, 2, total))]
    ov = path(node[:10]) + path(node[10:10 + n], closed=True) + path(node[10 + n:310 + n]) + path(node[310 + n:], closed=True)
    c, u, stats = check(with_reads(gs.build(800 + rng.integers(0, 300, total), ov)))
    assert u["num_nodes"] == 8 and int(c["circular"].sum()) == 4 and stats["cycle_nodes"] == 2 * (n + 3)
    ring, off, nodes = node[10:10 + n], c["chain_off"].tolist(), c["chain_nodes"].tolist()
    i = min(range(n), key=lambda k: ring[k] >> 1)                                             # the cycle starts at 2r, or ends at 2r + 1
    k = i if ring[i] % 2 == 0 else (i + 1) % n
    j = int(c["unitig"][ring[k]])
    assert nodes[off[j]:off[j + 1]] == ring[k:] + ring[:k] and bool(c["circular"][j])


@gpu
def test_graphs_without_links_and_without_edges():
    c, u, _ = check(gs.build([1000] * 4, [(0, 2, 500), (0, 4, 500), (6, 2, 400), (6, 4, 300), (0, 0, 100), (5, 4, 200)]))
    assert not c["link"].any() and u["num_nodes"] == 8 and u["src"].numel() == 11
    empty = {"src": np.zeros(0, dtype=np.int64), "dst": np.zeros(0, dtype=np.int64), "num_nodes": 0,
             "prefix_length": np.zeros(0, dtype=np.int64), "overlap_length": np.zeros(0, dtype=np.int64),
             "read_length": np.zeros(0, dtype=np.int64)}
    c, u, _ = check(empty)
    assert u["num_nodes"] == 0 and c["chain_off"].tolist() == [0]
    c, u, _ = check(with_reads(dict(empty, num_nodes=10, read_length=np.repeat(np.arange(500, 505), 2))))
    assert u["num_nodes"] == 10 and c["chain_nodes"].tolist() == list(range(10)) and torch.equal(u["read_length"], c["length"])


@gpu
def test_a_300_way_hub():
    g = hub_graph(0)
    c, u, _ = check(g)
    assert int(torch.bincount(u["src"]).max()) == 300 and int(u["src"][u["edge_origin"] == 0]) == int(c["unitig"][0])


# ---- the GFA round trip ----------------------------------------------------------------------------------------------------------

def round_trip(u, path):
    unitigs.write_gfa(u, str(path))
    back = gfa.read_gfa(str(path), similarity=None, keep_sequences=True)
    assert back["num_nodes"] == u["num_nodes"]
    edges = lambda g: sorted(zip(*(torch.as_tensor(g[f]).tolist() for f in ("src", "dst", "overlap_length", "prefix_length"))))   # noqa: E731
    assert edges(back) == edges(u) and torch.equal(back["read_length"], torch.as_tensor(u["read_length"]).cpu())
    data, off = u["reads"][0].cpu().numpy().tobytes(), u["reads"][1].tolist()
    for r in range(u["num_nodes"] // 2):
        assert back["read_seqs"][2 * r] == data[off[r]:off[r + 1]].decode()
    if u.get("overlap_similarity") is not None and u["src"].numel():                          # read_gfa: no L line, no similarities
        sim = lambda g: dict(zip(zip(g["src"].tolist(), g["dst"].tolist()), g["overlap_similarity"].tolist()))   # noqa: E731
        assert sim(back) == sim(u)
    else:
        assert back["overlap_similarity"] is None
    return back


@gpu
def test_gfa_round_trip(sim, tmp_path):
    g = overlapper.overlap_graph(mutate(sim[1], seed=3), simplify={"fuzz": 0}, **KW)
    g["node_to_read"] = {v: f"r{int(g['kept_reads'][v >> 1])}" for v in range(g["num_nodes"])}
    u = unitigs.compact_unitigs(g)
    back = round_trip(u, tmp_path / "sim.gfa")
    assert u["src"].numel() > 0 and all(back["node_to_read"][v] == u["node_to_read"][v] for v in range(u["num_nodes"]))
    assert back["read_to_node"] == u["read_to_node"] and back["read_to_node2"] == u["read_to_node2"]
    assert u["node_to_read"][0][0][0].startswith("r") and max(len(m) for m in u["node_to_read"].values()) > 1
    lines = (tmp_path / "sim.gfa").read_text().splitlines()
    assert sum(x[0] == "S" for x in lines) == u["num_nodes"] // 2 and sum(x[0] == "A" for x in lines) == g["num_nodes"] // 2
    assert sum(x[0] == "L" for x in lines) == u["src"].numel() // 2 and all("\tSI:f:" in x for x in lines if x[0] == "L")
    # the error-free reads: one segment of 42 members on both strands and no link
    u = unitigs.compact_unitigs(overlapper.overlap_graph(sim[1], simplify={"fuzz": 0}, **KW))
    back = round_trip(u, tmp_path / "line.gfa")
    assert back["node_to_read"][0] == u["node_to_read"][0] and {s for _, s in back["node_to_read"][0]} == {"+", "-"}
    assert len(back["node_to_read"][1]) == 42 and back["node_to_read"][0][0][0].startswith("read") and back["src"].numel() == 0
    # cycles, a hairpin, a fork and a join, no similarities, default names; and the read graph itself, which has no chains
    ov = path([0, 2, 4, 6], closed=True) + path([8, 11, 12]) + [(12, 14, 300), (12, 16, 310), (14, 18, 320), (16, 18, 330), (18, 19, 340)]
    h = as_device(with_reads(gs.build(700 + np.arange(10), ov)))
    u = unitigs.compact_unitigs(h)
    back = round_trip(u, tmp_path / "hand.gfa")
    assert sorted(back["read_to_node"]) == ["utg000001c", "utg000002l", "utg000003l", "utg000004l", "utg000005l"]
    assert back["node_to_read"][0] == [("read0", "+"), ("read1", "+"), ("read2", "+"), ("read3", "+")]
    assert back["node_to_read"][2] == [("read4", "+"), ("read5", "-"), ("read6", "+")]
    text = (tmp_path / "hand.gfa").read_text()
    assert "A\tutg000002l\t0\t+\tread4\t0\t704\n" in text and f"A\tutg000002l\t{704 - 300}\t-\tread5\t0\t705\n" in text
    assert "L\tutg000001c\t-\tutg000001c\t-\t333M\n" in text and "L\tutg000005l\t+\tutg000005l\t-\t340M\n" in text
    back = round_trip(h, tmp_path / "reads.gfa")
    assert back["node_to_read"][3] == "read1" and back["read_to_node2"] == {}
    with pytest.raises(ValueError, match="parallel"):
        unitigs.write_gfa(as_device(with_reads(gs.build([1000] * 2, [(0, 2, 500), (0, 2, 400)]))), str(tmp_path / "no.gfa"))
    with pytest.raises(ValueError, match="reads"):
        unitigs.write_gfa({f: v for f, v in h.items() if f != "reads"}, str(tmp_path / "no.gfa"))


# ---- end to end -----------------------------------------------------------------------------------------------------------------

@gpu
def test_assemble_reads_to_fasta_on_unitigs_spells_the_covered_genome(sim, tmp_path):
    """The assertion of test_graph_simplify_device.py's pipeline test, decoded on the unitig graph."""
    genome, reads, strand, start, end = sim
    path_ = tmp_path / "reads.fasta"
    with open(path_, "w") as f:
        for i, (r, t, a, e) in enumerate(zip(reads, strand.tolist(), start.tolist(), end.tolist())):
            f.write(f">read_{i} strand={'+' if t == 1 else '-'} start={a} end={e} chr=1\n{r.decode()}\n")
    out = tmp_path / "asm.fasta"
    walks, contigs, stats, g = pipeline.assemble_reads_to_fasta(str(path_), None, str(out), len_threshold=1000, use_labels=True,
                                                                simplify={"fuzz": 0}, unitigs=True, **KW)
    covered = genome[int(start.min()):int(end.max())].decode()
    assert walks == [[0]] and len(contigs) == 1 and contigs.sequence(0) in (covered, st.revcomp(covered.encode()).decode())
    assert stats["longest_contig"] == len(covered) and out.read_text().count(">") == 1
    assert g["num_nodes"] == 2 and len(g["node_to_read"][0]) == 42 and g["node_to_read"][0][0][0].startswith("read_")
    assert g["y"].numel() == 0 and int(g["read_length"][0]) == len(covered)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

@gpu
def test_refusals():
    g = gs.build([1000] * 3, [(0, 2, 500), (2, 4, 500)])
    dev = as_device(g)
    one_missing = {f: (v[:-1] if torch.is_tensor(v) and v.numel() == 4 else v) for f, v in dev.items()}
    for fn in (unitigs.unitig_chains, unitigs.compact_unitigs):
        with pytest.raises(ValueError, match="mates"):
            fn(one_missing)
        with pytest.raises(ValueError, match="prefix_length"):
            fn(dict(dev, prefix_length=dev["prefix_length"] + 1))
        with pytest.raises(ValueError, match="overlap_length"):
            fn({f: v for f, v in dev.items() if f != "overlap_length"})
        with pytest.raises(ValueError, match="node ids"):
            fn(dict(dev, dst=dev["dst"] + 2))
    with pytest.raises(ValueError, match="unitigs"):
        overlapper.overlap_graph([b"ACGT" * 100], unitigs="yes")
