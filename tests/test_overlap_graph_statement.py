"""tests/overlap_graph_statement.py on error-free reads of a random genome against what the read positions alone say.  The genome (fixed
seed) has no 15-mer that occurs twice, on either strand - asserted below - so every shared minimizer is a true one and the comparison is
exact, not statistical: the dovetail edges, their overlap lengths and the containment flags.  No GPU."""
import numpy as np
import pytest

import overlap_graph_statement as st

K, W, MIN_OVERLAP, MAX_OCC = 15, 5, 300, 64


@pytest.fixture(scope="module")
def sim():
    genome, reads, strand, start, end = st.simulate()
    ov = st.overlaps(reads, k=K, w=W, max_occ=MAX_OCC, min_overlap=MIN_OVERLAP)
    return genome, reads, strand, start, end, ov


def test_the_genome_has_no_repeated_kmer(sim):
    genome, reads = sim[0], sim[1]
    assert len(genome) == 20000 and st.canonical_kmers_unique(genome, K)
    assert 100 <= len(reads) <= 140 and min(map(len, reads)) >= 300 and max(map(len, reads)) <= 2500
    assert {-1, 1} == set(sim[2].tolist())


def test_hash_is_a_bijection_on_2k_bits():
    x = np.arange(1 << 10, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = st.mix(x, 5)
    assert sorted(h.tolist()) == x.tolist() and h.tolist() != x.tolist()


def test_sketch_follows_the_window_rule_on_a_small_read():
    seq = b"ACGTTGCAAGGCTTACCGATNACGGTCATTGACCA"
    k, w = 5, 4
    sk = st.sketch([seq], k, w)
    h, strand = st.kmer_hashes(np.frombuffer(seq, dtype=np.uint8), k)
    want = set()
    for s in range(len(h) - w + 1):
        win = [(int(h[p]), p) for p in range(s, s + w) if h[p] != st.INVALID]
        if win:
            want.add(min(win)[1])
    assert sk["pos"].tolist() == sorted(want) and sk["off"].tolist() == [0, len(want)]
    assert sk["strand"].tolist() == [int(strand[p]) for p in sorted(want)]
    n_at = seq.index(b"N")
    assert all(h[p] == st.INVALID for p in range(n_at - k + 1, n_at + 1))
    assert st.sketch([seq[:k + w - 2]], k, w)["pos"].size == 0 and st.sketch([seq[:k + w - 1]], k, w)["pos"].size >= 1


def test_dovetail_edges_and_overlap_lengths_equal_the_positional_truth(sim):
    _, _, strand, start, end, ov = sim
    truth, _ = st.positional_truth(strand, start, end, MIN_OVERLAP)
    g = st.graph(ov, drop_contained=False)
    got = {(u, v): ol for u, v, ol in zip(g["src"].tolist(), g["dst"].tolist(), g["overlap_length"].tolist())}
    assert len(got) == len(g["src"]) and len(truth) > 200
    assert set(got) == set(truth)
    assert got == truth
    assert (g["prefix_length"] == g["read_length"][g["src"]] - g["overlap_length"]).all()
    for (u, v), ol in got.items():
        assert got[(v ^ 1, u ^ 1)] == ol


def test_containment_flags_equal_the_positional_truth(sim):
    _, _, strand, start, end, ov = sim
    _, contained = st.positional_truth(strand, start, end, MIN_OVERLAP)
    assert 0 < contained.sum() < len(contained)
    assert ov["contained"].tolist() == contained.tolist()


def test_dropping_contained_reads_keeps_the_rest_connected(sim):
    _, _, strand, start, end, ov = sim
    g = st.graph(ov, drop_contained=True)
    touched = set(g["src"].tolist()) | set(g["dst"].tolist())
    assert not any(ov["contained"][v >> 1] for v in touched)
    # the reads that are left chain into one piece per strand: what the pipeline test spells
    alive = [r for r in range(len(start)) if not ov["contained"][r]]
    parent = {2 * r + s: 2 * r + s for r in alive for s in (0, 1)}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in zip(g["src"].tolist(), g["dst"].tolist()):
        parent[find(u)] = find(v)
    assert len({find(x) for x in parent}) == 2


def test_max_pairs_below_the_exact_count_raises(sim):
    reads, ov = sim[1], sim[5]
    P = len(ov["records"])
    assert st.pair_count(ov["sketch"], MAX_OCC) == P
    with pytest.raises(ValueError, match="max_pairs"):
        st.overlaps(reads, k=K, w=W, max_occ=MAX_OCC, min_overlap=MIN_OVERLAP, max_pairs=P - 1)
