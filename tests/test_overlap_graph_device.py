"""gnnome_amd.overlapper (csrc/overlap_graph.hip) against tests/overlap_graph_statement.py, stage by stage and bit for bit: the sketch
arrays, the seed-pair records, the Overlaps fields and the graph dict.  Everything is an integer, so every comparison is exact; the one
float, overlap_similarity, is compared with 1.0 on error-free reads, where the edit distance is 0 and 1 - 0 / ol is exact."""
import numpy as np
import pytest
import torch

import overlap_graph_statement as st
from gnnome_amd import _lib, labels, overlapper, pipeline

gpu = pytest.mark.gpu
K, W, MIN_OVERLAP, MAX_OCC = 15, 5, 300, 64
KW = dict(k=K, w=W, max_occ=MAX_OCC, min_overlap=MIN_OVERLAP)


def check(reads, drop_contained=True, similarity=False, **kw):
    """Every stage of the device result on `reads` equals the statement -> (graph dict, statement overlaps)."""
    want = st.overlaps(reads, **kw)
    k, w = kw.get("k", 19), kw.get("w", 10)
    sk = overlapper.sketch_reads(reads, k, w)
    assert sk.hash.dtype == torch.uint64 and sk.read.dtype == sk.pos.dtype == torch.int32 and sk.strand.dtype == torch.uint8 and sk.hash.is_cuda
    assert np.array_equal(sk.hash.cpu().numpy(), want["sketch"]["hash"])
    for f in ("read", "pos", "strand", "off"):
        assert np.array_equal(getattr(sk, f).cpu().numpy(), want["sketch"][f]), f
    g = overlapper.overlap_graph(reads, sk, drop_contained=drop_contained, similarity=similarity,
                                 **{a: b for a, b in kw.items() if a not in ("k", "w")})
    ov = g["overlaps"]
    assert np.array_equal(ov.record_fields().cpu().numpy(), want["records"])
    for f in st.FIELDS:
        assert getattr(ov, f).dtype == torch.int32 and np.array_equal(getattr(ov, f).cpu().numpy(), want[f]), f
    assert np.array_equal(g["contained"].cpu().numpy(), want["contained"])
    wg = st.graph(want, drop_contained=drop_contained)
    assert g["num_nodes"] == wg["num_nodes"] == 2 * len(reads)
    for f in ("src", "dst", "overlap_length", "prefix_length", "read_length"):
        assert g[f].dtype == torch.int64 and np.array_equal(g[f].cpu().numpy(), wg[f]), f
    return g, want


def mutate(reads, seed, sub=0.01, indel=0.005):
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


def random_seq(seed, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)])


@pytest.fixture(scope="module")
def sim():
    return st.simulate()


def annotations(strand, start, end):
    node = lambda x, flip=False: torch.from_numpy(np.stack([x, -x if flip else x], 1).reshape(-1).astype(np.int64))   # noqa: E731
    return [node(strand, True), node(start), node(end), torch.ones(2 * len(start), dtype=torch.int64)]


# ---- (a), (b): the simulated read set -------------------------------------------------------------------------------------------

@gpu
def test_error_free_reads_every_stage_similarity_and_labels(sim):
    genome, reads, strand, start, end = sim
    check(reads, drop_contained=False, **KW)
    g, want = check(reads, similarity=False, **KW)
    g = overlapper.overlap_graph(reads, annotations=annotations(strand, start, end), **KW)
    assert g["src"].numel() > 100 and bool((g["overlap_similarity"] == 1.0).all())
    truth, _ = st.positional_truth(strand, start, end, MIN_OVERLAP)
    assert {(u, v) for u, v in zip(g["src"].tolist(), g["dst"].tolist())} <= set(truth)
    ids, y = labels.process_graph(g)
    s = g["read_strand"]
    assert bool((s[g["src"].cpu()] == s[g["dst"].cpu()]).all())     # every edge joins same-strand reads that overlap on the reference ...
    assert bool((y.cpu() == 1).all()) and ids.numel() == g["src"].numel()   # ... and every one of them is labelled 1


@gpu
def test_reads_with_substitutions_and_indels(sim):
    noisy = mutate(sim[1], seed=3)
    assert sum(x != y for x, y in zip(noisy, sim[1])) > 100
    g, want = check(noisy, **KW)
    assert len(want["a"]) > 100 and g["src"].numel() > 100
    assert len(set(want["d_beg"] - want["d_end"])) > 3      # the indels move the diagonal inside a band


# ---- (c): edge reads ------------------------------------------------------------------------------------------------------------

@gpu
def test_edge_reads():
    k, w = 15, 5
    base = random_seq(11, 700)
    with_n = bytearray(random_seq(12, 400))
    with_n[::10] = b"N" * len(with_n[::10])
    clean = random_seq(14, 600)
    few_n = bytearray(clean)
    n_at = (100, 101, 300, 450)
    for p in n_at:                                                    # isolated Ns: valid and invalid k-mers mix in one run and one window
        few_n[p] = ord("N")
    reads = [base[:k - 1], base[:k], base[:k + w - 2], base[:k + w - 1], bytes(with_n), base.lower(), b"A" * 300, base, base[100:700],
             st.revcomp(base[50:650]), random_seq(13, 400), b"ACGTACGTAC" * 30, base, st.revcomp(base), bytes(few_n), clean[50:550]]
    g, want = check(reads, k=k, w=w, min_overlap=100, max_occ=64)
    off = want["sketch"]["off"]
    assert (off[1:4] == off[0:3]).all() and off[4] == off[3] + 1     # k - 1, k, k + w - 2: nothing; k + w - 1: its one window
    assert off[5] == off[4]                                           # an N every 10 bases leaves no valid k-mer
    assert off[7] - off[6] == 300 - k - w + 2                         # a homopolymer: every window's leftmost k-mer (all hashes tie)
    assert np.array_equal(want["sketch"]["pos"][off[5]:off[6]], want["sketch"]["pos"][off[7]:off[8]])   # lower case = upper case
    by_pair = {(a, b, r): kd for a, b, r, kd in zip(*(want[f].tolist() for f in ("a", "b", "rel", "kind")))}
    assert by_pair[(5, 7, 0)] == 1 and by_pair[(7, 12, 0)] == 1       # two identical reads (lower case, byte for byte): the later one is contained
    assert by_pair[(7, 9, 1)] == 1 and by_pair[(7, 8, 0)] == 1        # a reverse-complemented piece, and a plain one
    tie = {f: want[f][[i for i, key in enumerate(by_pair) if key == (7, 13, 1)][0]] for f in ("kind", "d_beg", "d_end")}
    assert tie == {"kind": 1, "d_beg": 0, "d_end": 0}                 # a read equal to another's reverse complement: b is the contained one
    assert by_pair[(12, 13, 1)] == 1 and (7, 13, 0) not in by_pair
    pos_n = want["sketch"]["pos"][off[14]:off[15]]
    assert len(pos_n) > 50 and not any(p <= x < p + k for p in pos_n.tolist() for x in n_at)   # no minimizer over an N ...
    assert any(x - k - w < p < x for p in pos_n.tolist() for x in n_at) and by_pair[(14, 15, 0)] == 1   # ... some right beside one


@gpu
def test_lowest_hash_on_the_tile_edge():
    k, w = 15, 5
    T = overlapper.sketch_tile_size()
    seq = bytearray(random_seq(21, 2 * T + 3))
    h = st.kmer_hashes(np.frombuffer(bytes(seq), dtype=np.uint8), k)[0]
    # move the read's smallest hash to the k-mer start T - 1 + w - 1: the last position of window T - 1 (the last of tile 0) and of no
    # earlier one, and a position of the first w - 1 windows of tile 1, which must not emit it again
    src, dst = int(np.argmin(h)), T + w - 2
    seq[dst:dst + k] = seq[src:src + k]
    seq = bytes(seq)
    h = st.kmer_hashes(np.frombuffer(seq, dtype=np.uint8), k)[0]
    assert h[dst] == h.min()
    g, want = check([seq, seq[T - 500:T + 500]], k=k, w=w, min_overlap=100, max_occ=64)
    pos = want["sketch"]["pos"][:want["sketch"]["off"][1]].tolist()
    assert pos.count(dst) == 1 and len(pos) == len(set(pos)) and pos == sorted(pos)


# ---- (d): max_occ ---------------------------------------------------------------------------------------------------------------

@gpu
def test_a_hash_with_exactly_max_occ_seeds_and_one_with_one_more():
    k, w, max_occ = 15, 1, 8
    kept, dropped = random_seq(31, k), random_seq(32, k)
    reads = [random_seq(100 + i, 40) + (kept if i < max_occ else b"") + random_seq(200 + i, 40) + dropped + random_seq(300 + i, 40)
             for i in range(max_occ + 1)]
    g, want = check(reads, k=k, w=w, max_occ=max_occ, min_seeds=1, min_overlap=0, max_hang=10 ** 6)
    hk, hd = (int(st.kmer_hashes(np.frombuffer(x, dtype=np.uint8), k)[0][0]) for x in (kept, dropped))
    count = lambda hv: int((want["sketch"]["hash"] == np.uint64(hv)).sum())   # noqa: E731
    assert count(hk) == max_occ and count(hd) == max_occ + 1
    a, b, rel, d, pa = want["records"].T                             # the kept k-mer starts at 40; the dropped one at 95, or at 80 in the last read
    assert int(((pa == 40) & (d == 0) & (rel == 0)).sum()) == max_occ * (max_occ - 1) // 2
    assert not ((pa == 95) & ((d == 0) | (d == 15))).any()


# ---- (e), (f): the chain kernel's carry and ties --------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("shared", (100, 5000))
def test_a_group_longer_than_one_pass(shared):
    k = 15
    common = random_seq(41, shared + k - 1)
    reads = [random_seq(42, 700) + common, common + random_seq(43, 900)]
    g, want = check(reads, k=k, w=1, min_overlap=50, max_occ=64)
    assert len(want["records"]) >= shared and (shared < 4096 or len(want["records"]) > 4096) and len(want["records"]) > 64
    assert want["kind"].tolist() == [3] and want["n_seeds"][0] >= shared and want["overlap_length"][0] == shared + k - 1
    noisy = mutate(reads, seed=5, sub=0.0, indel=0.004)            # several bands: the open band and the best one cross the passes
    g, want = check(noisy, k=k, w=1, band=2, min_overlap=50, max_occ=64, max_hang=10 ** 6)
    assert len(want["records"]) > 64


@gpu
def test_two_bands_of_equal_seed_count_keep_the_first():
    k = 15
    piece = random_seq(51, 60)
    # the bases around the three copies differ, so no shared k-mer reaches beyond the piece
    reads = [random_seq(52, 49) + b"A" + piece + b"A" + random_seq(53, 698) + b"C" + piece + b"C" + random_seq(54, 49),
             random_seq(55, 299) + b"G" + piece + b"G" + random_seq(56, 299)]
    g, want = check(reads, k=k, w=1, band=10, min_seeds=3, min_overlap=0, max_hang=10 ** 6)
    rec = want["records"]
    d = sorted(set(rec[:, 3].tolist()))
    assert len(d) == 2 and d[1] - d[0] > 10 and (rec[:, 3] == d[0]).sum() == (rec[:, 3] == d[1]).sum() == 60 - k + 1
    assert want["d_beg"].tolist() == [d[0]] and want["n_seeds"].tolist() == [60 - k + 1]


# ---- (g), (h) -------------------------------------------------------------------------------------------------------------------

@gpu
def test_max_pairs_one_below_the_exact_count_raises_before_writing(sim, monkeypatch):
    """The record pass of gnnome_seed_pairs is the call with key_ab set; the count pass (key_ab NULL) writes to its workspace only."""
    lib = _lib.load()
    entry, record_passes = lib.gnnome_seed_pairs, []

    def spy(*args):
        record_passes.append(getattr(args[9], "value", args[9]) is not None)   # key_ab: None or a c_void_p
        return entry(*args)

    monkeypatch.setattr(lib, "gnnome_seed_pairs", spy)
    reads = sim[1][:30]
    ov = overlapper.find_overlaps(reads, **KW)
    P = int(ov.records[0].numel())
    assert P == st.pair_count(st.sketch(reads, K, W), MAX_OCC) and P > 1000
    assert int(overlapper.find_overlaps(reads, max_pairs=P, **KW).records[0].numel()) == P
    assert record_passes == [False, True, False, True]
    del record_passes[:]
    with pytest.raises(ValueError, match="max_occ.*max_pairs"):
        overlapper.find_overlaps(reads, max_pairs=P - 1, **KW)
    assert record_passes == [False]                                   # counted, refused, and no record pass was launched


@gpu
def test_two_launches_give_equal_bytes(sim):
    reads = mutate(sim[1], seed=9)
    runs = [overlapper.overlap_graph(reads, similarity=False, **KW) for _ in range(2)]
    for x, y in zip(*[[g["overlaps"].sketch.hash.view(torch.int64), g["overlaps"].sketch.pos, *g["overlaps"].records, g["src"], g["dst"],
                       g["overlap_length"], g["overlaps"].d_beg, g["overlaps"].d_end, g["overlaps"].n_seeds] for g in runs]):
        assert torch.equal(x, y)


# ---- (i): reads file to FASTA ---------------------------------------------------------------------------------------------------

@gpu
def test_assemble_reads_to_fasta_spells_the_covered_genome(sim, tmp_path):
    """With the labels as scores every walk follows true overlaps, and the reads that are left after the contained ones are dropped chain
    into one piece (tests/test_overlap_graph_statement.py), so the first - longest - contig reaches from the leftmost to the rightmost
    read: the covered genome, on the strand the walk happened to take.  A walk marks its reverse complement visited, so the other strand
    is not spelled again; whatever else is spelled comes from reads the greedy walk skipped and is a piece of the genome as well."""
    genome, reads, strand, start, end = sim
    path = tmp_path / "reads.fasta"
    with open(path, "w") as f:
        for i, (r, t, a, e) in enumerate(zip(reads, strand.tolist(), start.tolist(), end.tolist())):
            f.write(f">read_{i} strand={'+' if t == 1 else '-'} start={a} end={e} chr=1\n{r.decode()}\n")
    out = tmp_path / "asm.fasta"
    walks, contigs, stats, g = pipeline.assemble_reads_to_fasta(str(path), None, str(out), len_threshold=1000, use_labels=True, **KW)
    covered = genome[int(start.min()):int(end.max())].decode()
    both = (genome.decode(), st.revcomp(genome).decode())
    assert len(contigs) >= 1 and contigs.sequence(0) in (covered, st.revcomp(covered.encode()).decode())
    assert all(any(contigs.sequence(i) in s for s in both) for i in range(len(contigs)))
    assert stats["longest_contig"] == len(covered) and out.read_text().count(">") == len(contigs)
