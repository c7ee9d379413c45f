"""Contig spelling (gnnome_amd/contigs.py, csrc/contig_spell.hip): walks -> sequences -> FASTA, N50 / NG50 (utils/evaluate.py:38-105).

The checker is evaluate.py:38-48 restated in plain Python (`spell_checker`, tests/contig_cases.py): reads[src][:prefix] for every step but the
last, the whole read for the last node, node 2r+1 the reverse complement of read r, prefixes under Python's slice rule."""
import ctypes
import gzip
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from contig_cases import _COMP, node_seq, spell_checker   # the statement: shared with test_contigs_adversarial.py
from gnnome_amd import _lib, contigs, gfa

# ---------------------------------------------------------------------------------------------------------------- CPU

def test_fasta_bytes_of_hand_made_contigs(tmp_path):
    """SeqIO.write(records, path, "fasta") (evaluate.py:51-53): '>id description', 60 columns, a final partial line."""
    seqs = ["A", "ACGTTGCAAC" * 5 + "ACGTTGCAA", "GATTACAGAT" * 6, "ccggaattNR" * 6 + "Y", "TTGACCAGTA" * 12]
    assert [len(s) for s in seqs] == [1, 59, 60, 61, 120]
    want = (">contig_1 length=1\nA\n"
            ">contig_2 length=59\nACGTTGCAACACGTTGCAACACGTTGCAACACGTTGCAACACGTTGCAACACGTTGCAA\n"
            ">contig_3 length=60\nGATTACAGATGATTACAGATGATTACAGATGATTACAGATGATTACAGATGATTACAGAT\n"
            ">contig_4 length=61\nccggaattNRccggaattNRccggaattNRccggaattNRccggaattNRccggaattNR\nY\n"
            ">contig_5 length=120\nTTGACCAGTATTGACCAGTATTGACCAGTATTGACCAGTATTGACCAGTATTGACCAGTA\n"
            "TTGACCAGTATTGACCAGTATTGACCAGTATTGACCAGTATTGACCAGTATTGACCAGTA\n")
    contigs.write_fasta(seqs, tmp_path / "a.fasta")
    assert (tmp_path / "a.fasta").read_bytes() == want.encode()
    records = [contigs.ContigRecord(f"contig_{i + 1}", f"length={len(s)}", s) for i, s in enumerate(seqs)]
    contigs.save_assembly(records, str(tmp_path), 3, suffix="_x")
    assert (tmp_path / "3_assembly_x.fasta").read_bytes() == want.encode()
    # FastaWriter's title rule: a description that starts with the id stands alone
    contigs.write_fasta([contigs.ContigRecord("r1", "r1 some read", "AC")], tmp_path / "b.fasta")
    assert (tmp_path / "b.fasta").read_text() == ">r1 some read\nAC\n"


def test_n50_and_ng50_by_hand():
    assert contigs.calculate_N50([10, 20, 30, 40]) == 30          # 40 + 30 = 70 >= 50
    assert contigs.calculate_N50([50, 50]) == 50                  # a tie: 50 >= 50
    assert contigs.calculate_N50([3, 3, 3]) == 3                  # 3 + 3 = 6 >= 4.5 (true division)
    assert contigs.calculate_N50([1, 2]) == 2                     # 2 >= 1.5
    assert contigs.calculate_N50([]) == -1
    assert contigs.calculate_NG50([10, 20, 30, 40], 200) == 10    # 40, 70, 90 < 100; 100 >= 100: the tie is in
    assert contigs.calculate_NG50([10, 20, 30, 40], 180) == 20    # 90 >= 90
    assert contigs.calculate_NG50([10, 20, 30, 40], 201) == -1    # 100 < 100.5 (true division)
    assert contigs.calculate_NG50([10, 20, 30, 40], 1000) == -1   # never reaches half the reference
    assert contigs.calculate_NG50([10, 20], 0) == -1 and contigs.calculate_NG50([10, 20], -5) == -1
    assert contigs.calculate_NG50([], 100) == -1
    recs = [contigs.ContigRecord("a", "", "A" * 7), contigs.ContigRecord("b", "", "C" * 5)]
    assert contigs.calculate_N50(recs) == 7 and contigs.calculate_N50(["AAAA", "CC", "G"]) == 4
    assert contigs.quick_evaluation([10, 20, 30, 40], 200) == (4, 40, 0.5, 30, 10)
    assert contigs.quick_evaluation([10, 20, 30, 40]) == (4, 40, -1, 30, -1)
    with pytest.raises(ValueError):
        contigs.quick_evaluation([])


def _write(path, text):
    if str(path).endswith("gz"):
        with gzip.open(path, "wt") as f:
            f.write(text)
    else:
        with open(path, "w") as f:
            f.write(text)


@pytest.mark.parametrize("name", ["r.fasta", "r.fa", "r.fna.gz", "r.fastq", "r.fq.gz", "r.fnq"])
def test_reads_file_parser(tmp_path, name):
    reads = {"read0": "ACGTACGTAC" * 13, "read1": "ggttNNRYac" * 7, "read2": "T"}
    if contigs.reads_file_type(name) == "fasta":   # multi-line records, a description, a record the GFA does not use
        text = (">read1 some description here\n" + "\n".join(reads["read1"][k:k + 30] for k in range(0, 70, 30)) + "\n"
                + ">unused\nAAAA\n>read0\n" + "\n".join(reads["read0"][k:k + 60] for k in range(0, 130, 60)) + "\n>read2 x\nT\n")
    else:                                          # FASTQ, one record wrapped over two sequence / quality lines
        text = (f"@read0 len=130\n{reads['read0'][:64]}\n{reads['read0'][64:]}\n+\n{'I' * 64}\n{'I' * 66}\n"
                f"@read1\n{reads['read1']}\n+read1\n{'#' * 70}\n@read2 desc\nT\n+\n@\n")
    path = tmp_path / name
    _write(path, text)
    got = contigs.read_sequences(str(path))
    assert {k: got[k].decode() for k in reads} == reads
    node_to_read = {2 * r + s: f"read{r}" for r in range(3) for s in range(2)}
    store = contigs.ReadStore.from_reads_file(str(path), node_to_read, 6, device=torch.device("cpu"))
    assert [store.sequence(2 * r) for r in range(3)] == [reads[f"read{r}"] for r in range(3)]
    assert store.sequence(3) == reads["read1"].translate(_COMP)[::-1]
    # only the reads the walks touch: zero-length slots for the rest
    part = contigs.ReadStore.from_reads_file(str(path), node_to_read, 6, keep=[1], device=torch.device("cpu"))
    assert part.sequence(2) == reads["read1"] and part.sequence(0) == "" and list(part.missing) == [True, False, True]
    node_to_read[4] = node_to_read[5] = "read9"
    with pytest.raises(KeyError, match="read9"):
        contigs.ReadStore.from_reads_file(str(path), node_to_read, 6, device=torch.device("cpu"))


def test_reads_file_errors(tmp_path):
    with pytest.raises(ValueError, match="suffix"):
        contigs.reads_file_type("reads.txt")
    g = gfa.read_gfa(os.path.join(GOLDEN, "g10_hifiasm8_utg.gfa"), similarity=None)
    path = tmp_path / "r.fasta"
    _write(path, ">read0\nACGT\n")
    with pytest.raises(ValueError, match="unitig"):          # the reference: TypeError on the list of (read, orientation)
        contigs.ReadStore.from_reads_file(str(path), g["node_to_read"], g["num_nodes"], device=torch.device("cpu"))
    assert contigs.gfa_sequences(os.path.join(GOLDEN, "g10_raven6.gfa")) is not None


def test_c_abi_argument_checks_without_a_gpu():
    lib = _lib.load()
    need = ctypes.c_size_t(0)
    assert lib.gnnome_contig_pieces_workspace_bytes(10, 100, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.gnnome_contig_pieces_workspace_bytes(-1, 100, ctypes.byref(need)) == -1
    one = ctypes.c_void_p(256)
    # zero walks: a no-op whatever the pointers
    assert lib.gnnome_contig_pieces(None, 0, None, 0, None, None, None, None, 10, None, 5, None, None, 0, None) == 0
    assert lib.gnnome_contig_spell(None, 0, None, 0, None, None, None, 5, None, 60, None, 0, None) == 0
    rc = lib.gnnome_contig_pieces(None, 4, one, 2, one, one, one, one, 10, one, 5, one, one, need.value, None)
    assert rc == -1 and b"null" in lib.gnnome_last_error()
    rc = lib.gnnome_contig_pieces(one, 4, one, 2, one, one, one, one, 10, one, 4, one, one, need.value, None)
    assert rc == -1 and b"read store" in lib.gnnome_last_error()
    rc = lib.gnnome_contig_pieces(one, 4, one, 2, one, one, one, one, 10, one, 5, one, one, 8, None)
    assert rc == -1 and b"workspace" in lib.gnnome_last_error()
    rc = lib.gnnome_contig_spell(one, 4, one, 2, one, None, one, 5, None, 0, one, 100, None)
    assert rc == -1 and b"null" in lib.gnnome_last_error()
    rc = lib.gnnome_contig_spell(one, 4, one, 2, one, one, one, 5, None, 60, one, 100, None)   # line_width > 0 needs body_off
    assert rc == -1 and b"null" in lib.gnnome_last_error()
    rc = lib.gnnome_contig_spell(one, 4, one, 2, one, one, one, 5, None, -1, one, 100, None)
    assert rc == -1 and b"line_width" in lib.gnnome_last_error()


# ---------------------------------------------------------------------------------------------------------------- GPU

def dev():
    return torch.device("cuda", 0)


def _random_walks(rng, succ, num_nodes, count, max_len):
    walks = []
    for k in range(count):
        u = int(rng.integers(num_nodes))
        if k % 5 == 0:
            u |= 1                                 # starts on an odd node
        w = [u]
        if k % 7 != 0:                             # every seventh walk is a single node
            for _ in range(int(rng.integers(1, max_len))):
                if not succ[w[-1]]:
                    break
                w.append(int(rng.choice(succ[w[-1]])))
        walks.append(w)
    return walks


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g10_hifiasm7.gfa", "g10_hifiasm8_utg.gfa", "g10_raven6.gfa"])
def test_kernel_against_the_restatement(tmp_path, name):
    from gnnome_amd.decode import DecodeGraph
    path = os.path.join(GOLDEN, name)
    g = gfa.read_gfa(path, similarity=None)
    seqs = [s.decode() for s in contigs.gfa_sequences(path)]
    n = g["num_nodes"]
    rng = np.random.default_rng(len(name))
    src, dst = g["src"].tolist(), g["dst"].tolist()
    # parallel edges: repeat a third of the pairs with other prefixes (the last id of a pair wins, graph_parser.py:77-80)
    rep = rng.choice(len(src), size=len(src) // 3, replace=False)
    src, dst = src + [src[i] for i in rep], dst + [dst[i] for i in rep]
    rl = [len(seqs[u >> 1]) for u in range(n)]
    # prefixes beyond the read and negative ones, under Python's slice rule
    prefix = [int(rng.integers(-rl[u] - 5, rl[u] + 6)) for u in src]
    dg = DecodeGraph(src, dst, n, prefix, g["read_length"], device=dev())
    succ = [[] for _ in range(n)]
    for u, v in zip(src, dst):
        succ[u].append(v)
    walks = _random_walks(rng, succ, n, 60, 25)
    assert any(len(w) == 1 for w in walks) and any(w[0] % 2 for w in walks)
    want = spell_checker(walks, src, dst, prefix, seqs)
    store = contigs.ReadStore.from_gfa(path, device=dev())
    c0 = contigs.spell_contigs(dg, walks, store)
    assert [c0.sequence(i) for i in range(len(walks))] == want
    assert c0.lengths.cpu().tolist() == [len(s) for s in want]
    assert [(r.id, r.description, r.seq) for r in c0.records()] == [(f"contig_{i + 1}", f"length={len(s)}", s) for i, s in enumerate(want)]
    for lw in (7, 60):
        c = contigs.spell_contigs(dg, walks, store, line_width=lw)
        assert [c.sequence(i) for i in range(len(walks))] == want
        contigs.write_fasta(want, tmp_path / "host.fasta", line_width=lw)
        assert c.fasta_bytes().tobytes() == (tmp_path / "host.fasta").read_bytes()
        assert c0.respell(lw).fasta_bytes().tobytes() == (tmp_path / "host.fasta").read_bytes()
    # the drop-in entry: a dict of node -> sequence (both strands, as graph_parser.py:365 builds it)
    reads = {u: node_seq(seqs, u) for u in range(n)}
    c1 = contigs.walk_to_sequence(walks, dg, reads, edges=None)
    assert [r.seq for r in c1] == want


def _genome(rng, size):
    g = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=size)
    for _ in range(200):                                    # lowercase stretches
        a = int(rng.integers(size - 5000))
        g[a:a + int(rng.integers(10, 5000))] |= 32
    for sym in b"NRY":                                      # IUPAC letters
        g[rng.choice(size, size=2000, replace=False)] = sym
    return g.tobytes().decode()


@pytest.mark.gpu
def test_gfa_to_fasta_end_to_end(tmp_path):
    from gnnome_amd import pipeline
    rng = np.random.default_rng(7)
    genome = _genome(rng, 5_200_000)
    start = np.cumsum(rng.integers(2000, 4000, size=2000))
    length = rng.integers(9000, 15000, size=2000)
    keep = start + length <= len(genome)
    start, length = start[keep], length[keep]
    reads = len(start)
    flip = rng.random(reads) < 0.3                          # a third of the reads are stored as their reverse complement
    fq, gf = tmp_path / "reads.fastq", tmp_path / "layout.gfa"
    with open(fq, "w") as f:
        for r in range(reads):
            s = genome[start[r]:start[r] + length[r]]
            s = s.translate(_COMP)[::-1] if flip[r] else s
            f.write(f"@read{r} pos={start[r]}\n{s}\n+\n{'I' * len(s)}\n")
    with open(gf, "w") as f:
        for r in range(reads):
            f.write(f"S\tread{r}\t*\tLN:i:{length[r]}\n")
        for r in range(reads):
            for t in range(r + 1, reads):
                ol = start[r] + length[r] - start[t]
                if ol <= 500:
                    break
                if start[t] + length[t] <= start[r] + length[r]:
                    continue
                o1, o2 = "-" if flip[r] else "+", "-" if flip[t] else "+"
                f.write(f"L\tread{r}\t{o1}\tread{t}\t{o2}\t{int(ol)}M\tSI:f:0.999\n")
    g = gfa.read_gfa(str(gf))
    src, dst = g["src"], g["dst"]
    hop = ((dst >> 1) - (src >> 1)).abs().float()          # test_gfa_and_mask.py:228-231, strand-blind for the flipped reads
    ideal = 10.0 - 2.0 * hop
    out = tmp_path / "asm.fasta"
    with pytest.raises(ValueError, match="no read sequences"):
        pipeline.assemble_to_fasta(str(gf), None, str(out), len_threshold=20_000, device=dev(), scores=ideal)
    torch.manual_seed(1)
    walks, ctg, stats = pipeline.assemble_to_fasta(str(gf), None, str(out), len_threshold=20_000, reads=str(fq), nb_paths=20,
                                                   device=dev(), scores=ideal, ref_length=len(genome))
    assert len(walks) == len(ctg) >= 1 and stats["num_contigs"] == len(walks)
    best = int(np.argmax(ctg.lengths_host()))
    rd = [v >> 1 for v in walks[best]]
    a, b = int(start[min(rd)]), int(max(start[r] + length[r] for r in rd))
    seq = ctg.sequence(best)
    assert seq == genome[a:b] or seq == genome[a:b].translate(_COMP)[::-1]
    assert b - a >= 0.9 * len(genome)
    # every spelled length is decode's contig length (get_contig_length, inference.py:29-36): LN is the true length here
    edges = {(u, v): i for i, (u, v) in enumerate(zip(src.tolist(), dst.tolist()))}
    pre, rlen = g["prefix_length"].tolist(), g["read_length"].tolist()
    dec = [sum(pre[edges[(x, y)]] for x, y in zip(w[:-1], w[1:])) + rlen[w[-1]] for w in walks]
    assert ctg.lengths_host().tolist() == dec
    assert stats["longest_contig"] == max(dec) and stats["n50"] == contigs.calculate_N50(dec)
    assert stats["ng50"] == contigs.calculate_NG50(dec, len(genome))
    back = contigs.read_sequences(str(out))
    assert [back[f"contig_{i + 1}"].decode() for i in range(len(ctg))] == [ctg.sequence(i) for i in range(len(ctg))]
    assert out.read_text().startswith(f">contig_1 length={dec[0]}\n")


@pytest.mark.gpu
def test_output_beyond_2_31_bytes():
    """A synthetic assembly of 2.3 GB (int64 offsets in every layer), checked piece by piece on the device against an independent
    torch restatement: searchsorted over the piece offsets, a gather from the store, the complement table for odd nodes."""
    from gnnome_amd.decode import DecodeGraph
    from gnnome_amd.overlap import COMPLEMENT
    R, L = 64, 1 << 20
    rng = np.random.default_rng(5)
    data = torch.from_numpy(rng.choice(np.frombuffer(b"ACGTNacgtRY", dtype=np.uint8), size=R * L))
    off = torch.arange(R + 1, dtype=torch.int64) * L
    store = contigs.ReadStore(data.to(dev()), off.to(dev()))
    n = 2 * R
    src = [u for u in range(n) for d in (2, 4, 7)]          # every node to three others, both parities
    dst = [(u + d) % n for u in range(n) for d in (2, 4, 7)]
    prefix = [int(x) for x in rng.integers(L // 2, L + 1000, size=len(src))]
    dg = DecodeGraph(src, dst, n, prefix, [L] * n, device=dev())
    succ = [[] for _ in range(n)]
    for u, v in zip(src, dst):
        succ[u].append(v)
    walks = []
    for k in range(3):
        w = [int(rng.integers(n))]
        for _ in range(1300):
            w.append(int(rng.choice(succ[w[-1]])))
        walks.append(w)
    c = contigs.spell_contigs(dg, walks, store)
    total = int(c.offsets[-1])
    assert total > 2 ** 31 + 2 ** 26
    pre = {(u, v): min(p, L) for u, v, p in zip(src, dst, prefix)}     # no parallel pairs here; 0 <= prefix
    piece_len = []
    for w in walks:
        piece_len += [pre[(a, b)] for a, b in zip(w[:-1], w[1:])] + [L]
    assert c.lengths_host().tolist() == [sum(pre[(a, b)] for a, b in zip(w[:-1], w[1:])) + L for w in walks]
    nodes = torch.tensor([v for w in walks for v in w], dtype=torch.int64, device=dev())
    po = torch.zeros(len(piece_len) + 1, dtype=torch.int64)
    po[1:] = torch.cumsum(torch.tensor(piece_len, dtype=torch.int64), 0)
    po = po.to(dev())
    comp = torch.from_numpy(COMPLEMENT.astype(np.int64)).to(dev())
    reads_d, roff = store.data, store.off
    chunk = 1 << 27
    for a in range(0, total, chunk):
        p = torch.arange(a, min(a + chunk, total), dtype=torch.int64, device=dev())
        s = torch.searchsorted(po, p, right=True) - 1
        k = p - po[s]
        u = nodes[s]
        r = u >> 1
        odd = (u & 1).bool()
        idx = torch.where(odd, roff[r + 1] - 1 - k, roff[r] + k)
        b = reads_d[idx].long()
        b = torch.where(odd, comp[b], b)
        assert torch.equal(c.data[a:a + p.numel()].long(), b), f"bytes [{a}, {a + p.numel()}) differ"


@pytest.mark.gpu
def test_errors_name_the_walk_and_the_pair():
    from gnnome_amd.decode import DecodeGraph
    path = os.path.join(GOLDEN, "g10_raven6.gfa")
    g = gfa.read_gfa(path, similarity=None)
    dg = DecodeGraph(g["src"], g["dst"], g["num_nodes"], g["prefix_length"], g["read_length"], device=dev())
    store = contigs.ReadStore.from_gfa(path, device=dev())
    src, dst = g["src"].tolist(), g["dst"].tolist()
    pairs = set(zip(src, dst))
    u, v = src[0], dst[0]
    x = next(y for y in range(g["num_nodes"]) if (v, y) not in pairs and y != v)
    with pytest.raises(_lib.GnnomeHipError, match=rf"walk 1: \({v}, {x}\) is not an edge"):
        contigs.spell_contigs(dg, [[u, v], [u, v, x]], store)
    n = g["num_nodes"]
    with pytest.raises(_lib.GnnomeHipError, match=rf"walk 2: pair \({u}, {n + 3}\) has a node outside \[0, {n}\)"):
        contigs.spell_contigs(dg, [[u], [v], [u, n + 3]], store)
    with pytest.raises(_lib.GnnomeHipError, match=r"walk 0: node -1 outside"):
        contigs.spell_contigs(dg, [[-1]], store)
    with pytest.raises(_lib.GnnomeHipError, match="walk 1 is empty"):
        contigs.spell_contigs(dg, [[u, v], []], store)
    assert len(contigs.spell_contigs(dg, [], store)) == 0


@pytest.mark.gpu
def test_two_runs_give_identical_bytes():
    from gnnome_amd.decode import DecodeGraph
    path = os.path.join(GOLDEN, "g10_hifiasm7.gfa")
    g = gfa.read_gfa(path, similarity=None)
    dg = DecodeGraph(g["src"], g["dst"], g["num_nodes"], g["prefix_length"], g["read_length"], device=dev())
    store = contigs.ReadStore.from_gfa(path, device=dev())
    succ = [[] for _ in range(g["num_nodes"])]
    for a, b in zip(g["src"].tolist(), g["dst"].tolist()):
        succ[a].append(b)
    walks = _random_walks(np.random.default_rng(3), succ, g["num_nodes"], 400, 40)
    one = contigs.spell_contigs(dg, walks, store, line_width=60).data
    two = contigs.spell_contigs(dg, walks, store, line_width=60).data
    assert one.numel() > 0 and torch.equal(one, two)
