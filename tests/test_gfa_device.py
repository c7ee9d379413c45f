"""The device GFA parser (csrc/gfa_parse.hip, gfa.read_gfa_device) against the host parser gfa.read_gfa, which golden G10 holds to the
reference's only_from_gfa: every tensor with torch.equal, every dict with ==, no key left out."""
import builtins
import gzip
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gfa_statement import adversarial_gfa
from gnnome_amd import gfa

pytestmark = pytest.mark.gpu

GOLDEN_GFAS = ("g10_hifiasm8_utg.gfa", "g10_hifiasm7.gfa", "g10_raven6.gfa", "g14_single.gfa", "g14_multi.gfa", "g14_utg_x.gfa")
G14_READS = {"g14_single.gfa": "g14_single.fasta", "g14_multi.gfa": "g14_multi.fasta", "g14_utg_x.gfa": "g14_utg_x.fastq.gz"}


def dev():
    return torch.device("cuda", 0)


def _same(got, want):
    assert got.keys() == want.keys()
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert torch.is_tensor(g) and g.dtype == w.dtype and g.device == w.device and torch.equal(g, w), k
        else:
            assert type(g) is type(w) and g == w, k


def _outcome(fn):
    try:
        return fn()
    except Exception as ex:   # noqa: BLE001 (the outcome IS the exception)
        return (type(ex), str(ex))


def _write(path, text):
    path.write_bytes(text if isinstance(text, bytes) else text.encode("ascii"))
    return str(path)


def _both(path, **kw):
    want = gfa.read_gfa(path, parser="host", **kw)
    _same(gfa.read_gfa(path, parser="device", **kw), want)
    _same(gfa.read_gfa(path, parser="auto", **kw), want)
    return want


@pytest.mark.parametrize("name", GOLDEN_GFAS)
def test_goldens_key_for_key(name):
    path = os.path.join(GOLDEN, name)
    _both(path, similarity=None)
    if name.startswith("g10"):      # sequences as long as their LN says: the aligner serves the overlaps
        want = _both(path, similarity="auto", keep_sequences=True)
        assert want["overlap_similarity"] is not None and want["src"].numel() > 0
    else:
        _both(path, similarity=None, keep_sequences=True)
    if name in G14_READS:
        got = _both(path, similarity=None, training=True, reads_path=os.path.join(GOLDEN, G14_READS[name]))
        assert got["y"] is not None and got["read_start"].numel() == got["num_nodes"]


@pytest.mark.parametrize("seed", range(30))
def test_adversarial_text(tmp_path, seed):
    tags, sequences = ("all", "all_but_one", "none")[seed % 3], seed % 2 == 0
    path = _write(tmp_path / "adv.gfa", adversarial_gfa(seed, tags=tags, sequences=sequences))
    want = _both(path, similarity="auto", keep_sequences=sequences)
    assert want["src"].numel() > 0
    if tags == "all" or sequences:
        assert want["overlap_similarity"] is not None    # the tags decide, or the aligner takes over
    if tags == "none" and not sequences:
        assert want["overlap_similarity"] is None
    g = gfa.read_gfa_device(path, similarity=None, keep_names=False)
    assert g["read_to_node"] is None and g["node_to_read"] is None and g["read_to_node2"] is None
    assert all(t.device == dev() for t in g.values() if torch.is_tensor(t)) and torch.equal(g["src"].cpu(), want["src"])
    assert (g["reads"] is None) == (not sequences)


def _reads_equal(path):
    from gnnome_amd.overlap import pack_reads
    want = gfa.read_gfa(path, similarity=None, keep_sequences=True)
    _same(gfa.read_gfa(path, similarity=None, keep_sequences=True, parser="device"), want)
    data, off = pack_reads([want["read_seqs"][2 * r] for r in range(want["num_nodes"] // 2)])
    g = gfa.read_gfa_device(path, similarity=None)
    assert g["reads"][0].device == dev() and g["reads"][0].dtype == torch.uint8 and g["reads"][1].dtype == torch.int64
    assert torch.equal(g["reads"][0].cpu(), data) and torch.equal(g["reads"][1].cpu(), off)


def test_tile_borders(tmp_path):
    """A sequence end, the field start behind it and the next line start on, one before and one after a multiple of each kernel's tile
    (and every offset in between: the first sequence's length walks across the border)."""
    rng = np.random.default_rng(5)
    for tile in (gfa.TOKENISE_TILE, gfa.PACK_TILE, 2 * gfa.TOKENISE_TILE):
        for q in range(tile - 18, tile + 3):
            seq = "".join("ACGT"[c] for c in rng.integers(0, 4, size=q))
            text = (f"S\ta\t{seq}\tLN:i:{q}\nS\tb\tACGTTGCAAC\tLN:i:10\n\nS\tc\t{seq[:37]}\tLN:i:37\n"
                    f"L\ta\t+\tb\t-\t5M\nL\tb\t+\tc\t+\t7M\nL\tc\t-\ta\t+\t{min(q, 30)}M")
            _reads_equal(_write(tmp_path / "border.gfa", text))


def test_one_long_sequence_among_short_ones(tmp_path):
    rng = np.random.default_rng(6)
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, size=n)) for n in (40, 70_001, 1, 55, 16, 15, 17)]
    text = "".join(f"S\ts{k}\t{s}\tLN:i:{len(s)}\n" for k, s in enumerate(seqs)) + "L\ts0\t+\ts1\t+\t30M\nL\ts1\t-\ts3\t+\t50M\n"
    _reads_equal(_write(tmp_path / "long.gfa", text))


def _pressure_names():
    tails = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ01234567"
    return [("N" * k) + t for k in range(1, 26) for t in tails]   # 1 500 names: one last byte, one length apart


def test_name_table_under_pressure(tmp_path):
    names = _pressure_names()
    assert len(names) == len(set(names)) == 1500
    rng = np.random.default_rng(7)
    links = [(int(a), int(b), "+-"[int(c)], "+-"[int(d)], int(n)) for a, b, c, d, n in
             zip(rng.integers(0, 1500, 6000), rng.integers(0, 1500, 6000), rng.integers(0, 2, 6000), rng.integers(0, 2, 6000), rng.integers(1, 99, 6000))]
    links += [(k, (k + 1) % 1500, "+", "+", 5) for k in range(1500)]    # every name is looked up
    body = "".join(f"L\t{names[a]}\t{c}\t{names[b]}\t{d}\t{n}M\n" for a, b, c, d, n in links)
    path = _write(tmp_path / "names.gfa", "".join(f"S\t{nm}\t*\tLN:i:{100 + k}\n" for k, nm in enumerate(names)) + body)
    want = gfa.read_gfa(path, similarity=None)
    data = np.fromfile(path, dtype=np.uint8)
    for cap in (2048, None):      # 2048: the smallest power of two above 1 500
        p = gfa._parse_on_device(data, dev(), table_capacity=cap)
        assert torch.equal(p["src"].cpu(), want["src"]) and torch.equal(p["dst"].cpu(), want["dst"])
        assert torch.equal(p["overlap_length"].cpu(), want["overlap_length"]) and torch.equal(p["read_length"].cpu(), want["read_length"])
    with pytest.raises(Exception, match="power of two"):
        gfa._parse_on_device(data, dev(), table_capacity=1024)
    # the same file with one name repeated twice more: the FIRST repeat is the line reported, whatever order the lanes arrive in
    dup = list(names)
    dup[900] = dup[1200] = dup[100]
    path = _write(tmp_path / "dup.gfa", "".join(f"S\t{nm}\t*\tLN:i:{100 + k}\n" for k, nm in enumerate(dup)) + body)
    for cap in (2048, None):
        with pytest.raises(gfa.GfaDeviceError, match="line 901: a second S line") as ex:
            gfa._parse_on_device(np.fromfile(path, dtype=np.uint8), dev(), path=path, table_capacity=cap)
        assert ex.value.line == 901


def _layout_with_sequences(path, reads, seed, tags=False):
    """A random genome read left to right: read r starts step bases after read r-1 and overlaps the next few; a few bases of every read are
    changed, so the overlaps' edit distances are not zero.  Sequences on the S lines; SI:f: tags only with tags=True."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=reads * 500 + 2500)
    start = np.cumsum(rng.integers(300, 500, size=reads))
    length = rng.integers(1200, 2000, size=reads)
    with open(path, "w") as f:
        for r in range(reads):
            s = genome[start[r]:start[r] + length[r]].copy()
            hit = rng.integers(0, s.size, size=5)
            s[hit] = (s[hit] + 1) % 4
            length[r] = s.size
            f.write(f"S\tread{r}\t{''.join('ACGT'[c] for c in s)}\tLN:i:{s.size}\n")
        for r in range(reads):
            for t in range(r + 1, reads):
                ol = start[r] + length[r] - start[t]
                if ol <= 100:
                    break
                if start[t] + length[t] <= start[r] + length[r]:
                    continue
                f.write(f"L\tread{r}\t+\tread{t}\t+\t{int(ol)}M" + (f"\tSI:f:{1.0 - 0.002 * rng.random():.6f}\n" if tags else "\n"))
    return str(path)


def test_similarity_without_the_host(tmp_path):
    path = _layout_with_sequences(tmp_path / "layout.gfa", 120, seed=8)
    want = gfa.read_gfa(path, similarity="device")
    g = gfa.read_gfa_device(path, similarity="device")
    sim = g["overlap_similarity"]
    assert sim.device == dev() and sim.dtype == torch.float32 and torch.equal(sim.cpu(), want["overlap_similarity"])
    # at most 10 changed bases in an overlap of more than 100: above 0.9, and not all of them 1
    assert 0.9 < float(sim.min()) and float(sim.max()) <= 1.0 and bool((sim < 1).any()) and sim.numel() > 200
    assert gfa.read_gfa_device(path, similarity=None)["overlap_similarity"] is None


S3 = "S\ta\t*\tLN:i:50\nS\tb\t*\tLN:i:60\nS\tutg1\t*\tLN:i:70\n"
DECLINES = [   # (name, text, 1-based line the device parser names)
    ("two S lines with one name", S3 + "S\tb\t*\tLN:i:9\nL\ta\t+\tb\t+\t5M\n", 4),
    ("a byte >= 0x80", S3.encode() + b"# caf\xc3\xa9\nL\ta\t+\tb\t+\t5M\n", 4),
    ("a bare carriage return", S3 + "L\ta\t+\tb\t+\t5M\rL\tb\t+\ta\t+\t6M\n", 4),
    ("a signed length", "S\ta\t*\tLN:i:50\nS\tb\t*\tLN:i:+60\nL\ta\t+\tb\t+\t5M\n", 2),
    ("nineteen digits", S3 + "L\ta\t+\tb\t+\t1234567890123456789M\n", 4),
    ("an overlap that is no integer", S3 + "L\ta\t+\tb\t+\t5M\nL\ta\t-\tb\t+\t12x4M\n", 5),
    ("a long tag value", S3 + "L\ta\t+\tb\t+\t5M\tSI:f:0.0000000000000000000000000000001\n", 4),
    ("an S line with three fields", "S\ta\t*\tLN:i:50\nS\tb\t*\nL\ta\t+\ta\t-\t5M\n", 2),
    ("an A line of a run with four fields", S3 + "A\tutg1\t0\t+\tm/1/ccs\nA\tutg1\t9\t-\nL\ta\t+\tb\t+\t5M\n", 5),
    ("an L line with five fields", S3 + "L\ta\t+\tb\t+\n", 4),
    ("an L line with nine fields", S3 + "L\ta\t+\tb\t+\t5M\tx\ty\tz\n", 4),
    ("a 7-field name without a suffix", S3 + "L\ta:1-9\t+\tb\t+\t5M\tL1:i:3\n", 4),
    ("an unknown segment", S3 + "L\ta\t+\tb\t+\t5M\nL\ta\t+\tnobody\t+\t5M\n", 5),
    ("a segment defined later", "S\ta\t*\tLN:i:50\nL\ta\t+\tb\t+\t5M\nS\tb\t*\tLN:i:60\n", 2),
    ("two faults, the earlier one", S3 + "L\ta\t+\tb\t+\n\nL\ta\t+\tnobody\t+\t5M\nS\ta\t*\tLN:i:1\n", 4),
    ("two faults, the later kind first", S3 + "L\ta\t+\tnobody\t+\t5M\nL\ta\t+\tb\t+\n", 4),
]
HOST_RAISES = {"an unknown segment": KeyError, "a segment defined later": KeyError, "an L line with five fields": ValueError,
               "an overlap that is no integer": ValueError, "two faults, the earlier one": ValueError}


@pytest.mark.parametrize("name,text,line", DECLINES, ids=[d[0] for d in DECLINES])
def test_declines_and_errors(tmp_path, name, text, line):
    path = _write(tmp_path / "bad.gfa", text)
    with pytest.raises(gfa.GfaDeviceError, match=f"line {line}:") as ex:
        gfa.read_gfa(path, similarity=None, parser="device")
    assert ex.value.line == line and isinstance(ex.value, ValueError)
    host = _outcome(lambda: gfa.read_gfa(path, similarity=None, parser="host"))
    auto = _outcome(lambda: gfa.read_gfa(path, similarity=None, parser="auto"))
    if isinstance(host, dict):
        _same(auto, host)
    else:
        assert auto == host
    if name in HOST_RAISES:
        assert not isinstance(host, dict) and host[0] is HOST_RAISES[name]
        if name == "an L line with five fields":
            assert host[1] == "Unknown GFA format!"
    # a zero overlap is dropped before its names are looked at, and a good file parses after a declined one in the same process
    good = _write(tmp_path / "good.gfa", S3 + "L\ta\t+\tnobody\t+\t0M\nA\tstray\t0\nL\ta\t+\tb\t-\t5M\tSI:f:1e-3\n")
    want = _both(good, similarity=None)
    assert want["src"].tolist() == [0, 2] and want["overlap_similarity"].tolist() == [np.float32(1e-3)] * 2


def test_gz_input(tmp_path):
    text = adversarial_gfa(3, tags="all", sequences=True).encode("ascii")
    path = str(tmp_path / "adv.gfa.gz")
    with gzip.open(path, "wb") as f:
        f.write(text)
    _both(path, similarity=None, keep_sequences=True)


def test_pipeline_reads_the_gfa_once(tmp_path, monkeypatch):
    from gnnome_amd import decode, pipeline
    path = _layout_with_sequences(tmp_path / "layout.gfa", 150, seed=9, tags=True)
    g = gfa.read_gfa(path)
    src, dst = g["src"], g["dst"]
    hop = torch.where(src % 2 == 0, (dst - src) // 2, (src - dst) // 2).float()
    scores = (10.0 - 2.0 * hop).to(dev())
    opened = []
    real_open, real_gz = builtins.open, gzip.open

    def counting(real):
        def wrapper(file, *a, **kw):
            if isinstance(file, (str, os.PathLike)) and os.fspath(file) == path:
                opened.append(file)
            return real(file, *a, **kw)
        return wrapper

    out = {}
    for parser in ("host", "device"):
        torch.manual_seed(1)
        fasta = tmp_path / f"{parser}.fasta"
        with monkeypatch.context() as m:
            m.setattr(builtins, "open", counting(real_open))
            m.setattr(gzip, "open", counting(real_gz))
            opened.clear()
            walks, contigs, stats = pipeline.assemble_to_fasta(path, None, str(fasta), 10, scores=scores, sampler=decode.sample_edges_device,
                                                               nb_paths=20, device=dev(), parser=parser)
            count = len(opened)
        out[parser] = (walks, fasta.read_bytes(), stats, count)
    assert out["device"][0] == out["host"][0] and len(out["host"][0]) >= 1
    assert out["device"][1] == out["host"][1] and len(out["host"][1]) > 1000
    assert out["device"][2] == out["host"][2]
    assert out["device"][3] == 1 and out["host"][3] > 1


def test_read_store_from_packed_keeps_the_touched_reads(tmp_path):
    from gnnome_amd import contigs
    path = _layout_with_sequences(tmp_path / "layout.gfa", 40, seed=10)
    g = gfa.read_gfa_device(path, similarity=None)
    keep = [0, 3, 4, 17, 39]
    got = contigs.ReadStore.from_packed(*g["reads"], keep=keep)
    want = contigs.ReadStore.from_gfa(path, keep=keep, device=dev())
    assert torch.equal(got.data, want.data) and torch.equal(got.off, want.off) and np.array_equal(got.missing, want.missing)
    whole = contigs.ReadStore.from_packed(*g["reads"])
    assert whole.missing is None and whole.num_reads == 40 and whole.data is g["reads"][0]
