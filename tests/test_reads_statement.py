"""Host-side checks of the device reads reader's surroundings (no GPU): the generator tests/reads_statement.py against the host
statement contigs.read_sequences / read_titles, and the torch glue of gnnome_amd/reads.py on CPU tensors against short Python
restatements.  The kernels themselves: tests/test_reads_device.py (-m gpu)."""
import gzip
import re
from collections import Counter

import numpy as np
import pytest
import torch

from gnnome_amd import _lib, contigs, gfa, reads
from reads_statement import reads_case

SEEDS = range(30)


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_says_what_the_host_reads(tmp_path, seed):
    case = reads_case(seed)
    plain = tmp_path / f"reads{case['suffix']}"
    plain.write_bytes(case["text"])
    packed = tmp_path / f"reads{case['suffix']}.gz"
    with gzip.open(packed, "wb") as f:
        f.write(case["text"])
    for path in (str(plain), str(packed)):
        assert contigs.reads_file_type(path) == case["kind"]
        assert contigs.read_sequences(path) == case["sequences"]
        assert contigs.read_titles(path) == case["titles"]
        assert contigs.read_sequences(path, set(case["wanted"])) == {r: case["sequences"][r] for r in case["wanted"]}
    assert set(case["names"]) <= set(case["sequences"]) and len(case["names"]) > len(set(case["names"]))
    for key in ("gfa_plain", "gfa_utg"):   # every read a GFA names has a record with the four fields
        g = tmp_path / "g.gfa"
        g.write_text(case[key])
        out = gfa.read_gfa(str(g), similarity=None, training=True, reads_path=str(plain), labels=False)
        assert out["read_start"].numel() == out["num_nodes"] > 0


def test_the_seeds_cover_what_they_claim():
    cases = [reads_case(s) for s in SEEDS]
    text = [c["text"] for c in cases]
    assert {c["kind"] for c in cases} == {"fasta", "fastq"}
    assert any(b"\r\n" in t for t in text) and any(not t.endswith(b"\n") for t in text)
    assert any(not t.startswith((b">", b"@")) for t in text)                      # lines above the first header
    assert any(re.search(rb"\n >", t) for t in text) and any(re.search(rb"\n>[ \t]+\S", t) for t in text)
    assert any("" in c["sequences"] for c in cases)                                  # the empty id
    assert any(re.search(rb"\n\+[^\n]*\r?\n[ \t\x0b\x0c\x1c]*\r?\n?@[^\n]*\r?\n@", t) or re.search(rb"\n\+[^\n]*\n@[^\n]*\n@", t)
               for c, t in zip(cases, text) if c["kind"] == "fastq")                 # a quality line that starts with '@'
    assert any(re.search(rb"\n\+[^\n]*\n\+", t) for c, t in zip(cases, text) if c["kind"] == "fastq")
    assert any(re.search(rb"start=\d{18}\b", t) for t in text) and any(b"xstart=7" in t for t in text)
    assert any(max(len(ln) for ln in t.split(b"\n")) > gfa.TOKENISE_TILE for t in text)


def _pack_items_python(last, keep, seq_first, item_beg, item_len):
    beg, length, first = [], [], [0]
    for r, k in enumerate(last):
        if k >= 0 and (keep is None or keep[r]):
            beg += item_beg[seq_first[k]:seq_first[k + 1]]
            length += item_len[seq_first[k]:seq_first[k + 1]]
        first.append(len(beg))
    return beg, length, first


@pytest.mark.parametrize("seed", range(8))
def test_pack_items_on_cpu_tensors(seed):
    rng = np.random.default_rng(seed)
    K, R = (0, 5) if seed == 0 else (int(rng.integers(1, 40)), int(rng.integers(0, 60)))
    per = rng.integers(0, 4, size=K)
    seq_first = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    S = int(seq_first[-1])
    item_beg, item_len = rng.integers(0, 10 ** 6, size=S), rng.integers(1, 99, size=S)
    last = rng.integers(-1, max(K, 1), size=R) if K else np.full(R, -1)
    for keep in (None, rng.random(R) < 0.5):
        got = reads.pack_items(torch.from_numpy(last.astype(np.int64)), None if keep is None else torch.from_numpy(keep),
                               torch.from_numpy(seq_first), torch.from_numpy(item_beg), torch.from_numpy(item_len))
        want = _pack_items_python(last.tolist(), keep, seq_first.tolist(), item_beg.tolist(), item_len.tolist())
        assert [t.tolist() for t in got] == [list(w) for w in want]


def _combine_python(owner, sign, ann, segments):
    out = [[0, 0, 0, 0] for _ in range(segments)]
    for s in range(segments):
        rows = [(a, o) for a, o, w in zip(ann, sign, owner) if w == s]
        if rows:     # gfa._node_annotations' own expressions
            out[s] = [1 if sum(a[0] * o for a, o in rows) >= 0 else -1, min(a[1] for a, _ in rows), max(a[2] for a, _ in rows),
                      Counter(a[3] for a, _ in rows).most_common()[0][0]]
    return out


@pytest.mark.parametrize("seed", range(8))
def test_combine_annotations_on_cpu_tensors(seed):
    rng = np.random.default_rng(100 + seed)
    segments = int(rng.integers(1, 30))
    count = rng.integers(0, 7, size=segments)
    owner = np.repeat(np.arange(segments), count)
    E = owner.size
    sign = rng.choice([-1, 1], size=E)
    ann = np.stack([rng.choice([-1, 1], size=E), rng.integers(0, 10 ** 18, size=E), rng.integers(0, 10 ** 18, size=E),
                    rng.choice([-3, -2, -1, 1, 2, 7], size=E)], axis=1).astype(np.int64).reshape(E, 4)
    got = reads.combine_annotations(torch.from_numpy(owner), torch.from_numpy(sign), torch.from_numpy(ann), segments)
    assert got.dtype == torch.int64 and got.tolist() == _combine_python(owner.tolist(), sign.tolist(), ann.tolist(), segments)


def test_wanted_reads_flattens_node_to_read():
    n2r = {0: "a", 1: "a", 2: [("r1", "+"), ("r2", "-")], 3: [("r1", "+"), ("r2", "-")], 4: [], 5: [], 6: "a", 7: "a"}
    names, owner, sign, segments = reads.wanted_reads(n2r, 8)
    assert names == ["a", "r1", "r2", "a"] and owner.tolist() == [0, 1, 1, 3] and sign.tolist() == [1, 1, -1, 1] and segments == 4
    assert reads._pack_names(["ab", "", "c"])[0].tobytes() == b"abc" and reads._pack_names(["ab", "", "c"])[1].tolist() == [0, 2, 2, 3]


def test_entries_declared_and_keywords_checked(tmp_path):
    header = open(_lib.HEADER_PATH).read()
    for name in ("gnnome_reads_records_fasta", "gnnome_reads_records_fastq", "gnnome_reads_names_insert", "gnnome_reads_match",
                 "gnnome_reads_annotations"):
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header)
    assert "graph_parser.py:121-136" in header and ":213-272" in header and ":341-366" in header
    assert set(reads._DECLINED) == set(range(1, 9)) and issubclass(reads.ReadsDeviceError, ValueError)
    err = reads.ReadsDeviceError("f.fa", 3, reads._DECLINED[1])
    assert err.line == 3 and err.reason == reads._DECLINED[1] and "line 3:" in str(err)
    with pytest.raises(ValueError, match="reads_parser="):
        gfa.read_gfa(str(tmp_path / "none.gfa"), reads_parser="gpu")
    with pytest.raises(ValueError, match="parser="):
        contigs.ReadStore.from_reads_file(str(tmp_path / "none.fa"), {}, 0, parser="gpu")
