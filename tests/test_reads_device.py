"""The device reads reader (csrc/reads_parse.hip, gnnome_amd/reads.py) against the host statement it restates: contigs.read_sequences /
read_titles through ReadStore.from_reads_file(parser="host"), and gfa._node_annotations through read_gfa(reads_parser="host").  Every
tensor with torch.equal, every error by type and text; "auto" is never the only path compared."""
import gzip
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gnnome_amd import contigs, gfa, reads
from reads_statement import reads_case

pytestmark = pytest.mark.gpu

G14 = {"g14_single.gfa": "g14_single.fasta", "g14_multi.gfa": "g14_multi.fasta", "g14_utg_x.gfa": "g14_utg_x.fastq.gz"}
T = "strand=+ start=1 end=9 chr=2"


def dev():
    return torch.device("cuda", 0)


def _outcome(fn):
    try:
        return fn()
    except Exception as ex:   # noqa: BLE001 (the outcome IS the exception)
        return (type(ex), str(ex))


def _write(path, text):
    path.write_bytes(text if isinstance(text, bytes) else text.encode("ascii"))
    return str(path)


def _same_dict(got, want):
    assert got.keys() == want.keys()
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert torch.is_tensor(g) and g.dtype == w.dtype and g.device == w.device and torch.equal(g, w), k
        else:
            assert type(g) is type(w) and g == w, k


def _training(gfa_path, reads_path, parsers=("host", "device"), must_serve=True):
    """read_gfa(training=True) with reads_parser "device" and "auto" against "host", under each GFA parser; -> the host outcome."""
    host = None
    for parser in parsers:
        run = lambda rp: gfa.read_gfa(gfa_path, similarity=None, training=True, reads_path=reads_path, labels=False,   # noqa: E731
                                      parser=parser, reads_parser=rp)
        host = _outcome(lambda: run("host"))
        for rp in ("device", "auto"):
            got = _outcome(lambda: run(rp))
            if isinstance(host, dict):
                assert isinstance(got, dict), got
                _same_dict(got, host)
                assert all(got[k].dtype == torch.int64 and got[k].device.type == "cpu" for k in ("read_strand", "read_start", "read_end", "read_chr"))
            else:
                assert got == host
        if must_serve:
            assert isinstance(host, dict), host
    return host


def _store(reads_path, g, keep=None, must_serve=True):
    """ReadStore.from_reads_file with parser "device" and "auto" against "host": equal data, off and missing, or the same exception."""
    run = lambda p: contigs.ReadStore.from_reads_file(reads_path, g["node_to_read"], g["num_nodes"], keep=keep, device=dev(), parser=p)   # noqa: E731
    host = _outcome(lambda: run("host"))
    for p in ("device", "auto"):
        got = _outcome(lambda: run(p))
        if isinstance(host, tuple):
            assert got == host
        else:
            assert isinstance(got, contigs.ReadStore), got
            assert got.data.dtype == torch.uint8 and got.off.dtype == torch.int64 and got.data.device == host.data.device
            assert torch.equal(got.data, host.data) and torch.equal(got.off, host.off)
            assert (got.missing is None) == (host.missing is None) and (host.missing is None or np.array_equal(got.missing, host.missing))
    if must_serve:
        assert isinstance(host, contigs.ReadStore), host
    return host


@pytest.mark.parametrize("name", sorted(G14))
def test_goldens(name):
    gfa_path, reads_path = os.path.join(GOLDEN, name), os.path.join(GOLDEN, G14[name])
    want = _training(gfa_path, reads_path)
    got = gfa.read_gfa(gfa_path, similarity=None, training=True, reads_path=reads_path, parser="device", reads_parser="device")
    assert got["y"] is not None and torch.equal(got["y"], gfa.read_gfa(gfa_path, similarity=None, training=True, reads_path=reads_path)["y"])
    host = _store(reads_path, want, must_serve=False)
    assert isinstance(host, tuple) == (name == "g14_utg_x.gfa")     # a unitig has no single record: the same ValueError


@pytest.mark.parametrize("seed", range(30))
def test_generator_seeds(tmp_path, seed):
    case = reads_case(seed)
    reads_path = _write(tmp_path / f"reads{case['suffix']}", case["text"])
    if seed % 7 == 5:
        reads_path += ".gz"
        with gzip.open(reads_path, "wb") as f:
            f.write(case["text"])
    res = reads.read_reads_device(reads_path, case["names"], device=dev(), sequences=True, titles=True)    # "device" itself serves it
    data, off = res.data.cpu().numpy().tobytes(), res.off.tolist()
    assert res.data.device == dev() and len(off) == len(case["names"]) + 1 and bool((res.last >= 0).all())
    for i, name in enumerate(case["names"]):
        assert data[off[i]:off[i + 1]] == case["sequences"][name], name
    assert reads.record_title(res, int(res.last[0])) == case["titles"][case["names"][0]]
    plain = _write(tmp_path / "plain.gfa", case["gfa_plain"])
    want = _training(plain, reads_path)
    _training(_write(tmp_path / "utg.gfa", case["gfa_utg"]), reads_path)
    R = want["num_nodes"] // 2
    mask = np.random.default_rng(seed).random(R) < 0.5
    for keep in (None, mask, [0, R - 1, R // 2]):
        _store(reads_path, want, keep=keep)


def _bases(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))


def _reads_gfa(tmp_path, ids):
    return _write(tmp_path / "reads.gfa", "".join(f"S\t{r}\t*\tLN:i:9\n" for r in ids))


@pytest.mark.parametrize("kind", ["fasta", "fastq"])
def test_tile_borders(tmp_path, kind):
    """The last sequence line of the first record ends 18 below to 2 above a multiple of each kernel's tile."""
    rng = np.random.default_rng(11)
    g = gfa.read_gfa(_reads_gfa(tmp_path, ["a", "b", "c"]), similarity=None)
    for tile in (gfa.TOKENISE_TILE, gfa.PACK_TILE, 2 * gfa.TOKENISE_TILE):
        for q in range(tile - 18, tile + 3):
            seq = _bases(rng, q)
            if kind == "fasta":
                text = f">a {T}\nACGTAC\n{seq}\n>b {T}\nACGTTGCAAC\n\n>c {T}\n{seq[:37]}"
            else:
                text = f"@a {T}\n{seq}\n+\n{'I' * q}\n@b {T}\nACGTTGCAAC\n+a\n@+III+III@\n\n@c {T}\n{seq[:37]}\n+\n{'+' * 37}"
            path = _write(tmp_path / f"border.{kind}", text)
            _store(path, g)
    _training(_reads_gfa(tmp_path, ["a", "b", "c"]), path)


@pytest.mark.parametrize("kind", ["fasta", "fastq"])
def test_one_long_read_among_short_ones(tmp_path, kind):
    rng = np.random.default_rng(12)
    seqs = [_bases(rng, n) for n in (40, 70_001, 1, 55, 16, 15, 17)]
    if kind == "fasta":
        text = "".join(f">s{k} {T}\n{s}\n" for k, s in enumerate(seqs))
    else:
        text = "".join(f"@s{k} {T}\n{s}\n+\n{'F' * len(s)}\n" for k, s in enumerate(seqs))
    g = gfa.read_gfa(_reads_gfa(tmp_path, [f"s{k}" for k in range(7)]), similarity=None)
    host = _store(_write(tmp_path / f"long.{kind}", text), g)
    assert host.off.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).tolist()


def _pressure_names():
    tails = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ01234567"
    return [("N" * k) + t for k in range(1, 26) for t in tails]   # 1 500 names: one last byte, one length apart (test_gfa_device's)


def test_name_table_under_pressure(tmp_path):
    names = _pressure_names()
    assert len(names) == len(set(names)) == 1500
    rng = np.random.default_rng(13)
    order = rng.permutation(1500)
    seqs = {names[k]: _bases(rng, 3 + k % 7) for k in range(1500)}
    path = _write(tmp_path / "names.fasta", "".join(f">{names[k]} {T}\n{seqs[names[k]]}\n" for k in order))
    position = {names[k]: i for i, k in enumerate(order)}
    for cap in (None, 2048):      # 2048: the smallest power of two above 1 500
        res = reads.read_reads_device(path, names, device=dev(), table_capacity=cap)
        assert res.last.tolist() == [position[nm] for nm in names]
        data, off = res.data.cpu().numpy().tobytes(), res.off.tolist()
        assert all(data[off[i]:off[i + 1]].decode() == seqs[nm] for i, nm in enumerate(names))
    with pytest.raises(reads.ReadsDeviceError, match="the name table is full") as ex:     # too small: reported, never a wrong match
        reads.read_reads_device(path, names, device=dev(), table_capacity=1024)
    assert ex.value.line == 0 and ex.value.reason == reads._DECLINED[7]
    with pytest.raises(Exception, match="power of two"):
        reads.read_reads_device(path, names, device=dev(), table_capacity=1500)
    many = names + [nm + "#" for nm in names[:547]]     # 2 047 distinct names in 2 048 slots: one free slot ends every failed search
    assert len(set(many)) == 2047
    res = reads.read_reads_device(path, many, device=dev(), table_capacity=2048)
    assert res.last[:1500].tolist() == [position[nm] for nm in names] and bool((res.last[1500:] == -1).all())
    g = gfa.read_gfa(_write(tmp_path / "names.gfa", "".join(f"S\t{nm}\t*\tLN:i:5\n" for nm in names)), similarity=None)
    _store(path, g)
    _training(str(tmp_path / "names.gfa"), path, parsers=("host",))


def test_last_record_wins(tmp_path):
    rng = np.random.default_rng(14)
    seqs = [_bases(rng, 20 + k) for k in range(64)]
    for kind, text in (("fasta", "".join(f">other {T}\nAC\n>dup start={k} {T}\n{s}\n" for k, s in enumerate(seqs))),
                       ("fastq", "".join(f"@dup start={k} {T}\n{s}\n+\n{'#' * len(s)}\n" for k, s in enumerate(seqs)))):
        path = _write(tmp_path / f"dup.{kind}", text)
        runs = [reads.read_reads_device(path, ["dup"], device=dev(), titles=True) for _ in range(2)]
        assert runs[0].data.cpu().numpy().tobytes().decode() == seqs[63] and runs[0].ann[0].tolist() == [1, 63, 9, 2]
        assert torch.equal(runs[0].data, runs[1].data) and torch.equal(runs[0].last, runs[1].last)
        g = gfa.read_gfa(_reads_gfa(tmp_path, ["dup"]), similarity=None)
        _store(path, g)


ERROR_GFAS = {
    "a wanted read absent, the first of several": "S\ta\t*\tLN:i:4\nS\tzz\t*\tLN:i:4\nS\tyy\t*\tLN:i:4\n",
    "absent and named only on an A line": "S\tutg1\t*\tLN:i:4\nA\tutg1\t0\t+\ta\nA\tutg1\t0\t-\tnobody\nS\tww\t*\tLN:i:2\n",
    "no strand": "S\ta\t*\tLN:i:4\nS\tm1\t*\tLN:i:4\n", "no start": "S\tm2\t*\tLN:i:4\n", "no end": "S\ta\t*\tLN:i:4\nS\tm3\t*\tLN:i:4\n",
    "no chr": "S\tm4\t*\tLN:i:4\nS\tm1\t*\tLN:i:4\n", "two fields at once": "S\tutg1\t*\tLN:i:4\nA\tutg1\t0\t+\ta\nA\tutg1\t0\t-\tm5\n",
    "a unitig without A lines": "S\ta\t*\tLN:i:4\nS\tutg2\t*\tLN:i:4\nS\tzz\t*\tLN:i:4\n",
    "nothing wrong": "S\tutg1\t*\tLN:i:4\nA\tutg1\t0\t-\ta\nA\tutg1\t0\t-\td\n",
}


@pytest.mark.parametrize("name", sorted(ERROR_GFAS))
def test_errors_equal_the_hosts(tmp_path, name):
    path = _write(tmp_path / "e.fasta", f">a {T}\nACGT\n>m1 start=1 end=9 chr=2\nAC\n>m2 strand=- start=x end=9 chr=X\nAC\n>m3 strand=- start=4 chr=M\nGG\n"
                                        f">m4 strand=- start=4 end=5 chr=Z\nGG\n>m5 start=4 chr=7\nGG\n>d strand=- start=0 end=5 chr=Y\nTT\n")
    g = _write(tmp_path / "e.gfa", ERROR_GFAS[name])
    host = _training(g, path, must_serve=False)
    assert isinstance(host, dict) == (name == "nothing wrong")
    if not isinstance(host, dict):
        assert host[0] is ValueError
    _store(path, gfa.read_gfa(g, similarity=None), must_serve=False)


DECLINES = [   # (a row of reads._DECLINED, file name, bytes, the 1-based line named)
    (1, "x.fasta", f">a {T}\nACGT\nAC GT\n", 3),
    (1, "q.fastq", f"@a {T}\nAC\tGT\n+\nIIII\n", 2),
    (2, "x.fastq", f"@a {T}\nACGT\n+\nIIII\n@b {T}\nACGT\nAC\n+\nIIIIII\n", 7),
    (2, "e.fastq", f"@b\n\n+\n\n@a {T}\nAC\n+\nII\n", 3),
    (2, "t.fastq", f"@a {T}\nACGT\n+\nIIII\n@b\nAC\n+\n", 5),
    (3, "x.fasta", f">z\nAC\n>a strand=+ start=1234567890123456789 end=9 chr=2\nAC\n", 3),
    (4, "x.fasta", f">a strand=+ start=1 end=9 chr=X1\nAC\n", 1),
    (5, "x.fasta", f">a {T}\nAC\n>b caf".encode() + b"\xc3\xa9\nAC\n", 3),
    (6, "x.fasta", f">a {T}\nAC\rGT\n", 2),
    (1, "two.fasta", f">a {T}\nAC GT\n>b start=1234567890123456789\nAC\n>a start=1234567890123456789 {T}\nAC\n", 2),
    (5, "two.fastq", f"@a {T}\nAC\n+\nI".encode() + b"\xff\n@b\nACGT\n+\nII\n", 4),
]


@pytest.mark.parametrize("code,name,text,line", DECLINES, ids=[f"{d[0]}-{d[1]}" for d in DECLINES])
def test_declined_inputs(tmp_path, code, name, text, line):
    path = _write(tmp_path / name, text)
    with pytest.raises(reads.ReadsDeviceError) as ex:
        reads.read_reads_device(path, ["a", "b"], device=dev(), sequences=True, titles=True)
    assert ex.value.line == line and ex.value.reason == reads._DECLINED[code] and f"line {line}:" in str(ex.value)
    g = _write(tmp_path / "g.gfa", "S\ta\t*\tLN:i:4\n")
    n2r = gfa.read_gfa(g, similarity=None)
    run = lambda p: contigs.ReadStore.from_reads_file(path, n2r["node_to_read"], 2, device=dev(), parser=p)   # noqa: E731
    host, auto = _outcome(lambda: run("host")), _outcome(lambda: run("auto"))
    if code in (3, 4):      # the titles' numbers are not read for the sequences: served, and equal to the host's
        auto = run("device")
    else:
        with pytest.raises(reads.ReadsDeviceError):
            run("device")
    if isinstance(host, tuple):
        assert auto == host
    else:
        assert torch.equal(auto.data, host.data) and torch.equal(auto.off, host.off)
    train = lambda rp: gfa.read_gfa(g, similarity=None, training=True, reads_path=path, labels=False, reads_parser=rp)   # noqa: E731
    host, auto = _outcome(lambda: train("host")), _outcome(lambda: train("auto"))
    if isinstance(host, tuple):
        assert auto == host
    else:
        _same_dict(auto, host)
    with pytest.raises(reads.ReadsDeviceError):
        train("device")


def test_max_bytes_declines_before_the_upload(tmp_path):
    path = _write(tmp_path / "big.fasta", f">a {T}\n" + "ACGT" * 5000 + "\n")
    size = os.path.getsize(path)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev())
    before = torch.cuda.memory_allocated(dev()), torch.cuda.max_memory_allocated(dev())
    for p in (path, path + ".gz"):
        if p.endswith(".gz"):
            with gzip.open(p, "wb") as f:
                f.write(open(path, "rb").read())
        with pytest.raises(reads.ReadsDeviceError, match="above max_bytes") as ex:
            reads.read_reads_device(p, ["a"], device=dev(), max_bytes=20_000)
        assert ex.value.line == 0
    assert (torch.cuda.memory_allocated(dev()), torch.cuda.max_memory_allocated(dev())) == before
    assert reads.read_reads_device(path, ["a"], device=dev(), max_bytes=size).off.tolist() == [0, 20_000]
    assert set(reads._DECLINED) == {d[0] for d in DECLINES} | {7, 8}


@pytest.mark.parametrize("text,kind", [("", "fasta"), ("", "fastq"), ("\n \n\t\n", "fasta"), ("\n \n\t\n", "fastq"), (">a", "fasta"), (">a\n\n", "fasta")])
def test_empty_and_near_empty_inputs(tmp_path, text, kind):
    path = _write(tmp_path / f"n.{kind}", text)
    res = reads.read_reads_device(path, ["a"], device=dev(), sequences=True, titles=True)
    assert res.last.tolist() == ([0] if text.startswith(">") else [-1]) and res.off.tolist() == [0, 0] and res.missing.tolist() == [15]
    none = reads.read_reads_device(path, [], device=dev(), sequences=True, titles=True)
    assert none.last.numel() == 0 and none.off.tolist() == [0] and none.data.numel() == 0 and tuple(none.ann.shape) == (0, 4)
    g = gfa.read_gfa(_reads_gfa(tmp_path, ["a"]), similarity=None)
    _store(path, g, must_serve=text.startswith(">"))
    _training(_reads_gfa(tmp_path, ["a"]), path, must_serve=False)


def test_assemble_to_fasta_end_to_end(tmp_path):
    from gnnome_amd import decode, pipeline
    case = reads_case(1, kind="fastq", records=24)
    reads_path = _write(tmp_path / "reads.fq", case["text"])
    order = case["wanted"]
    lengths = {r: len(case["sequences"][r]) for r in order}
    text = "".join(f"S\t{r}\t*\tLN:i:{lengths[r]}\n" for r in order) + "".join(f"L\t{a}\t+\t{b}\t+\t3M\n" for a, b in zip(order, order[1:]))
    path = _write(tmp_path / "chain.gfa", text)
    g = gfa.read_gfa(path, similarity=None)
    scores = torch.where(g["src"] % 2 == 0, 5.0, -5.0).to(dev())
    out = {}
    for parser, reads_parser in (("host", "host"), ("device", "device")):
        torch.manual_seed(1)
        fasta = tmp_path / f"{parser}.fasta"
        walks, _, stats = pipeline.assemble_to_fasta(path, None, str(fasta), 10, reads=reads_path, similarity=None, scores=scores,
                                                     sampler=decode.sample_edges_device, nb_paths=5, device=dev(), parser=parser,
                                                     reads_parser=reads_parser)
        out[parser] = (walks, fasta.read_bytes(), stats)
    assert out["device"] == out["host"] and len(out["host"][0]) >= 1 and len(out["host"][1]) > 100
