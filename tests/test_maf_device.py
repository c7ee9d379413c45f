"""The device MAF reader (csrc/maf_parse.hip, gnnome_amd/maf.py) against the host statement it restates: every tensor with torch.equal,
every decline by type, line and reason; "auto" is never the only path compared.  The shapes of tests/maf_statement.py are the whole
workload: no large file is generated."""
import gzip
import json
import os

import pytest
import torch

from conftest import GOLDEN
from gnnome_amd import gfa, maf
from maf_statement import BAD_CASES, bad_case, maf_case

pytestmark = pytest.mark.gpu


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


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and g.device.type == "cpu" and torch.equal(g, w)


@pytest.mark.parametrize("seed", range(24))
def test_generator_seeds(tmp_path, seed):
    case = maf_case(seed)
    path = _write(tmp_path / "sim.maf", case["text"])
    if seed % 7 == 5:
        path += ".gz"
        with gzip.open(path, "wb") as f:
            f.write(case["text"])
    host = maf.read_maf_annotations(path, case["names"], case["chr"], parser="host")
    assert host[0].tolist() == case["ann"] and host[1].tolist() == case["last"]
    for parser in ("device", "auto"):
        _same(maf.read_maf_annotations(path, case["names"], case["chr"], parser=parser, device=dev()), host)
    _same(maf.read_maf_annotations(path, [], case["chr"], parser="device"), maf.read_maf_annotations(path, [], case["chr"]))
    for key in ("gfa_plain", "gfa_utg_chr"):
        g = gfa.read_gfa(_write(tmp_path / "g.gfa", case[key]), similarity=None)
        want = maf.node_annotations(g["node_to_read"], g["num_nodes"], path, chr=case["chr"], parser="host")
        _same(maf.node_annotations(g["node_to_read"], g["num_nodes"], path, chr=case["chr"], parser="device", device=dev()), want)


def test_fixture_and_the_multi_file_rule(tmp_path):
    want = json.load(open(os.path.join(GOLDEN, "maf_pbsim_small.json")))
    path = os.path.join(GOLDEN, "maf_pbsim_small.maf")
    ann, last = maf.read_maf_annotations(path, want["names"], want["chr"], parser="device")
    assert ann.tolist() == want["ann"] and last.tolist() == want["last"]
    other = _write(tmp_path / "cx.maf", "a\ns ref 70 4 + 99 ACGT\ns S1_1 0 4 - 4 ACGT\n\na\ns ref 80 4 + 99 ACGT\ns S2_1 0 4 + 4 ACGT")
    files = [(path, "chr21"), (other, "X")]
    names = ["S1_1_chrX", "S1_1_chr21", "S1_2", "S2_1", "S2_1_chr21", "S1_3"]
    _same(maf.read_maf_annotations(files, names, parser="device"), maf.read_maf_annotations(files, names))
    for parser in ("host", "device"):
        with pytest.raises(ValueError, match="read 'S1_1' has a block in more than one MAF file"):
            maf.read_maf_annotations(files, ["S1_2", "S1_1"], parser=parser)


@pytest.mark.parametrize("name", BAD_CASES)
def test_declined_inputs(tmp_path, name):
    case = bad_case(name)
    path = _write(tmp_path / "bad.maf", case["text"])
    with pytest.raises(maf.MafDeviceError) as ex:
        maf.read_maf_annotations(path, case["names"], 5, parser="device", device=dev())
    assert ex.value.line == case["line"] and ex.value.reason == maf._DECLINED[case["code"]] and f"line {case['line']}:" in str(ex.value)
    host = _outcome(lambda: maf.read_maf_annotations(path, case["names"], 5, parser="host"))
    auto = _outcome(lambda: maf.read_maf_annotations(path, case["names"], 5, parser="auto", device=dev()))
    assert isinstance(host, tuple) and (host[0] is ValueError) == case["raises"]
    if case["raises"]:
        assert auto == host and f"line {case['line']}: " in host[1]
    else:
        _same(auto, host)
        assert host[0].tolist() == case["ann"] and host[1].tolist() == case["last"]


def test_the_earliest_line_is_named(tmp_path):
    text = "a\ns ref 1 4 + 9 ACGT\n\na\ns ref 1 4 + 9 ACGT\ns r 0 4 + 4 ACGT\nq r 99\ns r2 0 5 + 4 ACGT\n\na\ns ref 7 3 + 9 ACGT\ns t 0 4 + 4 AC-T\n"
    for skip, line, code in ((0, 1, 7), (3, 4, 5), (3.5, 4, 7), (9, 2, 9)):
        lines = text.split("\n")[int(skip):]
        if skip == 3.5:
            del lines[3]
        path = _write(tmp_path / "e.maf", "\n".join(lines))
        with pytest.raises(maf.MafDeviceError) as ex:
            maf.read_maf_annotations(path, ["r"], 1, parser="device")
        assert (ex.value.line, ex.value.reason) == (line, maf._DECLINED[code])
        with pytest.raises(ValueError, match=f"line {line}: ") as host:
            maf.read_maf_annotations(path, ["r"], 1, parser="host")
        assert maf._DECLINED[code] in str(host.value)


def test_name_table_and_max_bytes(tmp_path):
    case = maf_case(1)
    path = _write(tmp_path / "sim.maf", case["text"])
    names = sorted(case["reads"])
    assert len(names) > 4
    with pytest.raises(maf.MafDeviceError, match="the name table is full") as ex:          # too small: reported, never a wrong match
        maf.read_maf_annotations(path, names, case["chr"], parser="device", table_capacity=4)
    assert ex.value.line == 0 and ex.value.reason == maf._DECLINED[12]
    host = maf.read_maf_annotations(path, names, case["chr"])
    _same(maf.read_maf_annotations(path, names, case["chr"], parser="auto", table_capacity=4), host)
    _same(maf.read_maf_annotations(path, names, case["chr"], parser="device", table_capacity=64), host)
    size = os.path.getsize(path)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev())
    before = torch.cuda.memory_allocated(dev()), torch.cuda.max_memory_allocated(dev())
    for p in (path, path + ".gz"):
        if p.endswith(".gz"):
            with gzip.open(p, "wb") as f:
                f.write(case["text"])
        with pytest.raises(maf.MafDeviceError, match="above max_bytes") as ex:
            maf.read_maf_annotations(p, names, case["chr"], parser="device", device=dev(), max_bytes=size - 1)
        assert ex.value.line == 0 and ex.value.reason.startswith(maf._DECLINED[13])
    assert (torch.cuda.memory_allocated(dev()), torch.cuda.max_memory_allocated(dev())) == before      # declined before the upload
    _same(maf.read_maf_annotations(path, names, case["chr"], parser="device", max_bytes=size), host)
    _same(maf.read_maf_annotations(path, names, case["chr"], parser="auto", max_bytes=size - 1), host)


@pytest.mark.parametrize("text", ["", "\n \n\t\n", "##maf version=1\n", "a\ns ref 1 1 + 9 A\ns r 0 1 + 1 A"])
def test_empty_and_near_empty_inputs(tmp_path, text):
    path = _write(tmp_path / "n.maf", text)
    for names in (["r", "q"], []):
        _same(maf.read_maf_annotations(path, names, "X", parser="device"), maf.read_maf_annotations(path, names, "X"))
    assert maf.read_maf_annotations(path, ["r"], "X", parser="device")[1].tolist() == ([0] if text.startswith("a") else [-1])


@pytest.mark.parametrize("name,reads,chrom", [("g14_single.gfa", "g14_single.fasta", "chr1"), ("g14_utg_x.gfa", "g14_utg_x.fastq.gz", "X")])
def test_read_gfa_gives_the_labels_of_the_titled_reads(tmp_path, name, reads, chrom):
    """The golden training graphs (plain S lines; utg* segments with A lines): a MAF written from their reads' titles - one block per
    read, the text as long as end - start - gives the read_* columns and the labels y that the titles give."""
    from gnnome_amd import contigs
    g, reads = os.path.join(GOLDEN, name), os.path.join(GOLDEN, reads)
    titles = contigs.read_titles(reads)
    text = "##maf version=1\n"
    for k, rid in enumerate(titles):
        strand, start, end, _ = gfa._annotation(titles, rid, reads)
        size = end - start
        text += f"a\ns ref {start} {size} + 248956422 {'ACGT'[k % 4] * size}\ns {rid} 0 {size} {'+' if strand > 0 else '-'} {size} {'ACGT'[k % 4] * size}\n\n"
    path = _write(tmp_path / "sim.maf", text)
    titled = gfa.read_gfa(g, similarity=None, training=True, reads_path=reads)
    got = gfa.read_gfa(g, similarity=None, training=True, maf=path, maf_chr=chrom, maf_parser="device", parser="device")
    host = gfa.read_gfa(g, similarity=None, training=True, maf=path, maf_chr=chrom)
    assert titled["y"] is not None and titled["y"].numel() == titled["src"].numel() > 0 and bool(titled["y"].any())
    for out in (got, host):
        assert out["y"] is not None and torch.equal(out["y"], titled["y"])
        assert all(torch.equal(out[k], titled[k]) for k in ("read_strand", "read_start", "read_end", "read_chr"))
