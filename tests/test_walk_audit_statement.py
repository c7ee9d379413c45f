"""The walk-audit statement (tests/walk_audit_statement.py) against the text the reference's utils/analyze.py printed
(tests/golden/walk_audit.json, recorded by tests/golden/make_golden_walk_audit.py), and the parts of gnnome_amd/analyze.py that need
no GPU: the two print-only helpers and the refusal to run without a device."""
import json
import os

import pytest

import walk_audit_statement as st

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_audit.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _arrays(golden):
    n = golden["nodes"]
    return n["read_strand"], n["read_start"], n["read_end"], n["read_chr"]


def test_statement_prints_what_the_reference_printed(golden):
    strand, start, end, chrom = _arrays(golden)
    assert len(golden["walks"]) == len(golden["text"]) >= 10
    for w, (walk, want) in enumerate(zip(golden["walks"], golden["text"])):
        assert st.format_strand(st.strand_findings(strand, walk)) == want["strand"], f"walk {w}: strand"
        assert st.format_chromosome(st.chromosome_findings(chrom, walk)) == want["chromosome"], f"walk {w}: chromosome"
        assert st.format_overlap(st.overlap_findings(strand, start, end, walk)) == want["overlap"], f"walk {w}: overlap"


def test_statement_audit_over_all_walks_agrees_with_the_recorded_text(golden):
    strand, start, end, chrom = _arrays(golden)
    a = st.statement_audit(strand, start, end, chrom, golden["walks"])
    assert [list(t) for t in a["text"]] == [[t["strand"], t["chromosome"], t["overlap"]] for t in golden["text"]]
    for w, t in enumerate(golden["text"]):   # a count is the number of blocks the reference printed
        assert a["counts"][w] == [t[k].count(st.RULE + "\n") for k in ("strand", "chromosome", "overlap")]
    for key in ("strand", "chromosome", "overlap"):
        rows = a[key]
        assert rows == sorted(rows, key=lambda r: (r[0], r[1])) and len(rows) == sum(c[("strand", "chromosome", "overlap").index(key)]
                                                                                       for c in a["counts"])


def test_fixture_covers_every_branch(golden):
    """the cases the fixture is there for, read off the reference's recorded text"""
    strand, start, end, chrom = _arrays(golden)
    walks, text = golden["walks"], golden["text"]
    silent = [not (t["strand"] or t["chromosome"] or t["overlap"]) for t in text]
    assert any(s and len(w) > 1 for s, w in zip(silent, walks)), "a clean walk"
    assert any(s and len(w) == 1 for s, w in zip(silent, walks)), "a walk of one node prints nothing"
    # strand differs at two later nodes with an agreeing node between them: both reported, so the comparison is with walk[0]
    assert any(t["strand"].count("walk index") == 2 and strand[w[2]] == strand[w[0]] != strand[w[1]] for w, t in zip(walks, text) if len(w) >= 4)
    assert any("node index" in t["chromosome"] and -1 in {chrom[v] for v in w} for w, t in zip(walks, text)), "a switch to X = -1"

    def pair_case(sign, delta, finding):
        for w, t in zip(walks, text):
            if len(w) == 2 and strand[w[0]] == strand[w[1]] == sign:
                gap = start[w[1]] - end[w[0]] if sign == 1 else start[w[0]] - end[w[1]]
                if gap == delta and bool(t["overlap"]) == finding:
                    return True
        return False

    assert pair_case(1, 0, False) and pair_case(1, 1, True), "+ pairs: dst_start == src_end silent, src_end + 1 a finding"
    assert pair_case(-1, 0, False) and pair_case(-1, 1, True), "- pairs: dst_end == src_start silent, src_start - 1 a finding"
    assert any(len(w) == 2 and strand[w[0]] == -strand[w[1]] and start[w[1]] > end[w[0]] and not t["overlap"] for w, t in zip(walks, text)), \
        "a mixed-strand pair with a gap is silent"
    assert any({0, 2} <= {strand[v] for v in w} and not t["overlap"] and t["strand"] for w, t in zip(walks, text)), "strands 0 and 2"
    assert any(max(start[v] for v in w) > 2 ** 32 and t["overlap"] for w, t in zip(walks, text)), "positions beyond 2^32"


def test_statement_refuses_an_empty_walk(golden):
    strand, start, end, chrom = _arrays(golden)
    with pytest.raises(ValueError, match="walk 1 is empty"):
        st.statement_audit(strand, start, end, chrom, [[0, 1], [], [2]])


def test_print_helpers_print_what_the_reference_printed(golden, capsys):
    import torch
    from gnnome_amd import analyze
    info = golden["helpers"]["graph_info"]
    graph = type("G", (), {"num_nodes": lambda self: info["num_nodes"],
                           "edges": lambda self: (torch.tensor(info["edges"][0]), torch.tensor(info["edges"][1]))})()
    capsys.readouterr()
    analyze.print_graph_info(info["idx"], graph)
    assert capsys.readouterr().out == info["text"]
    for step in golden["helpers"]["prediction"]:
        analyze.print_prediction(step["walk"], step["current"], {int(k): v for k, v in step["neighbors"].items()},
                                 torch.tensor(step["actions"], dtype=torch.float64), step["choice"], step["best_neighbor"])
        assert capsys.readouterr().out == step["text"]


def test_audit_without_a_gpu_is_a_runtime_error(golden, monkeypatch):
    import torch
    from gnnome_amd import analyze
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    n = golden["nodes"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        analyze.audit_walks(n, golden["walks"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        analyze.assert_overlap(n, golden["walks"][0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        analyze.audit_walks(n, golden["walks"], device="cpu")


def test_random_case_finds_each_kind_often_enough():
    strand, start, end, chrom, walks = st.random_case(seed=5)
    a = st.statement_audit(strand, start, end, chrom, walks)
    totals = [sum(c[k] for c in a["counts"]) for k in range(3)]
    assert len(walks) == 50 and len(strand) == 3000 and min(totals) >= 20, totals
    assert any(r[4] - r[5] == 1 or r[4] > r[5] for r in a["overlap"] if strand[r[2]] == -1), "a - strand finding among them"
