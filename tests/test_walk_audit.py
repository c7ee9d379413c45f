"""The device walk audit (gnnome_amd/analyze.py, csrc/walk_audit.hip) against its statement (tests/walk_audit_statement.py) on the
same inputs, and through the statement against the text the reference's utils/analyze.py printed (tests/golden/walk_audit.json).
Everything is compared exactly: counts, the three finding lists with their columns, and the text of every walk."""
import json
import os

import pytest
import torch

import walk_audit_statement as st

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_audit.json")


def graph_of(strand, start, end, chrom):
    return {"read_strand": torch.tensor(strand, dtype=torch.int64), "read_start": torch.tensor(start, dtype=torch.int64),
            "read_end": torch.tensor(end, dtype=torch.int64), "read_chr": torch.tensor(chrom, dtype=torch.int64)}


def rows_of(found):
    return [tuple(r) for r in torch.stack(list(found), 1).cpu().tolist()] if found.walk.numel() else []


def check(strand, start, end, chrom, walks):
    """audit on the device == the statement; -> (the audit, the statement's result)"""
    from gnnome_amd import analyze
    want = st.statement_audit(strand, start, end, chrom, walks)
    got = analyze.audit_walks(graph_of(strand, start, end, chrom), walks)
    assert got.counts.dtype == torch.int32 and got.counts.is_cuda and tuple(got.counts.shape) == (len(walks), 3)
    assert got.counts.cpu().tolist() == want["counts"]
    assert rows_of(got.strand) == want["strand"]
    assert rows_of(got.chromosome) == want["chromosome"]
    assert rows_of(got.overlap) == want["overlap"]
    for i in range(len(walks)):
        assert tuple(got.text(i)) == want["text"][i], f"walk {i}"
    return got, want


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_walks_device_statement_and_reference_agree(golden):
    n = golden["nodes"]
    got, _ = check(n["read_strand"], n["read_start"], n["read_end"], n["read_chr"], golden["walks"])
    for i, t in enumerate(golden["text"]):
        assert got.text(i) == (t["strand"], t["chromosome"], t["overlap"]), f"walk {i}"


def disturbed_chain(num_nodes, every=7):
    """a + chain on chromosome 1 in which every `every`-th node (not node 0) sits on strand -1 and chromosome 3 - a strand and a
    chromosome finding against a + first node - and every node 3 mod `every` starts one base past its predecessor's end: an overlap
    finding for the pair that ends there when both are +"""
    strand, start, end, chrom = st.chain_arrays(num_nodes)
    for v in range(every, num_nodes, every):
        strand[v], chrom[v] = -1, 3
    for v in range(3, num_nodes, every):            # v - 1 and v are both +: move v past v - 1's end
        start[v], end[v] = end[v - 1] + 1, end[v - 1] + 1001
        for u in range(v + 1, min(v + 3, num_nodes)):   # and keep its successors in touch with it
            start[u], end[u] = start[v] + 100 * (u - v), end[v] + 100 * (u - v)
    return strand, start, end, chrom


def test_walk_borders_inside_a_wavefront_on_its_border_and_across_workgroups():
    strand, start, end, chrom = disturbed_chain(600, every=5)
    walks, at = [], 0
    for n in (1, 2, 63, 64, 65, 257):               # 452 positions: two workgroups of 256
        walks.append(list(range(at, at + n)))
        at += n
    _, want = check(strand, start, end, chrom, walks)
    assert all(sum(c) > 0 for c in want["counts"][2:]) and want["counts"][0] == [0, 0, 0]


def test_two_hundred_walks_of_one_node_share_wavefronts_and_count_nothing():
    strand, start, end, chrom = disturbed_chain(400, every=3)
    got, want = check(strand, start, end, chrom, [[v] for v in range(0, 400, 2)])
    assert len(got) == 200 and int(got.counts.abs().sum()) == 0 and not want["strand"] and not want["overlap"]


def test_one_long_walk_is_summed_over_several_workgroups():
    strand, start, end, chrom = disturbed_chain(5000, every=7)
    got, want = check(strand, start, end, chrom, [list(range(5000))])
    assert want["counts"][0][0] == want["counts"][0][1] == len(range(7, 5000, 7)) and want["counts"][0][2] >= 5000 // 7 - 1


def test_findings_at_the_first_and_at_the_last_pair():
    strand, start, end, chrom = st.chain_arrays(70)
    start[1], end[1] = end[0] + 1, end[0] + 1001    # pair (0, 1)
    for v in range(2, 69):                          # the chain between them hangs on node 1
        start[v], end[v] = start[1] + 10 * v, end[1] + 10 * v
    start[69], end[69] = end[68] + 1, end[68] + 1001  # pair (68, 69)
    _, want = check(strand, start, end, chrom, [list(range(70))])
    assert [r[1] for r in want["overlap"]] == [0, 68]


def test_last_position_of_a_walk_does_not_look_into_the_next_walk():
    # walk 0 ends at node 2, walk 1 starts at node 3, and (2, 3) would be an overlap finding; walk 1's first node also differs in
    # strand and chromosome from walk 0's - nothing of it belongs to either walk
    strand = [1, 1, 1, 1, 1, -1, -1]
    start = [0, 500, 1000, 9000, 9500, 700, 100]
    end = [1000, 1500, 2000, 10000, 10500, 1700, 650]
    chrom = [1, 1, 1, 1, 1, 2, 2]
    got, want = check(strand, start, end, chrom, [[0, 1, 2], [3, 4], [5], [6]])
    assert want["counts"] == [[0, 0, 0]] * 4
    _, want = check(strand, start, end, chrom, [[0, 1, 2, 3, 4], [5, 6]])   # the same nodes, joined: now they are findings
    assert want["counts"] == [[0, 0, 1], [0, 0, 1]]


def test_positions_above_two_to_the_32_stay_whole():
    big = 1 << 32
    strand = [1, 1, 1, -1, -1]
    start = [big + 5, 5 + 2000, 2 * big + 1006, 3 * big + 10, 10 - 500]   # equal low words, different high words
    end = [big + 1005, 5 + 3000, 2 * big + 2006, 3 * big + 500, 9]
    chrom = [1, 1, 1, 1, 1]
    _, want = check(strand, start, end, chrom, [[1, 0, 2], [0, 1], [3, 4], [4, 3]])
    assert want["overlap"] == [(0, 0, 1, 0, 5 + 3000, big + 5), (0, 1, 0, 2, big + 1005, 2 * big + 1006), (2, 0, 3, 4, 3 * big + 10, 9)]


def test_strands_zero_and_two_are_silent_pairs_and_reported_against_the_first_node():
    strand = [1, 0, 0, 2, 2, 1, 0]
    start = [0, 5000, 90000, 200000, 400000, 500, 100]
    end = [1000, 6000, 91000, 201000, 401000, 1500, 1100]
    chrom = [1] * 7
    _, want = check(strand, start, end, chrom, [[0, 1, 2, 3, 4, 5], [6, 1, 2, 0, 3]])
    assert want["counts"] == [[4, 0, 0], [2, 0, 0]]


@pytest.mark.parametrize("seed", [1, 2])
def test_random_graphs(seed):
    strand, start, end, chrom, walks = st.random_case(seed)
    _, want = check(strand, start, end, chrom, walks)
    totals = [sum(c[k] for c in want["counts"]) for k in range(3)]
    assert len(strand) == 3000 and len(walks) == 50 and min(totals) >= 20, totals


def test_no_walks_give_empty_results():
    from gnnome_amd import analyze
    strand, start, end, chrom = st.chain_arrays(4)
    got = analyze.audit_walks(graph_of(strand, start, end, chrom), [])
    assert len(got) == 0 and tuple(got.counts.shape) == (0, 3) and got.counts.is_cuda
    assert all(col.numel() == 0 and col.is_cuda for found in (got.strand, got.chromosome, got.overlap) for col in found)
    with pytest.raises(IndexError):
        got.text(0)


def test_entry_returns_without_a_launch_when_there_is_nothing_to_do():
    import ctypes
    from gnnome_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    # every pointer is NULL: a launch (or the pointer check in front of one) could not succeed
    assert lib.gnnome_walk_audit(null, null, null, 0, 0, null, null, null, null, 5, null, null, null) == 0
    assert lib.gnnome_walk_audit(null, null, null, 3, 0, null, null, null, null, 5, null, null, null) == 0
    assert lib.gnnome_walk_audit(null, null, null, 0, 7, null, null, null, null, 5, null, null, null) == 0
    assert lib.gnnome_walk_audit(null, null, null, -1, 7, null, null, null, null, 5, null, null, null) < 0
    assert b"walk_audit" in lib.gnnome_last_error()


def test_empty_walk_among_others_is_named():
    from gnnome_amd import analyze
    g = graph_of(*st.chain_arrays(6))
    with pytest.raises(ValueError, match="walk 2 is empty"):
        analyze.audit_walks(g, [[0, 1], [2], [], [3, 4]])


@pytest.mark.parametrize("bad", [6, -1])
def test_node_id_out_of_range_raises_and_leaves_the_device_usable(bad):
    from gnnome_amd import analyze
    arrays = st.chain_arrays(6)
    g = graph_of(*arrays)
    with pytest.raises(IndexError, match=f"walk 1: node {bad} "):
        analyze.audit_walks(g, [[0, 1], [2, bad, 3], [4, 5]])
    with pytest.raises(IndexError, match=f"walk 0: node {bad} at position 0"):   # as the walk's first node, which every position reads
        analyze.audit_walks(g, [[bad, 1, 2]])
    torch.cuda.synchronize()
    check(*arrays, [[0, 1], [2, 3], [4, 5]])


def test_graph_without_an_array_is_named():
    from gnnome_amd import analyze
    g = graph_of(*st.chain_arrays(6))
    del g["read_end"]
    with pytest.raises(KeyError, match="read_end"):
        analyze.audit_walks(g, [[0, 1]])
    with pytest.raises(KeyError, match="read_strand"):
        analyze.audit_walks(type("G", (), {"ndata": {}})(), [[0, 1]])


def test_drop_in_functions_print_the_text_of_the_walk(golden, capsys):
    from gnnome_amd import analyze
    n = golden["nodes"]
    g = graph_of(n["read_strand"], n["read_start"], n["read_end"], n["read_chr"])
    dgl_like = type("G", (), {"ndata": g})()
    audit = analyze.audit_walks(g, golden["walks"])
    printed_any = False
    for i, walk in enumerate(golden["walks"]):
        for graph in (g, dgl_like):
            for fn, want in zip((analyze.assert_strand, analyze.assert_chromosome, analyze.assert_overlap), audit.text(i)):
                capsys.readouterr()
                fn(graph, walk)
                out = capsys.readouterr().out
                assert out == want, f"walk {i}: {fn.__name__}"
                printed_any |= bool(out)
    assert printed_any


def test_walk_report_sums_the_statements_counts():
    from gnnome_amd import pipeline
    strand, start, end, chrom, walks = st.random_case(3)
    want = st.statement_audit(strand, start, end, chrom, walks)["counts"]
    report = pipeline.walk_report(graph_of(strand, start, end, chrom), walks)
    kinds = ("strand", "chromosome", "overlap")
    assert report == {"walks": 50, **{k: sum(c[i] for c in want) for i, k in enumerate(kinds)},
                      **{"walks_with_" + k: sum(c[i] > 0 for c in want) for i, k in enumerate(kinds)}}
    assert min(report[k] for k in kinds) >= 20
