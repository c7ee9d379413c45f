"""gnnome_amd.labels.interval_union_device / reference_coverage (csrc/interval_union.hip) against tests/interval_statement.py, the
plain-Python restatement of utils/labels.py:5-20 that tests/test_interval_union_statement.py ties to the reference's recorded results.
The data are integers: every comparison is exact.  T is the exported tile size; the cases sit on its edges."""
import ctypes
import os
import random

import pytest
import torch

import interval_statement as st
from conftest import GOLDEN, load_golden
from gnnome_amd import _lib, labels, pipeline, trainer

gpu = pytest.mark.gpu


def tile():
    return labels.interval_union_tile_size()


def graph(start, end, strand=None, chrom=None):
    n = len(start)
    return {"read_strand": torch.tensor(strand if strand is not None else [1] * n, dtype=torch.int64),
            "read_start": torch.tensor(start, dtype=torch.int64), "read_end": torch.tensor(end, dtype=torch.int64),
            "read_chr": torch.tensor(chrom if chrom is not None else [1] * n, dtype=torch.int64)}


def check(g, by="all", strand=1):
    """The device result of g equals the statement in every field -> (IntervalUnion, statement rows)."""
    cols = [g[k].tolist() for k in ("read_strand", "read_start", "read_end")]
    _, s, e, grp = st.select(*cols, g["read_chr"].tolist() if by == "chr" else None, want=strand)
    rows, heads, per_group = st.islands(s, e, grp)
    u = labels.interval_union_device(g, by=by, strand=strand)
    assert u.group.dtype == torch.int32 and u.start.dtype == u.end.dtype == u.covered.dtype == torch.int64 and u.start.is_cuda
    assert len(u) == len(rows)
    assert u.group.tolist() == [r[0] for r in rows]
    assert torch.equal(u.start.cpu(), torch.tensor([r[1] for r in rows], dtype=torch.int64))
    assert torch.equal(u.end.cpu(), torch.tensor([r[2] for r in rows], dtype=torch.int64))
    assert u.head.tolist() == heads
    codes = sorted(per_group)
    assert u.groups.tolist() == codes
    assert u.covered.tolist() == [per_group[c][0] for c in codes] and u.count.tolist() == [per_group[c][1] for c in codes]
    assert u.tolist() == ([r[1:] for r in rows] if by == "all" else rows)
    return u, rows


def random_graph(seed, n, span=None, max_len=40, chroms=(1,), offset=0):
    rng = random.Random(seed)
    span = span or 20 * n
    start = [offset + rng.randrange(span) for _ in range(n)]
    return graph(start, [s + rng.randrange(max_len + 1) for s in start], [rng.choice((1, -1)) for _ in range(n)],
                 [rng.choice(chroms) for _ in range(n)])


# ---- the reference's recorded results ----------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("case", range(3))
def test_golden_cases_equal_the_reference(case):
    c = load_golden("g14_labels.pt")["cases"][case]
    g = {k: c[k] for k in ("read_strand", "read_start", "read_end", "read_chr")}
    assert labels.interval_union_device(g).tolist() == c["interval_union"] == labels.interval_union(g)
    check(g)
    check(g, by="chr")


# ---- sizes on the tile edges --------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("which", range(7))
def test_random_intervals_at_tile_edge_sizes(which):
    T = tile()
    n = (1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5)[which]
    g = random_graph(which, n)
    g["read_strand"][:] = 1
    u, rows = check(g)
    assert n < 3 or 1 < len(rows) < n          # the draw merges some and not all
    check(g, by="chr")
    check(random_graph(100 + which, n, chroms=(4, -1, 9)), by="chr", strand=None)


@gpu
def test_one_long_first_interval_carries_across_whole_tiles():
    T = tile()
    n = 3 * T + 7
    rng = random.Random(1)
    start = [0] + sorted(rng.randrange(1, 10 ** 6) for _ in range(n - 1))
    end = [10 ** 9] + [s + rng.randrange(50) for s in start[1:]]
    u, rows = check(graph(start, end))
    assert rows == [[0, 0, 10 ** 9]] and u.head.sum().item() == 1 and u.covered.tolist() == [10 ** 9] and u.count.tolist() == [1]


@gpu
def test_all_disjoint_every_interval_is_a_head():
    T = tile()
    n = 3 * T
    u, rows = check(graph([10 * i for i in range(n)], [10 * i + 5 for i in range(n)]))
    assert len(rows) == n and u.count.tolist() == [n] and u.covered.tolist() == [5 * n]
    head = u.head.tolist()
    assert all(head[t * T] == 1 and head[t * T + T - 1] == 1 for t in range(3)) and sum(head) == n


@gpu
@pytest.mark.parametrize("where", ["middle", "straddle"])
def test_touching_merges_adjacent_splits(where):
    """A chain of touching intervals [10 i, 10 i + 10] with one long interval before position p that sets the running maximum X and a
    short nested one at p - 1; the interval at p starts at X (merges) or X + 1 (splits).  p in the middle of the second tile, or at its
    first slot so that the pair (p - 1, p) straddles the tile boundary."""
    T = tile()
    n = 2 * T + 9
    p = T + T // 2 if where == "middle" else T
    for gap, islands in ((0, 1), (1, 2)):
        start, end = [10 * i for i in range(n)], [10 * i + 10 for i in range(n)]
        X = end[p - 2] + 1000
        end[p - 2] = X
        end[p - 1] = start[p - 1] + 1           # nested, far below X: the gap to ITS end must not split
        for i in range(p, n):                    # the rest of the chain moves behind X
            start[i], end[i] = X + gap + 10 * (i - p), X + gap + 10 * (i - p) + 10
        u, rows = check(graph(start, end))
        assert len(rows) == islands and u.head[p].item() == gap and u.head[p - 1].item() == 0
        assert rows[0][2] == (end[-1] if gap == 0 else X)


@gpu
def test_equal_starts_and_nested_intervals():
    check(graph([5, 5, 5, 20, 20, 40], [6, 30, 7, 21, 25, 40]))
    # nested [2, 3] then [9, 12]: beyond the nested end, not beyond the running maximum 10 -> one island [0, 12]
    u, rows = check(graph([0, 2, 9, 13], [10, 3, 12, 13]))
    assert rows == [[0, 0, 12], [0, 13, 13]]
    T = tile()
    g = random_graph(7, 2 * T + 3, span=50, max_len=3)     # many equal starts, in every tile
    g["read_start"] += torch.arange(2 * T + 3) // 7 * 3
    g["read_end"] = g["read_start"] + torch.arange(2 * T + 3) % 5
    check(g, strand=None)


@gpu
@pytest.mark.parametrize("offset", [(1 << 31) + 5, (1 << 33) + 1, (1 << 62) - (1 << 20)])
def test_large_positions(offset):
    T = tile()
    u, rows = check(random_graph(3, T + 9, offset=offset), strand=None)
    assert rows[0][1] >= offset and 1 < len(rows)
    check(random_graph(4, T + 9, offset=offset, chroms=(2, 5)), by="chr", strand=None)


# ---- groups -------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_group_boundary_at_and_beside_a_tile_boundary(shift):
    """Chromosome -3 fills the first T + shift sorted slots and ends far out (10^12); chromosome -2 is one interval; chromosome -1 starts
    again near 0: a maximum that leaked across a group start would swallow it whole.  Codes are negative and unsorted in node order."""
    T = tile()
    n1, n3 = T + shift, T + 5
    rng = random.Random(shift)
    chrom = [-3] * n1 + [-2] + [-1] * n3
    start = [rng.randrange(10 ** 6) for _ in range(n1)] + [7] + [rng.randrange(20 * n3) for _ in range(n3)]
    end = [s + rng.randrange(40) for s in start]
    end[0] = 10 ** 12
    perm = list(range(len(chrom)))
    rng.shuffle(perm)
    g = graph([start[i] for i in perm], [end[i] for i in perm], chrom=[chrom[i] for i in perm])
    u, rows = check(g, by="chr")
    assert u.groups.tolist() == [-3, -2, -1] and u.count[1].item() == 1 and u.count[2].item() > 1
    assert u.head[n1].item() == 1 and u.head[n1 + 1].item() == 1
    check(g)    # and on one line the long interval does swallow the rest, as the reference has it


# ---- strands, refusals, determinism ----------------------------------------------------------------------------------------------

@gpu
def test_strand_minus_one_and_both():
    T = tile()
    g = random_graph(11, T + 40, chroms=(1, 2))
    for strand in (1, -1, None):
        check(g, strand=strand)
        check(g, by="chr", strand=strand)
    assert len(labels.interval_union_device(g, strand=None).head) == T + 40


@gpu
def test_refusals_before_any_launch():
    g = graph([0, 5], [3, 9], strand=[-1, -1])
    with pytest.raises(IndexError, match=r"interval_union: no strand \+1 node"):
        labels.interval_union_device(g)
    with pytest.raises(IndexError, match=r"interval_union: no strand \+1 node"):
        labels.interval_union(g)               # the host function's text
    with pytest.raises(IndexError, match="no strand -1 node"):
        labels.interval_union_device(graph([0], [1]), strand=-1)
    bad = graph([0, 5, 9, 4], [3, 9, 8, 2], strand=[1, -1, 1, 1])
    with pytest.raises(ValueError, match="node 2 ends at 8, before its start 9"):
        labels.interval_union_device(bad)
    labels.interval_union_device(bad, strand=-1)   # the bad reads are not selected
    short = graph([0, 5], [3, 9])
    short["read_end"] = short["read_end"][:1]
    with pytest.raises(ValueError, match="read_end has 1 entries"):
        labels.interval_union_device(short)
    with pytest.raises(ValueError, match="by="):
        labels.interval_union_device(g, by="strand")


def test_entry_argument_checks_launch_nothing():
    lib = _lib.load()
    one, res, need = ctypes.c_void_p(16), (ctypes.c_int64 * 2)(7, 7), ctypes.c_size_t(0)
    assert lib.gnnome_interval_union(None, None, None, 0, None, None, None, None, 0, None, None, None, res, None, 0, None) == 0
    assert list(res) == [0, 0]                                       # M = 0: K = 0, no launch
    T = ctypes.c_int(0)
    assert lib.gnnome_interval_union_tile_size(ctypes.byref(T)) == 0 and T.value >= 64 and T.value % 64 == 0
    assert lib.gnnome_interval_union_workspace_bytes(3 * T.value + 5, ctypes.byref(need)) == 0 and need.value >= 4 * 16
    args = lambda ws, nbytes, M=5, start=one: (start, one, one, M, one, one, one, one, 1, one, one, one, res, ws, nbytes, None)  # noqa: E731
    assert lib.gnnome_interval_union(*args(one, need.value - 1, M=3 * T.value + 5)) == -3 and b"workspace" in lib.gnnome_last_error()
    assert lib.gnnome_interval_union(*args(None, 1 << 20)) == -1 and b"null workspace" in lib.gnnome_last_error()
    assert lib.gnnome_interval_union(*args(one, 1 << 20, start=None)) == -1 and b"null" in lib.gnnome_last_error()
    assert lib.gnnome_interval_union(*args(one, 1 << 20, M=1 << 31)) == -1 and b"2^31" in lib.gnnome_last_error()
    assert lib.gnnome_interval_union_workspace_bytes(1 << 31, ctypes.byref(need)) == -1
    with pytest.raises(_lib.GnnomeHipError):
        _lib.check(-3, "interval_union")


@gpu
def test_same_input_same_bits_and_node_order_does_not_matter():
    T = tile()
    g = random_graph(21, 3 * T + 5, chroms=(-1, -2, -3))
    a, b = (labels.interval_union_device(g, by="chr") for _ in range(2))
    for name in ("group", "start", "end", "groups", "covered", "count", "head"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    perm = torch.randperm(3 * T + 5, generator=torch.Generator().manual_seed(5))
    c = labels.interval_union_device({k: v[perm] for k, v in g.items()}, by="chr")
    for name in ("group", "start", "end", "groups", "covered", "count"):
        assert torch.equal(getattr(a, name), getattr(c, name)), name


# ---- the reports --------------------------------------------------------------------------------------------------------------

@gpu
def test_reference_coverage_on_the_multi_golden():
    c = {x["name"]: x for x in load_golden("g14_labels.pt")["cases"]}["multi"]
    g = {k: c[k] for k in ("read_strand", "read_start", "read_end", "read_chr")}
    want = st.coverage(*(g[k].tolist() for k in ("read_strand", "read_start", "read_end", "read_chr")))
    assert len(want) >= 2
    rep = labels.reference_coverage(g)
    assert rep["chromosomes"] == want and list(rep["chromosomes"]) == sorted(want) and "fraction" not in rep
    for key in ("covered", "islands"):
        assert rep[key] == sum(v[key] for v in want.values())
    assert rep["longest_island"] == max(v["longest_island"] for v in want.values())
    ref = {code: 3 * v["covered"] + 11 for code, v in want.items()}
    ref[99] = 1000                                     # a chromosome without reads still counts in the total
    rep = pipeline.coverage_report(g, ref_length=ref)
    for code, v in want.items():
        assert rep["chromosomes"][code] == dict(v, fraction=v["covered"] / ref[code])
    assert rep["fraction"] == rep["covered"] / sum(ref.values())
    assert pipeline.coverage_report(g, ref_length=12345)["fraction"] == rep["covered"] / 12345
    with pytest.raises(ValueError, match="no entry for chromosome"):
        labels.reference_coverage(g, ref_length={99: 5})


@gpu
def test_trainer_process_coverage_switch(tmp_path):
    from gnnome_amd import gfa
    paths = os.path.join(GOLDEN, "g14_multi.gfa"), os.path.join(GOLDEN, "g14_multi.fasta")
    plain = trainer.process(*paths, str(tmp_path / "a" / "0.pt"))
    again = trainer.process(*paths, str(tmp_path / "b" / "0.pt"), coverage=False)
    with_cov = trainer.process(*paths, str(tmp_path / "c" / "0.pt"), coverage=True)
    read = gfa.read_gfa(paths[0], reads_path=paths[1], training=True, labels=False)
    assert list(plain) == list(again) and set(plain) == set(read) | {"in_deg", "out_deg"}   # the keys of the parent commit
    assert (tmp_path / "a" / "0.pt").read_bytes() == (tmp_path / "b" / "0.pt").read_bytes()
    assert list(with_cov) == list(plain) + ["coverage"]
    saved = torch.load(str(tmp_path / "c" / "0.pt"), weights_only=False)
    assert saved["coverage"] == labels.reference_coverage(plain) and list(saved) == list(with_cov)
    for k, v in plain.items():
        assert (torch.equal(v, saved[k]) if isinstance(v, torch.Tensor) else v == saved[k]), k
