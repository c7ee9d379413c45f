"""tests/interval_statement.py against the reference's recorded interval_union results (tests/golden/g14_labels.pt), against the host
function gnnome_amd.labels.interval_union, and on seeded random inputs against a merge written another way (a sweep over sorted end
points).  No GPU."""
import random

import pytest
import torch

import interval_statement as st
from conftest import load_golden
from gnnome_amd import labels

KEYS = ("read_strand", "read_start", "read_end")


def golden_cases():
    return load_golden("g14_labels.pt")["cases"]


def random_reads(rng, n, span, max_len, chroms=(1,)):
    start = [rng.randrange(span) for _ in range(n)]
    return {"read_strand": [rng.choice((1, -1)) for _ in range(n)], "read_start": start,
            "read_end": [s + rng.randrange(max_len + 1) for s in start], "read_chr": [rng.choice(chroms) for _ in range(n)]}


def sweep_union(intervals):
    """The union of closed intervals by counting open intervals over the sorted end points (openings before closings at one point, so
    touching intervals merge): independent of the statement's walk."""
    events = sorted([(s, 0) for s, _ in intervals] + [(e, 1) for _, e in intervals])
    out, depth = [], 0
    for x, closing in events:
        if not closing:
            if depth == 0:
                out.append([x, x])
            depth += 1
        else:
            depth -= 1
            out[-1][1] = max(out[-1][1], x)
    return out


@pytest.mark.parametrize("case", range(3))
def test_statement_reproduces_the_reference(case):
    c = golden_cases()[case]
    got = st.interval_union(*(c[k].tolist() for k in KEYS))
    assert got == c["interval_union"] and len(got) >= 1
    assert got == labels.interval_union({k: c[k] for k in KEYS})


def test_the_multi_golden_has_several_chromosomes_and_the_reference_merges_across_them():
    c = {x["name"]: x for x in golden_cases()}["multi"]
    cols = [c[k].tolist() for k in KEYS]
    chrom = c["read_chr"].tolist()
    assert {-1, -2, -3} <= set(chrom)
    _, s, e, grp = st.select(*cols, chrom)
    rows, heads, per_group = st.islands(s, e, grp)
    assert [r[0] for r in rows] == sorted(r[0] for r in rows) and sum(heads) == len(rows) == sum(n for _, n in per_group.values())
    assert len(rows) >= len(c["interval_union"])   # one line can only merge more
    for code in set(grp):                          # per chromosome the grouped walk is the reference's walk of that chromosome alone
        own = [i for i, x in enumerate(grp) if x == code]
        assert [r[1:] for r in rows if r[0] == code] == [r[1:] for r in st.islands([s[i] for i in own], [e[i] for i in own])[0]]


@pytest.mark.parametrize("seed", range(6))
def test_statement_host_function_and_sweep_agree_on_random_reads(seed):
    rng = random.Random(seed)
    n = rng.choice((1, 2, 17, 300))
    g = random_reads(rng, n, span=rng.choice((5, 40, 20 * n)), max_len=rng.choice((0, 3, 30)), chroms=(3, -2, 7))
    g["read_strand"][0] = 1
    want = st.interval_union(*(g[k] for k in KEYS))
    assert want == labels.interval_union(g) == labels.interval_union({k: torch.tensor(v) for k, v in g.items()})
    _, s, e, grp = st.select(*(g[k] for k in KEYS), g["read_chr"])
    assert want == sweep_union(list(zip(s, e)))
    rows, heads, per_group = st.islands(s, e, grp)
    for code in set(grp):
        mine = [(a, b) for a, b, c in zip(s, e, grp) if c == code]
        assert [r[1:] for r in rows if r[0] == code] == sweep_union(mine)
        assert per_group[code] == [sum(b - a for a, b in sweep_union(mine)), len(sweep_union(mine))]
    cov = st.coverage(*(g[k] for k in KEYS), g["read_chr"])
    assert {c: [v["covered"], v["islands"]] for c, v in cov.items()} == per_group


def test_touching_merges_adjacent_does_not_and_the_running_maximum_decides():
    assert st.islands([0, 10], [10, 20])[0] == [[0, 0, 20]]
    assert st.islands([0, 11], [10, 20])[0] == [[0, 0, 10], [0, 11, 20]]
    # [2, 3] is nested; [9, 12] lies beyond its end but not beyond the running maximum 10
    assert st.islands([0, 2, 9], [10, 3, 12]) == ([[0, 0, 12]], [1, 0, 0], {0: [12, 1]})
    assert st.islands([5, 5, 5], [6, 30, 7])[0] == [[0, 5, 30]]
    assert st.islands([0, 0], [100, 1], [1, 2])[0] == [[1, 0, 100], [2, 0, 1]]   # another group never merges
    with pytest.raises(IndexError):
        st.select([-1, -1], [0, 1], [2, 3])
