"""utils/labels.py:5-20 (interval_union) restated in plain Python on lists, extended with groups - the statement that
tests/test_interval_union_statement.py holds against the reference's recorded results (tests/golden/g14_labels.pt) and the host
function, and that tests/test_interval_union_device.py holds the device result (gnnome_amd.labels.interval_union_device) to.

The reference: collect [start, end] of the strand +1 nodes, sort by start (list.sort: stable), then walk: an interval whose start is <=
the end of the last result merges into it (the end becomes the larger one), any other is appended.  With groups the walk is over
(group, start) order and an interval of another group than the last result's is always appended."""


def select(strand, start, end, chrom=None, want=1):
    """The (node ids, starts, ends, groups) of the nodes whose strand is `want` (None: every node), in node order; group = the
    chromosome code, or 0 for every node when chrom is None.  IndexError when nothing is selected, as intervals[0] gives it."""
    nodes = [i for i, s in enumerate(strand) if want is None or s == want]
    if not nodes:
        raise IndexError("interval_union: nothing selected")
    return (nodes, [start[i] for i in nodes], [end[i] for i in nodes], [0 if chrom is None else chrom[i] for i in nodes])


def islands(start, end, group=None):
    """-> (rows, heads, per_group): rows = [[group, start, end], ...] of the merged intervals in (group, start) order; heads[j] = 1 when
    the j-th interval of that order opened a row; per_group = {group: [covered, count]} with covered = the sum of end - start."""
    group = [0] * len(start) if group is None else group
    order = sorted(range(len(start)), key=lambda i: (group[i], start[i]))   # stable, as list.sort is
    rows, heads = [], []
    for i in order:
        if rows and rows[-1][0] == group[i] and start[i] <= rows[-1][2]:
            rows[-1][2] = max(rows[-1][2], end[i])
            heads.append(0)
        else:
            rows.append([group[i], start[i], end[i]])
            heads.append(1)
    per_group = {}
    for grp, s, e in rows:
        acc = per_group.setdefault(grp, [0, 0])
        acc[0] += e - s
        acc[1] += 1
    return rows, heads, per_group


def interval_union(strand, start, end):
    """The reference's return value: [[start, end], ...] over the strand +1 nodes, one coordinate line."""
    _, s, e, _ = select(strand, start, end)
    return [r[1:] for r in islands(s, e)[0]]


def coverage(strand, start, end, chrom):
    """{chromosome: {"covered", "islands", "longest_island"}} of the strand +1 nodes, merged within each chromosome."""
    _, s, e, grp = select(strand, start, end, chrom)
    out = {}
    for c, a, b in islands(s, e, grp)[0]:
        row = out.setdefault(c, {"covered": 0, "islands": 0, "longest_island": 0})
        row["covered"] += b - a
        row["islands"] += 1
        row["longest_island"] = max(row["longest_island"], b - a)
    return out
