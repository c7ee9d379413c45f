"""The graphs tests/test_bubble_statement.py and tests/test_bubble_device.py share (no GPU, no torch): a diploid overlap graph from read
positions alone, and hand-made graphs (graph_simplify_statement.build) that sit on the edges of the bubble rule."""
import numpy as np

import graph_simplify_statement as gs

SITES = (8000, 15000, 15600, 22000)
DIPLOID_SEEDS = (1, 2, 4, 5)


def diploid_positions(seed, n_reads=300, genome_len=30000, lo=800, hi=2500):
    """-> (length, start, end, strand +1 / -1, haplotype 0 / 1), drawn in this order from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    length = rng.integers(lo, hi + 1, n_reads)
    start = rng.integers(0, genome_len - length + 1)
    strand = np.where(rng.integers(0, 2, n_reads) == 1, 1, -1)
    hap = rng.integers(0, 2, n_reads)
    return length, start, start + length, strand, hap


def diploid_graph(seed, min_overlap=300, sites=SITES):
    """The overlap graph of a diploid read set from positions alone.  Two reads are compatible when they have the same haplotype or their
    common interval holds none of `sites`.  The edges are overlap_graph_statement.positional_truth's between compatible reads only;
    containment counts only inside a compatible read, and contained reads are dropped (they keep their node numbers and have no edge)."""
    length, start, end, strand, hap = (x.tolist() for x in diploid_positions(seed))
    R = len(start)

    def compatible(i, j):
        a, b = max(start[i], start[j]), min(end[i], end[j])
        return hap[i] == hap[j] or not any(a <= x < b for x in sites)

    inside = lambda j, i: start[i] <= start[j] and end[j] <= end[i] and ((start[i], end[i]) != (start[j], end[j]) or i < j)   # noqa: E731
    contained = [any(i != j and compatible(i, j) and inside(j, i) for i in range(R)) for j in range(R)]
    fwd = [2 * r if strand[r] == 1 else 2 * r + 1 for r in range(R)]
    ov = []
    for i in range(R):
        for j in range(R):
            n = min(end[i], end[j]) - max(start[i], start[j])
            if (i != j and start[i] < start[j] and n >= min_overlap and compatible(i, j) and not contained[i] and not contained[j]
                    and not inside(j, i) and not inside(i, j)):
                ov.append((fwd[i], fwd[j], n))
    return gs.build(length, ov)


def chain(nodes, ol=500):
    """The overlaps of the path nodes[0] -> nodes[1] -> ..; ol: one overlap length for all, or one per edge."""
    ols = [ol] * (len(nodes) - 1) if isinstance(ol, int) else list(ol)
    return [(u, v, o) for u, v, o in zip(nodes, nodes[1:], ols)]


def two_arms(k1=1, k2=3, ol1=500, ol2=500, length=1000, flip=False):
    """Read 0 -> s = read 1 -> two arms of k1 and k2 reads -> t = read 2 -> read 3.  The first arm is reads 4 .., the second the reads after
    them.  flip: every node of every path complemented - the same reads, the bubble built on the other strand, from t ^ 1's side.
    -> (graph, arm 1, arm 2)."""
    a1 = [2 * (4 + i) for i in range(k1)]
    a2 = [2 * (4 + k1 + i) for i in range(k2)]
    paths = [([0, 2], 500), ([4, 6], 500), ([2] + a1 + [4], ol1), ([2] + a2 + [4], ol2)]
    ov = []
    for nodes, ol in paths:
        ols = [ol] * (len(nodes) - 1) if isinstance(ol, int) else list(ol)
        if flip:
            nodes = [v ^ 1 for v in nodes]
        ov += chain(nodes, ols)
    lengths = [length] * (4 + k1 + k2) if isinstance(length, int) else length
    return gs.build(lengths, ov), a1, a2


def no_bubble_graphs():
    """name -> graph: shapes that look like a bubble and are none."""
    frame = chain([0, 2]) + chain([4, 6])
    return {
        "a direct edge beside an arm": gs.build([1000] * 5, frame + chain([2, 8, 4]) + [(2, 4, 100)]),
        "parallel edges into a_1": gs.build([1000] * 6, frame + [(2, 8, 500), (2, 8, 400), (8, 4, 500)] + chain([2, 10, 4])),
        "t == s": gs.build([1000] * 4, chain([0, 2]) + chain([2, 4, 2]) + chain([2, 6, 2])),
        "t == s ^ 1": gs.build([1000] * 4, chain([0, 2]) + chain([2, 4, 3]) + chain([2, 6, 3])),
        "an arm that forks before it joins": gs.build([1000] * 8, frame + chain([2, 8, 4]) + chain([2, 10, 12, 4]) + chain([10, 14])),
        "an arm that ends in out-degree 0": gs.build([1000] * 6, frame + chain([2, 8, 4]) + chain([2, 10])),
        "a circular chain": gs.build([1000] * 4, chain([0, 2, 4, 6, 0])),
    }


def two_bubbles_at_one_source():
    """s = node 2 with three arms into t = node 4 (reads 4, 5, 6; overlaps 500, 520, 510) and two into t' = node 6 (reads 7 and 8, 9)."""
    ov = chain([0, 2]) + chain([4, 20]) + chain([6, 22])
    ov += chain([2, 8, 4], 500) + chain([2, 10, 4], 520) + chain([2, 12, 4], 510)
    ov += chain([2, 14, 6]) + chain([2, 16, 18, 6])
    return gs.build([1000] * 12, ov)


def nested_bubble():
    """s = node 2, t = node 4.  One arm is node 8 alone; the other runs 10 -> (12 | 14, 16) -> 18 with a bubble of its own between nodes 10
    and 18: round 1 pops node 12 (weight 1 against 2), round 2 then sees the arms [8] and [10, 14, 16, 18] and pops node 8.  The distances
    are 0 for [8] and 4000 - 5 * 700 = 500 for the long arm."""
    ov = chain([0, 2]) + chain([4, 6])
    ov += chain([2, 8, 4]) + chain([2, 10], 700) + chain([10, 12, 18], 700) + chain([10, 14, 16, 18], 700) + chain([18, 4], 700)
    return gs.build([1000] * 10, ov)


def hub_bubbles(hub, arms=70, reads=None, sinks=3, step=1):
    """Node `hub` is the source of `arms` arms of one read each, spread over `sinks` sinks in turn; arm i has overlaps 400 + step * i on both
    of its edges, so the last arm of every sink wins and dist = 2000 - 2 * (400 + step * i): with step = 3 the arms more than 166 before
    the winner differ from it by more than the default max_diff and stay.  The other reads' numbers are a permutation, their strands
    random.  -> (graph, arm nodes)."""
    reads = arms + sinks + 1 if reads is None else reads
    rng = np.random.default_rng(7)
    others = np.array([r for r in range(reads) if r != hub >> 1])
    picked = rng.permutation(others)[:arms + sinks]
    node = [2 * int(r) + int(s) for r, s in zip(picked, rng.integers(0, 2, arms + sinks))]
    sink, arm = node[:sinks], node[sinks:]
    ov = []
    for i, a in enumerate(arm):
        ov += [(hub, a, 400 + step * i), (a, sink[i % sinks], 400 + step * i)]
    return gs.build([2000] * reads, ov), arm

