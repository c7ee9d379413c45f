"""The walk checks of utils/analyze.py:1-38 restated in plain Python over lists: the statement the device audit (gnnome_amd/analyze.py,
csrc/walk_audit.hip) is checked against, itself anchored to the text the reference printed (tests/golden/walk_audit.json,
tests/test_walk_audit_statement.py).

The node arrays strand, start, end, chrom are sequences of ints indexed by node id; a walk is a list of node ids.

assert_strand / assert_chromosome (:1-18)
    every node of walk[1:] is compared with walk[0] - not with its predecessor; EVERY node that differs is a finding, not only the
    first switch; the printed `walk index` enumerates walk[1:], so it is one less than the node's position in the walk.
    A finding is (idx, node).
assert_overlap (:21-38)
    over the pairs (walk[i], walk[i+1]), idx = i; the chromosome is not looked at.
    both strands == 1:  a finding when dst_start > src_end, printed `end: {src_end}, start: {dst_start}`
    both strands == -1: a finding when dst_end < src_start, printed `end: {src_start}, start: {dst_end}`
    pairs of unequal strands and strand values other than 1 / -1 are silent; equality is no finding.
    A finding is (idx, src, dst, printed end, printed start).
An empty walk is an IndexError in the reference (walk[0]); the statement says ValueError, as the device audit does.  Node ids are
taken as they are: the statement is only ever given ids in [0, N)."""
import random

RULE = "-" * 20


def strand_findings(strand, walk):
    if not walk:
        raise ValueError("empty walk")
    first = strand[walk[0]]
    return [(idx, node) for idx, node in enumerate(walk[1:]) if strand[node] != first]


def chromosome_findings(chrom, walk):
    if not walk:
        raise ValueError("empty walk")
    first = chrom[walk[0]]
    return [(idx, node) for idx, node in enumerate(walk[1:]) if chrom[node] != first]


def overlap_findings(strand, start, end, walk):
    if not walk:
        raise ValueError("empty walk")
    out = []
    for idx in range(len(walk) - 1):
        src, dst = walk[idx], walk[idx + 1]
        if strand[src] == strand[dst] == 1 and start[dst] > end[src]:
            out.append((idx, src, dst, end[src], start[dst]))
        if strand[src] == strand[dst] == -1 and end[dst] < start[src]:
            out.append((idx, src, dst, start[src], end[dst]))
    return out


def _format_nodes(findings):
    return "".join(f"{RULE}\nwalk index: {idx}\nnode index: {node}\n" for idx, node in findings)


def format_strand(findings):
    """what assert_strand prints for one walk, from strand_findings."""
    return _format_nodes(findings)


def format_chromosome(findings):
    """what assert_chromosome prints for one walk, from chromosome_findings."""
    return _format_nodes(findings)


def format_overlap(findings):
    """what assert_overlap prints for one walk, from overlap_findings."""
    return "".join(f"{RULE}\nwalk index: {idx}\nnodes not connected: {src}, {dst}\nend: {a}, start: {b}\n" for idx, src, dst, a, b in findings)


def statement_audit(strand, start, end, chrom, walks):
    """-> dict: counts [W][3]; strand, chromosome: rows (walk, idx, node); overlap: rows (walk, idx, src, dst, end, start) - each list
    in the order a loop of the reference's calls over the walks prints; text: per walk the three printed texts."""
    counts, s_rows, c_rows, o_rows, text = [], [], [], [], []
    for w, walk in enumerate(walks):
        walk = [int(v) for v in walk]
        if not walk:
            raise ValueError(f"walk {w} is empty")
        s, c, o = strand_findings(strand, walk), chromosome_findings(chrom, walk), overlap_findings(strand, start, end, walk)
        counts.append([len(s), len(c), len(o)])
        s_rows += [(w,) + f for f in s]
        c_rows += [(w,) + f for f in c]
        o_rows += [(w,) + f for f in o]
        text.append((format_strand(s), format_chromosome(c), format_overlap(o)))
    return {"counts": counts, "strand": s_rows, "chromosome": c_rows, "overlap": o_rows, "text": text}


def chain_arrays(num_nodes, strand=1, chrom=1, step=500, length=1000, base=0):
    """Reads laid end over end on one chromosome and strand so that the walk 0, 1, 2, ... has no finding: for strand +1 the starts
    ascend, for -1 they descend; consecutive reads overlap by length - step."""
    strands = [strand] * num_nodes
    chroms = [chrom] * num_nodes
    order = range(num_nodes) if strand == 1 else range(num_nodes - 1, -1, -1)
    starts = [0] * num_nodes
    for k, v in enumerate(order):
        starts[v] = base + k * step
    ends = [s + length for s in starts]
    return strands, starts, ends, chroms


def random_case(seed, num_nodes=3000, num_walks=50, min_len=20, max_len=120, rate=0.1):
    """A seeded graph of `num_nodes` chained + strand reads with about `rate` of the nodes disturbed - a third each: strand flipped
    (to -1, 0 or 2), another chromosome (X = -1 among them), position shifted past the neighbour's end - and `num_walks` walks along
    runs of consecutive node ids.  -> (strand, start, end, chrom, walks)."""
    rng = random.Random(seed)
    strand, start, end, chrom = chain_arrays(num_nodes)
    for v in range(num_nodes):
        if rng.random() >= rate:
            continue
        kind = rng.randrange(3)
        if kind == 0:
            strand[v] = rng.choice([-1, -1, 0, 2])
        elif kind == 1:
            chrom[v] = rng.choice([-1, 2, 7])
        else:
            shift = rng.choice([501, 2000, 1 << 33])
            start[v] += shift
            end[v] += shift
    for v in range(0, num_nodes - 1, 97):   # a few reverse-strand neighbours that do not meet, for the -1 branch
        strand[v] = strand[v + 1] = -1
        start[v + 1], end[v + 1] = start[v] - 3000, start[v] - 1 - (v % 2)
    walks = []
    for _ in range(num_walks):
        n = rng.randint(min_len, max_len)
        a = rng.randrange(0, num_nodes - n)
        walks.append(list(range(a, a + n)))
    return strand, start, end, chrom, walks
