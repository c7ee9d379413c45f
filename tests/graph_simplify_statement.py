"""Overlap-graph simplification, restated in NumPy / plain Python (no GPU, no torch): what gnnome_amd.simplify and csrc/graph_simplify.hip
must reproduce bit for bit.  Integers only.  The graph is a dict that follows the complement convention: node v ^ 1 is the reverse
complement of v, edge (u, v) has the mate (v ^ 1, u ^ 1); p(e) = prefix_length[e].

Transitive edges (`transitive_edges`).  A simultaneous rule on the input graph: edge e = (v, x) is transitive iff there are a node w,
w != v and w != x, and edges e1 = (v, w), e2 = (w, x) with |p(e1) + p(e2) - p(e)| <= fuzz.  Nothing is removed while the rule is applied, so
the order the edges are looked at does not matter.  fuzz is an absolute number of bases: p(e1) + p(e2) - p(e) = len(w) - ol(e1) - ol(e2)
+ ol(e) has the same value for the three mates, so an edge is transitive iff its mate is.

Tips (`tip_nodes`), on the graph restricted to the edges of `keep`.  A tip start is a node s with in-degree 0 and out-degree 1.  From c0 = s
follow the unique out-edge: c0 -> c1 -> ...; the node reached next is looked at in this order: in-degree >= 2 makes it the junction j
and ends the chain; otherwise out-degree != 1 ends it without a junction; otherwise it is the next chain node.  With m chain nodes
c0 .. c(m-1), the chain is a candidate iff it reached a junction and m <= max_tip; its weight is the sum of p over its m edges (the
one into j included).  At a junction with an in-edge that does not come from the last node of one of its candidates, every candidate is a
tip; where all in-edges do, every candidate but one is a tip: the one of the largest weight, ties to the smallest c(m-1), survives.  The
nodes of a tip and their complements are marked.

`simplify_graph`: the transitive edges, then the tips of what is kept, then the edges that are marked or touch a tip node are dropped in
place (relative order kept); compact drops the reads both of whose nodes are left without an edge and renumbers the others 2r', 2r' + 1 in
the old order."""
import numpy as np

EDGE_KEYS = ("overlap_length", "prefix_length", "overlap_similarity", "y")
NODE_KEYS = ("read_length", "read_strand", "read_start", "read_end", "read_chr")


def transitive_edges(g, fuzz=10):
    """-> bool[E]."""
    src, dst, p = (np.asarray(g[f]).tolist() for f in ("src", "dst", "prefix_length"))
    out = {}
    for e, (u, v) in enumerate(zip(src, dst)):
        out.setdefault(u, []).append((v, p[e]))
    mark = np.zeros(len(src), dtype=bool)
    for e, (v, x) in enumerate(zip(src, dst)):
        for w, p1 in out[v]:
            if w == v or w == x:
                continue
            if any(x2 == x and abs(p1 + p2 - p[e]) <= fuzz for x2, p2 in out.get(w, ())):
                mark[e] = True
                break
    return mark


def tip_nodes(g, keep=None, max_tip=4):
    """-> bool[N]."""
    N = int(g["num_nodes"])
    src, dst, p = (np.asarray(g[f]).tolist() for f in ("src", "dst", "prefix_length"))
    live = [True] * len(src) if keep is None else np.asarray(keep).tolist()
    out, inn = [[] for _ in range(N)], [[] for _ in range(N)]
    for e, (u, v) in enumerate(zip(src, dst)):
        if live[e]:
            out[u].append((v, p[e]))
            inn[v].append(u)
    cand = {}                                    # junction -> [(weight, last node, chain)]
    for s in range(N):
        if inn[s] or len(out[s]) != 1:
            continue
        chain, weight, c = [], 0, s
        while True:
            chain.append(c)
            if len(chain) > max_tip:
                break
            nxt, pe = out[c][0]
            weight += pe
            if len(inn[nxt]) >= 2:
                cand.setdefault(nxt, []).append((weight, c, chain))
                break
            if len(out[nxt]) != 1:
                break
            c = nxt
    tip = np.zeros(N, dtype=bool)
    for j, cs in cand.items():
        lasts = {c for _, c, _ in cs}
        survivor = None
        if all(u in lasts for u in inn[j]):
            survivor = min(cs, key=lambda t: (-t[0], t[1]))[1]
        for _, last, chain in cs:
            if last != survivor:
                for c in chain:
                    tip[c] = tip[c ^ 1] = True
    return tip


def mate_closed(src, dst):
    """The edge multiset equals the multiset of its mates."""
    a = sorted(zip(np.asarray(src).tolist(), np.asarray(dst).tolist()))
    b = sorted((v ^ 1, u ^ 1) for u, v in a)
    return a == b


def simplify_graph(g, fuzz=10, max_tip=4, tips=True, compact=True):
    """-> dict of numpy arrays: src, dst, num_nodes, kept_reads, edge_origin, removed, and whichever of EDGE_KEYS, NODE_KEYS, contained
    and reads (data, off) the input carries."""
    N = int(g["num_nodes"])
    src, dst = np.asarray(g["src"]).astype(np.int64), np.asarray(g["dst"]).astype(np.int64)
    trans = transitive_edges(g, fuzz)
    tip = tip_nodes(g, ~trans, max_tip) if tips else np.zeros(N, dtype=bool)
    keep = ~trans & ~tip[src] & ~tip[dst]
    origin = np.nonzero(keep)[0].astype(np.int64)
    src, dst = src[origin], dst[origin]
    touched = np.zeros(N, dtype=bool)
    touched[src] = True
    touched[dst] = True
    has = touched[0::2] | touched[1::2]
    reads = np.nonzero(has)[0].astype(np.int64) if compact else np.arange(N // 2, dtype=np.int64)
    out = {"kept_reads": reads, "edge_origin": origin, "num_nodes": 2 * len(reads),
           "removed": {"transitive_edges": int(trans.sum()), "tip_nodes": int(tip.sum()), "reads": N // 2 - len(reads)}}
    new = np.full(N // 2, -1, dtype=np.int64)
    new[reads] = np.arange(len(reads))
    out["src"], out["dst"] = 2 * new[src >> 1] + (src & 1), 2 * new[dst >> 1] + (dst & 1)
    nodes = np.stack([2 * reads, 2 * reads + 1], 1).reshape(-1)
    for f in EDGE_KEYS:
        if g.get(f) is not None:
            out[f] = np.asarray(g[f])[origin]
    for f in NODE_KEYS:
        if g.get(f) is not None:
            out[f] = np.asarray(g[f])[nodes]
    if g.get("contained") is not None:
        out["contained"] = np.asarray(g["contained"])[reads]
    if g.get("reads") is not None:
        data, off = (np.asarray(t) for t in g["reads"])
        pieces = [data[off[r]:off[r + 1]] for r in reads.tolist()]
        new_off = np.zeros(len(reads) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in pieces], out=new_off[1:])
        out["reads"] = (np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8), new_off)
    return out


def build(read_length, overlaps):
    """A graph dict from read lengths (one per read) and overlaps (u, v, overlap_length): each gives its edge and the mate
    (v ^ 1, u ^ 1) with the same overlap; an overlap that is its own mate gives one edge.  The edges come by source node, then in the
    order given; p = len(src) - overlap, as in an overlap graph, so the residual of the rule is the same on both strands."""
    events = []
    for u, v, ol in overlaps:
        events.append((u, v, ol))
        if (v ^ 1, u ^ 1) != (u, v):
            events.append((v ^ 1, u ^ 1, ol))
    order = sorted(range(len(events)), key=lambda e: (events[e][0], e))
    col = lambda i: np.array([events[e][i] for e in order], dtype=np.int64)   # noqa: E731
    length = np.repeat(np.asarray(read_length, dtype=np.int64), 2)
    src, dst, ol = col(0), col(1), col(2)
    return {"src": src, "dst": dst, "num_nodes": len(length), "overlap_length": ol, "prefix_length": length[src] - ol, "read_length": length}
