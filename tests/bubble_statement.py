"""Simple bubbles of an overlap graph, restated in NumPy / plain Python (no GPU, no torch): what gnnome_amd.bubbles and csrc/bubbles.hip must
reproduce bit for bit.  Integers only.  The graph is a dict that follows the complement convention - node v ^ 1 is the reverse complement
of v, edge (u, v) has the mate (v ^ 1, u ^ 1) - restricted to the edges of `keep`; what is kept is closed under mates and has
p(e) = read_length[src] - overlap_length (both checked by unitig_statement.columns: ValueError).  Degrees count parallel edges.

Arm.  A chain a_1 .. a_k (k >= 1) of unitig_statement.unitig_chains on the kept edges that is not circular, whose head has in-degree 1 and
whose tail has out-degree 1 - every node of it then has in-degree 1 and out-degree 1 - whose one in-edge comes from a node s of out-degree
>= 2, whose one out-edge goes to a node t of in-degree >= 2, with t != s and t != s ^ 1.  s -> a_1 and a_k -> t are no links, so an arm is
one whole chain; a direct edge s -> t is no arm (that is the transitive rule's case), and parallel edges s -> a_1 make a_1 a join.

Figures, equal for an arm and for its mate arm a_k ^ 1 .. a_1 ^ 1 from t ^ 1 to s ^ 1: weight = the sum of weight[a_i] (a column with
weight[v] == weight[v ^ 1], else ValueError; default 1 per node); overlap = the sum of overlap_length over the arm's k + 1 edges; dist =
the sum of read_length[a_i] - overlap, the bases between the end of s and the start of t (it may be negative).

Bubble.  The arms that share (s, t), when there are at least two.  The winner has the largest (weight, overlap, -min(a_1, a_k ^ 1)); the
last component is equal for an arm and its mate and differs between two arms of one bubble.  Another arm of the bubble is a loser iff
dist(winner) <= max_dist, dist(arm) <= max_dist and |dist(arm) - dist(winner)| <= max_diff.  `bubble_nodes` marks the nodes of every loser
and their complements; all bubbles are judged on the input at once.  s and t are no arm nodes and arms are disjoint, so the mark is the
same on both strands, the kept edges stay closed under mates and s still reaches t.

Rounds (`pop_bubbles`).  A round marks, and the edges at marked nodes are dropped; the next round judges what is kept.  Rounds repeat until
one marks nothing or `rounds` of them have run: a bubble inside an arm of another goes first and leaves a longer plain arm."""
import numpy as np

import graph_simplify_statement as gs
import unitig_statement as us

ARM_KEYS = ("first", "last", "source", "sink", "nodes", "weight", "overlap", "dist")


def restrict(g, keep):
    """The graph of the kept edges (keep bool[E]; None: all), with the columns the rule reads."""
    sel = slice(None) if keep is None else np.asarray(keep, dtype=bool)
    out = {f: np.asarray(g[f]).astype(np.int64)[sel] for f in ("src", "dst", "prefix_length", "overlap_length")}
    out.update(num_nodes=int(g["num_nodes"]), read_length=np.asarray(g["read_length"]).astype(np.int64))
    return out


def node_weight(weight, N):
    if weight is None:
        return [1] * N
    w = np.asarray(weight)
    if w.dtype.kind not in "iu" or w.shape != (N,) or not np.array_equal(w[0::2], w[1::2]):
        raise ValueError("weight: an int column with one entry per node and weight[v] == weight[v ^ 1]")
    return w.tolist()


def arm_list(g, keep=None, weight=None):
    """-> the arms as dicts of Python ints (ARM_KEYS and `chain`, the list of nodes), in ascending order of their first node."""
    h = restrict(g, keep)
    N, src, dst, p, ol, rl = us.columns(h)
    w = node_weight(weight, N)
    c = us.unitig_chains(h)
    out_deg, in_deg, in_edge, out_edge = [0] * N, [0] * N, {}, {}
    for e, (u, v) in enumerate(zip(src, dst)):
        out_deg[u] += 1
        in_deg[v] += 1
        out_edge[u], in_edge[v] = e, e                          # read only where the degree is 1
    off, nodes = c["chain_off"].tolist(), c["chain_nodes"].tolist()
    arms = []
    for j in range(len(off) - 1):
        chain = nodes[off[j]:off[j + 1]]
        first, last = chain[0], chain[-1]
        if c["circular"][j] or in_deg[first] != 1 or out_deg[last] != 1:
            continue
        e_in, e_out = in_edge[first], out_edge[last]
        s, t = src[e_in], dst[e_out]
        if out_deg[s] < 2 or in_deg[t] < 2 or t == s or t == s ^ 1:
            continue
        overlap = ol[e_in] + ol[e_out] + sum(ol[out_edge[a]] for a in chain[:-1])
        arms.append({"first": first, "last": last, "source": s, "sink": t, "nodes": len(chain), "weight": sum(w[a] for a in chain),
                     "overlap": overlap, "dist": sum(rl[a] for a in chain) - overlap, "chain": chain})
    return sorted(arms, key=lambda a: a["first"])


def bubble_arms(g, keep=None, weight=None):
    """-> dict of int64 arrays, one entry per arm, in ascending order of `first`: ARM_KEYS."""
    arms = arm_list(g, keep, weight)
    return {f: np.array([a[f] for a in arms], dtype=np.int64) for f in ARM_KEYS}


def losers(g, keep=None, weight=None, max_dist=50000, max_diff=1000):
    """-> [(loser arm, winner arm)], the arms as arm_list gives them."""
    bubbles = {}
    for a in arm_list(g, keep, weight):
        bubbles.setdefault((a["source"], a["sink"]), []).append(a)
    out = []
    for arms in bubbles.values():
        if len(arms) < 2:
            continue
        win = max(arms, key=lambda a: (a["weight"], a["overlap"], -min(a["first"], a["last"] ^ 1)))
        for a in arms:
            if a is not win and win["dist"] <= max_dist and a["dist"] <= max_dist and abs(a["dist"] - win["dist"]) <= max_diff:
                out.append((a, win))
    return out


def bubble_nodes(g, keep=None, weight=None, max_dist=50000, max_diff=1000):
    """-> bool[N]: the nodes of every loser and their complements."""
    mark = np.zeros(int(g["num_nodes"]), dtype=bool)
    for a, _ in losers(g, keep, weight, max_dist, max_diff):
        for v in a["chain"]:
            mark[v] = mark[v ^ 1] = True
    return mark


def pop_rounds(g, keep=None, rounds=4, weight=None, max_dist=50000, max_diff=1000):
    """-> (bool[N] the nodes marked by all rounds, the number of rounds that marked a node, bool[E] the edges kept)."""
    if int(rounds) != rounds or rounds < 1:
        raise ValueError(f"rounds={rounds}: an int >= 1")
    src, dst = np.asarray(g["src"]).astype(np.int64), np.asarray(g["dst"]).astype(np.int64)
    keep = np.ones(len(src), dtype=bool) if keep is None else np.asarray(keep, dtype=bool).copy()
    total, done = np.zeros(int(g["num_nodes"]), dtype=bool), 0
    for _ in range(rounds):
        mark = bubble_nodes(g, keep, weight, max_dist, max_diff)
        if not mark.any():
            break
        total |= mark
        keep &= ~mark[src] & ~mark[dst]
        done += 1
    return total, done, keep


def kept_graph(g, keep, removed, compact=True):
    """The tail of graph_simplify_statement.simplify_graph: the edges of `keep`, the reads left without an edge dropped and the others
    renumbered (compact), the columns gathered; `removed` gains the count of dropped reads."""
    N = int(g["num_nodes"])
    src, dst = np.asarray(g["src"]).astype(np.int64), np.asarray(g["dst"]).astype(np.int64)
    origin = np.nonzero(keep)[0].astype(np.int64)
    src, dst = src[origin], dst[origin]
    touched = np.zeros(N, dtype=bool)
    touched[src] = True
    touched[dst] = True
    reads = np.nonzero(touched[0::2] | touched[1::2])[0].astype(np.int64) if compact else np.arange(N // 2, dtype=np.int64)
    out = {"kept_reads": reads, "edge_origin": origin, "num_nodes": 2 * len(reads), "removed": dict(removed, reads=N // 2 - len(reads))}
    new = np.full(N // 2, -1, dtype=np.int64)
    new[reads] = np.arange(len(reads))
    out["src"], out["dst"] = 2 * new[src >> 1] + (src & 1), 2 * new[dst >> 1] + (dst & 1)
    nodes = np.stack([2 * reads, 2 * reads + 1], 1).reshape(-1)
    for f in gs.EDGE_KEYS:
        if g.get(f) is not None:
            out[f] = np.asarray(g[f])[origin]
    for f in gs.NODE_KEYS:
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


def pop_bubbles(g, rounds=4, keep=None, weight=None, max_dist=50000, max_diff=1000, compact=True):
    """-> the dict of graph_simplify_statement.simplify_graph's shape, removed = {"bubble_nodes", "bubble_rounds", "reads"}."""
    total, done, keep = pop_rounds(g, keep, rounds, weight, max_dist, max_diff)
    return kept_graph(g, keep, {"bubble_nodes": int(total.sum()), "bubble_rounds": done}, compact)


def simplify_graph(g, fuzz=10, max_tip=4, tips=True, compact=True, bubbles=True):
    """graph_simplify_statement.simplify_graph with the bubbles popped after the tips, on what is kept, before the one compaction.
    bubbles: True or a dict of bubble_nodes' keywords and `rounds`."""
    N = int(g["num_nodes"])
    src, dst = np.asarray(g["src"]).astype(np.int64), np.asarray(g["dst"]).astype(np.int64)
    trans = gs.transitive_edges(g, fuzz)
    tip = gs.tip_nodes(g, ~trans, max_tip) if tips else np.zeros(N, dtype=bool)
    keep = ~trans & ~tip[src] & ~tip[dst]
    total, done, keep = pop_rounds(g, keep, **({} if bubbles is True else bubbles))
    removed = {"transitive_edges": int(trans.sum()), "tip_nodes": int(tip.sum()), "bubble_nodes": int(total.sum()), "bubble_rounds": done}
    return kept_graph(g, keep, removed, compact)
