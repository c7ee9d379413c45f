"""Unitig compaction, restated in NumPy / plain Python (no GPU, no torch): what gnnome_amd.unitigs and csrc/unitigs.hip must reproduce bit
for bit.  Integers only.  The graph is a dict that follows the complement convention - node v ^ 1 is the reverse complement of v, edge
(u, v) has the mate (v ^ 1, u ^ 1) - whose edge multiset is closed under mates and whose prefixes are p(e) = read_length[src] -
overlap_length (both checked: ValueError).

Link.  Degrees count parallel edges.  Edge (u, v) is a link iff out_deg(u) == 1, in_deg(v) == 1 and u >> 1 != v >> 1 (no self-loop, no
hairpin u -> u ^ 1).  Chains are the maximal paths over links; a node without links is a chain of one.  A component all of whose edges are
links has no head: with r its smallest read, the cycle that holds node 2r starts at 2r and the cycle that holds 2r + 1 ends at 2r + 1; the
link that enters the start is the cut link and is not internal.

Numbering.  Of a chain and its complement (reversed, every node ^ 1) the forward one has the smaller head; the pairs are numbered q = 0,
1, .. by ascending forward head; unitig node 2q is the forward chain, 2q + 1 its complement.

Unitig graph (`compact_unitigs`).  Every edge that is not internal becomes (unitig[u], unitig[v]) in the old relative order - a cut link
thereby the self-edge (U, U); overlap_length, overlap_similarity and y are gathered, prefix_length = length[src] - overlap_length,
read_length = length.  The sequence of an even unitig node is the walk along its chain: reads[c][:p] for every node but the last, the
whole last read."""
import numpy as np

from graph_simplify_statement import mate_closed

_COMP = bytes.maketrans(b"ACGTMRWSYKVHDBXNUacgtmrwsykvhdbxnu", b"TGCAKYWSRMBDHVXNAtgcakywsrmbdhvxna")


def columns(g):
    """-> (N, src, dst, p, overlap, read_length) as lists; ValueError for what the rule does not take."""
    N = int(g["num_nodes"])
    src, dst, p, ol = (np.asarray(g[f]).tolist() for f in ("src", "dst", "prefix_length", "overlap_length"))
    rl = np.asarray(g["read_length"]).tolist()
    if N % 2 or len(rl) != N or not (len(src) == len(dst) == len(p) == len(ol)):
        raise ValueError("num_nodes is even, read_length per node, the other columns per edge")
    if any(not 0 <= x < N for x in src + dst):
        raise ValueError("a node id outside [0, num_nodes)")
    if not mate_closed(src, dst):
        raise ValueError("the edge set is not closed under mates")
    if any(p[e] != rl[src[e]] - ol[e] for e in range(len(src))):
        raise ValueError("prefix_length is not read_length[src] - overlap_length")
    return N, src, dst, p, ol, rl


def unitig_chains(g):
    """-> dict: unitig int32[N], rank int32[N], offset int64[N], chain_off int64[U + 1], chain_nodes int32[N], length int64[U],
    circular bool[U], link bool[E]."""
    N, src, dst, p, ol, rl = columns(g)
    out_deg, in_deg = [0] * N, [0] * N
    for u, v in zip(src, dst):
        out_deg[u] += 1
        in_deg[v] += 1
    link = [out_deg[u] == 1 and in_deg[v] == 1 and u >> 1 != v >> 1 for u, v in zip(src, dst)]
    succ, pred, weight, edge_of = {}, {}, {}, {}
    for e, (u, v) in enumerate(zip(src, dst)):
        if link[e]:
            succ[u], pred[v], weight[u], edge_of[u] = v, u, p[e], e
    # what no head reaches lies on a cycle: cut it at its smallest read
    seen = set()
    for h in range(N):
        if h not in pred:
            while h is not None:
                seen.add(h)
                h = succ.get(h)
    on_cycle = set()
    for v in range(N):
        if v in seen:
            continue
        cyc, x = [v], succ[v]
        while x != v:
            cyc.append(x)
            x = succ[x]
        r = min(c >> 1 for c in cyc)
        a, b = (pred[2 * r], 2 * r) if 2 * r in cyc else (2 * r + 1, succ[2 * r + 1])     # the cut link a -> b
        link[edge_of[a]] = False
        del succ[a], pred[b]
        seen.update(cyc)
        on_cycle.update(cyc)
    chains = {}
    for h in range(N):
        if h not in pred:
            chain, x = [], h
            while x is not None:
                chain.append(x)
                x = succ.get(x)
            chains[h] = chain
    forward = [h for h in sorted(chains) if h < chains[h][-1] ^ 1]
    ordered = []
    for h in forward:
        ordered += [chains[h], chains[chains[h][-1] ^ 1]]
    U = len(ordered)
    unitig, rank, offset = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int64)
    chain_off, length, circular = np.zeros(U + 1, dtype=np.int64), np.zeros(U, dtype=np.int64), np.zeros(U, dtype=bool)
    chain_nodes = []
    for j, chain in enumerate(ordered):
        bases = 0
        for i, c in enumerate(chain):
            unitig[c], rank[c], offset[c] = j, i, bases
            bases += weight[c] if i + 1 < len(chain) else rl[c]
        chain_nodes += chain
        chain_off[j + 1], length[j], circular[j] = len(chain_nodes), bases, chain[0] in on_cycle
    return {"unitig": unitig, "rank": rank, "offset": offset, "chain_off": chain_off, "chain_nodes": np.array(chain_nodes, dtype=np.int32),
            "length": length, "circular": circular, "link": np.array(link, dtype=bool)}


def node_sequence(g, v):
    data, off = (np.asarray(t) for t in g["reads"])
    s = data[off[v >> 1]:off[(v >> 1) + 1]].tobytes()
    return s if v % 2 == 0 else s.translate(_COMP)[::-1]


def spell(g, chain):
    """The bytes of the walk `chain` (a list of nodes linked by edges of g)."""
    src, dst, p = (np.asarray(g[f]).tolist() for f in ("src", "dst", "prefix_length"))
    prefix = {(u, v): x for u, v, x in zip(src, dst, p)}
    return b"".join(node_sequence(g, c)[:prefix[(c, n)]] for c, n in zip(chain, chain[1:])) + node_sequence(g, chain[-1])


def compact_unitigs(g):
    """-> dict of numpy arrays: src, dst, num_nodes, overlap_length, prefix_length, read_length, edge_origin, chain_off, chain_nodes,
    chain_pos and chain_read_length (the offset and the read length of every member, in chain_nodes' order), circular, unitig_of, whichever of overlap_similarity and y the input carries, and reads (data, off) where it carries reads."""
    c = unitig_chains(g)
    origin = np.nonzero(~c["link"])[0].astype(np.int64)
    src = c["unitig"][np.asarray(g["src"])[origin]].astype(np.int64)
    dst = c["unitig"][np.asarray(g["dst"])[origin]].astype(np.int64)
    ol = np.asarray(g["overlap_length"])[origin].astype(np.int64)
    out = {"src": src, "dst": dst, "num_nodes": len(c["length"]), "overlap_length": ol, "prefix_length": c["length"][src] - ol,
           "read_length": c["length"], "edge_origin": origin, "chain_off": c["chain_off"], "chain_nodes": c["chain_nodes"],
           "chain_pos": c["offset"][c["chain_nodes"]], "chain_read_length": np.asarray(g["read_length"]).astype(np.int64)[c["chain_nodes"]],
           "circular": c["circular"], "unitig_of": c["unitig"]}
    for f in ("overlap_similarity", "y"):
        if g.get(f) is not None:
            out[f] = np.asarray(g[f])[origin]
    if g.get("reads") is not None:
        off, nodes = c["chain_off"].tolist(), c["chain_nodes"].tolist()
        seqs = [spell(g, nodes[off[j]:off[j + 1]]) for j in range(0, len(c["length"]), 2)]
        new_off = np.zeros(len(seqs) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in seqs], out=new_off[1:])
        out["reads"] = (np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), new_off)
    return out
