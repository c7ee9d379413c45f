"""Unitigs on the MI355X: every maximal non-branching path of an overlap graph merged into one segment, the form of the GFAs hifiasm
(r_utg) and raven write and the reference trains and decodes on.

    c = unitig_chains(g)                                  # unitig, rank, offset per node; chain_off, chain_nodes; length, circular; link
    u = compact_unitigs(g)                                # the unitig graph as a new graph dict, with the unitig sequences as its reads
    write_gfa(u, "asm.utg.gfa")                           # S / A / L lines that gfa.read_gfa reads back

`g`: a graph dict of this package that follows the complement convention and whose edge multiset is closed under mates, with
prefix_length = read_length[src] - overlap_length on every edge - as overlapper.overlap_graph and simplify.simplify_graph give it;
anything else is a ValueError before a kernel is launched.  The rule is stated in include/gnnome_hip.h and, executable, in
tests/unitig_statement.py; the kernels are csrc/unitigs.hip: the link decision with the successor, predecessor and link-weight tables,
the list ranking (pointer jumping over 16-byte records, O(log n) launches for a chain of n nodes) and the scatter of the chain members.
torch does the plumbing: degrees, the mates check, the numbering of the chains (a scan over the heads), the gathers.  The sequences are
spelled by contigs.spell_contigs with the chains as walks.  Simple bubbles are popped by bubbles.py, on these chains."""
import ctypes

import torch

from . import _lib
from .ops import _on, _ptr, _stream
from .overlapper import _Stages
from .simplify import _graph, mates_closed

EDGE_KEYS = ("overlap_similarity", "y")


def _columns(g, device):
    """-> (src, dst, p, overlap, read_length int64 on the device, N, device); ValueError for what the rule does not take."""
    for f in ("overlap_length", "read_length"):
        if g.get(f) is None:
            raise ValueError(f"the graph dict carries no {f}")
    src, dst, p, N, dev = _graph(g, device)
    ol, rl = (torch.as_tensor(g[f]).to(dev, torch.int64).reshape(-1).contiguous() for f in ("overlap_length", "read_length"))
    if ol.numel() != src.numel() or rl.numel() != N:
        raise ValueError(f"overlap_length has {ol.numel()} entries for {src.numel()} edges, read_length {rl.numel()} for {N} nodes")
    return src, dst, p, ol, rl, N, dev


def _chains(src, dst, p, ol, rl, N, stages, grid=0):
    dev, E = src.device, int(src.numel())
    if not mates_closed(src, dst, N):
        raise ValueError("the edge set is not closed under mates: some edge (u, v) lacks (v ^ 1, u ^ 1)")
    if E and bool((p != rl[src] - ol).any()):
        raise ValueError("prefix_length is not read_length[src] - overlap_length on every edge")
    if N and int(rl.abs().max()) >= (1 << 31):
        raise ValueError("read lengths of 2^31 and more are not taken")
    out_deg = torch.bincount(src, minlength=N).to(torch.int32)
    in_deg = torch.bincount(dst, minlength=N).to(torch.int32)
    succ, pred, weight, succ_edge, head, rank = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(6))
    link, cyc = torch.zeros(E, dtype=torch.uint8, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)
    offset = torch.zeros(N, dtype=torch.int64, device=dev)
    stages.mark("unitig_lists")
    lib = _lib.load()
    rounds = (ctypes.c_int64 * 4)()
    if N:
        need = ctypes.c_size_t(0)
        _lib.check(lib.gnnome_unitig_rank_workspace_bytes(N, ctypes.byref(need)), "unitig_rank_workspace_bytes")
        ws = torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=dev)
        with _on(dev):
            _lib.check(lib.gnnome_unitig_links(_ptr(src), _ptr(dst), _ptr(p), _ptr(out_deg), _ptr(in_deg), N, E, _ptr(succ), _ptr(pred),
                                               _ptr(weight), _ptr(succ_edge), _ptr(link), _stream(dev)), "unitig_links")
            stages.mark("unitig_links")
            _lib.check(lib.gnnome_unitig_rank(_ptr(succ), _ptr(pred), _ptr(weight), _ptr(succ_edge), N, E, _ptr(link), _ptr(cyc), _ptr(head),
                                              _ptr(rank), _ptr(offset), int(grid), rounds, _ptr(ws), ws.numel(), _stream(dev)), "unitig_rank")
        del ws
    else:
        stages.mark("unitig_links")
    stages.mark("unitig_rank")
    # plumbing: the tail of every chain, the pairing of a chain with its complement, the numbering by ascending forward head
    node = torch.arange(N, device=dev)
    head = head.long()
    tail = torch.nonzero(succ < 0).squeeze(1)
    tail_of = torch.full((N,), -1, dtype=torch.int64, device=dev)
    tail_of[head[tail]] = tail                                         # one tail per head
    is_head = head == node
    forward = torch.nonzero(is_head & (node < (tail_of ^ 1))).squeeze(1)
    Q = int(forward.numel())
    U = 2 * Q
    if int(is_head.sum()) != U or (Q and not bool(is_head[tail_of[forward] ^ 1].all())):
        raise ValueError("a chain has no complement chain: the graph does not follow the complement convention")
    heads = torch.stack([forward, tail_of[forward] ^ 1], 1).reshape(-1)  # the head of unitig node j
    unitig_of_head = torch.full((N,), -1, dtype=torch.int64, device=dev)
    unitig_of_head[heads] = torch.arange(U, device=dev)
    unitig = unitig_of_head[head].to(torch.int32)
    tails = tail_of[heads]
    chain_off = torch.zeros(U + 1, dtype=torch.int64, device=dev)
    torch.cumsum(rank[tails].long() + 1, 0, out=chain_off[1:])
    length = offset[tails] + rl[tails]
    circular = cyc[heads].bool()
    chain_nodes = torch.empty(N, dtype=torch.int32, device=dev)
    stages.mark("unitig_number")
    if N:
        with _on(dev):
            _lib.check(lib.gnnome_unitig_scatter(_ptr(unitig), _ptr(rank), _ptr(chain_off), N, U, _ptr(chain_nodes), _stream(dev)),
                       "unitig_scatter")
    stages.mark("unitig_scatter")
    if stages.stats is not None:
        stages.stats.update(rank_rounds=int(rounds[0]), cycle_min_rounds=int(rounds[1]), cycle_rank_rounds=int(rounds[2]),
                            cycle_nodes=int(rounds[3]))
    return {"unitig": unitig, "rank": rank, "offset": offset, "chain_off": chain_off, "chain_nodes": chain_nodes, "length": length,
            "circular": circular, "link": link.bool()}


def unitig_chains(g, device=None, stats=None, grid=0):
    """-> dict of device tensors: unitig int32[N] (the unitig node of each graph node), rank int32[N] (its 0-based place in the chain),
    offset int64[N] (the summed prefix_length of the links before it), chain_off int64[U + 1] / chain_nodes int32[N] (the nodes of
    unitig node j in order), length int64[U] (offset[tail] + read_length[tail]), circular bool[U], link bool[E] (the edge is internal to
    a chain; the cut link of a cycle is not).  U is even: 2q is the forward chain of pair q, 2q + 1 its complement.  ValueError where
    the edges are not closed under mates or prefix_length is not read_length[src] - overlap_length.  stats: a dict that receives the
    device-event times unitig_lists_ms (torch: checks, degrees), unitig_links_ms (the link kernel), unitig_rank_ms (the ranking: its
    launches and the count read-backs), unitig_number_ms (torch), unitig_scatter_ms (the scatter kernel), and rank_rounds,
    cycle_min_rounds, cycle_rank_rounds, cycle_nodes (a graph without cycles has 0 for the last three).  grid: workgroups per ranking
    launch (0: by size); no result depends on it, the tests vary it."""
    src, dst, p, ol, rl, N, dev = _columns(g, device)
    stages = _Stages(stats, dev)
    out = _chains(src, dst, p, ol, rl, N, stages, grid)
    stages.finish()
    return out


def _member_names(g, N):
    """The name of the read of every even node: g["node_to_read"] where it names one, else read{r}."""
    table = g.get("node_to_read") if isinstance(g.get("node_to_read"), dict) else {}
    return [table[v] if isinstance(table.get(v), str) else f"read{v >> 1}" for v in range(0, N, 2)]


def unitig_name(q, circular):
    return "utg%06d%s" % (q + 1, "c" if circular else "l")


def compact_unitigs(g, device=None, stats=None):
    """-> a new graph dict, the unitig graph: every edge of g that is not internal to a chain becomes (unitig[u], unitig[v]), in the old
    relative order (edge_origin int64[E'] indexes back; the cut link of a cycle becomes a self-edge); overlap_length, overlap_similarity
    and y are gathered, prefix_length = length[src] - overlap_length, read_length = length, num_nodes = U.  Also chain_off, chain_nodes,
    circular (unitig_chains'), chain_pos and chain_read_length int64[N] (the offset in its unitig and the length of every member, in
    chain_nodes' order: the A lines of write_gfa), unitig_of (its `unitig`); where g carries packed `reads`, reads = the sequences of the even unitig nodes,
    spelled on the device by contigs.spell_contigs along the chains; and the name tables in gfa.read_gfa's unitig form: node_to_read[2q]
    = node_to_read[2q + 1] = [(read name, "+" / "-"), ...] (the names of g["node_to_read"] where present, else read{r}), read_to_node
    {unitig name: (2q, 2q + 1)}, read_to_node2 {read name: (2q, 2q + 1)}.  The read_* position columns and `contained` are not carried:
    labels on a unitig graph come through write_gfa and gfa.read_gfa(training=True).  stats: unitig_chains' and unitig_edges_ms,
    unitig_spell_ms, unitig_names_ms."""
    src, dst, p, ol, rl, N, dev = _columns(g, device)
    E = int(src.numel())
    stages = _Stages(stats, dev)
    c = _chains(src, dst, p, ol, rl, N, stages)
    U = int(c["length"].numel())
    origin = torch.nonzero(~c["link"]).squeeze(1)
    unitig = c["unitig"].long()
    new_src, new_dst, new_ol = unitig[src[origin]], unitig[dst[origin]], ol[origin]
    out = {"src": new_src, "dst": new_dst, "num_nodes": U, "overlap_length": new_ol, "prefix_length": c["length"][new_src] - new_ol,
           "read_length": c["length"], "overlap_similarity": None, "edge_origin": origin, "chain_off": c["chain_off"],
           "chain_nodes": c["chain_nodes"], "chain_pos": c["offset"][c["chain_nodes"].long()], "chain_read_length": rl[c["chain_nodes"].long()],
           "circular": c["circular"], "unitig_of": c["unitig"], "read_seqs": None}
    for f in EDGE_KEYS:
        if g.get(f) is not None:
            t = torch.as_tensor(g[f])
            if t.dim() == 0 or t.shape[0] != E:
                raise ValueError(f"{f}: expected {E} entries, got shape {tuple(t.shape)}")
            out[f] = t[origin.to(t.device)]
    stages.mark("unitig_edges")
    if g.get("reads") is not None:
        from .contigs import ReadStore, spell_contigs
        from .decode import DecodeGraph
        data, off = (t.to(dev).contiguous() for t in g["reads"])
        if int(off.numel()) != N // 2 + 1:
            raise ValueError(f"reads: {int(off.numel()) - 1} packed reads for {N // 2} reads of the graph")
        if U:
            # the chains of the even unitig nodes as (int32 nodes, int64 offsets) walks
            counts = (c["chain_off"][1:] - c["chain_off"][:-1])[0::2]
            walk_off = torch.zeros(U // 2 + 1, dtype=torch.int64, device=dev)
            torch.cumsum(counts, 0, out=walk_off[1:])
            walk_nodes = c["chain_nodes"][(c["unitig"][c["chain_nodes"].long()] & 1) == 0].contiguous()
            spelled = spell_contigs(DecodeGraph(src, dst, N, p, rl, device=dev), (walk_nodes, walk_off), ReadStore.from_packed(data, off.long()))
            if not torch.equal(spelled.lengths, c["length"][0::2]):
                raise ValueError("a unitig's sequence is not as long as its chain says: an overlap is longer than its read")
            out["reads"] = (spelled.data, spelled.offsets)
        else:
            out["reads"] = (torch.zeros(0, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    stages.mark("unitig_spell")
    names = _member_names(g, N)
    nodes, offs, circ = c["chain_nodes"].tolist(), c["chain_off"].tolist(), c["circular"].tolist()
    node_to_read, read_to_node, read_to_node2 = {}, {}, {}
    for q in range(U // 2):
        members = [(names[v >> 1], "+-"[v & 1]) for v in nodes[offs[2 * q]:offs[2 * q + 1]]]
        node_to_read[2 * q] = node_to_read[2 * q + 1] = members
        read_to_node[unitig_name(q, circ[2 * q])] = (2 * q, 2 * q + 1)
        for name, _ in members:
            read_to_node2[name] = (2 * q, 2 * q + 1)
    out.update(node_to_read=node_to_read, read_to_node=read_to_node, read_to_node2=read_to_node2)
    stages.mark("unitig_names")
    stages.finish()
    return out


def _mate_index(src, dst, N):
    """The index of every edge's mate; ValueError for parallel edges or a missing mate."""
    key = src * N + dst
    ks, order = torch.sort(key)
    if int(key.numel()) > 1 and bool((ks[1:] == ks[:-1]).any()):
        raise ValueError("parallel edges: gfa.read_gfa keeps one edge per (src, dst) pair, so the file would not read back as this graph")
    want = (dst ^ 1) * N + (src ^ 1)
    at = torch.searchsorted(ks, want).clamp(max=max(int(key.numel()) - 1, 0))
    if int(key.numel()) and not bool((ks[at] == want).all()):
        raise ValueError("the edge set is not closed under mates: some edge (u, v) lacks (v ^ 1, u ^ 1)")
    return order[at]


def write_gfa(g, path):
    """Write the graph dict `g` (packed `reads` required) as a GFA that gfa.read_gfa reads back as the same graph:
    `S <name> <seq> LN:i:<len>` per read, named by g["node_to_read"] where that names single reads, else read{r}; for a dict with chains
    (compact_unitigs') the names utg%06dl / utg%06dc (circular) and one `A <utg> <offset> <+/-> <read> 0 <read_length>` line per member;
    one `L <a> <+/-> <b> <+/-> <overlap>M` line per mate pair, taken from the edge whose index is not larger than its mate's (an edge that is
    its own mate gives one line), with the SI:f: tag as gfa.write_similarity_tags writes it where g carries overlap_similarity.  Tensors
    come to the host once; the lines are formatted there.  ValueError for parallel edges (read_gfa collapses them) and for a dict without
    packed reads."""
    if g.get("reads") is None:
        raise ValueError("write_gfa: the graph dict carries no packed reads (the S lines need the sequences)")
    N = int(g["num_nodes"])
    src, dst, ol = (torch.as_tensor(g[f]).reshape(-1).long() for f in ("src", "dst", "overlap_length"))
    mate = _mate_index(src, dst.to(src.device), N).cpu()
    src, dst, ol = src.tolist(), dst.tolist(), ol.tolist()
    sim = g.get("overlap_similarity")
    sim = None if sim is None else torch.as_tensor(sim).reshape(-1).float().tolist()
    data, off = g["reads"]
    buf, off = data.cpu().numpy().tobytes(), off.tolist()
    if len(off) != N // 2 + 1:
        raise ValueError(f"write_gfa: {len(off) - 1} packed reads for {N // 2} reads of the graph")
    length = torch.as_tensor(g["read_length"]).reshape(-1).tolist()
    chains = g.get("chain_nodes") is not None
    if chains:
        coff, circ = g["chain_off"].tolist(), g["circular"].tolist()
        cpos, clen = g["chain_pos"].tolist(), g["chain_read_length"].tolist()
        names = [unitig_name(q, circ[2 * q]) for q in range(N // 2)]
    else:
        names = _member_names(g, N)
    with open(path, "w", newline="\n") as f:
        for r, name in enumerate(names):
            f.write(f"S\t{name}\t{buf[off[r]:off[r + 1]].decode('latin-1')}\tLN:i:{length[2 * r]}\n")
            if chains:
                a, b = coff[2 * r], coff[2 * r + 1]
                for (read, strand), at, n in zip(g["node_to_read"][2 * r], cpos[a:b], clen[a:b]):
                    f.write(f"A\t{name}\t{at}\t{strand}\t{read}\t0\t{n}\n")
        for e, m in enumerate(mate.tolist()):
            if e <= m:
                tag = "" if sim is None else f"\tSI:f:{sim[e]:.9g}"
                f.write(f"L\t{names[src[e] >> 1]}\t{'+-'[src[e] & 1]}\t{names[dst[e] >> 1]}\t{'+-'[dst[e] & 1]}\t{ol[e]}M{tag}\n")
    return path
