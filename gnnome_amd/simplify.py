"""Simplify an overlap graph on the MI355X: what hifiasm's r_utg and raven's graph have had done to them before the reference trains and
decodes on them.

    mark = transitive_edges(g, fuzz=10)                  # bool[E]: the edges a two-hop path explains
    tip = tip_nodes(g, keep=~mark, max_tip=4)            # bool[N]: short dead ends at a junction, and their complements
    s = simplify_graph(g)                                # both, the edges dropped, the reads left without an edge removed and renumbered
    s = simplify_graph(g, bubbles=True)                  # and the simple bubbles of what is kept popped (bubbles.py), off by default

`g`: any graph dict of this package that follows the complement convention - node v ^ 1 is the reverse complement of v, edge (u, v) has
the mate (v ^ 1, u ^ 1) - as overlapper.overlap_graph, gfa.read_gfa / read_gfa_device, synth and decode do; src, dst, num_nodes,
prefix_length are read (simplify_graph gathers the other columns).  The rules are stated in include/gnnome_hip.h and, executable, in
tests/graph_simplify_statement.py; the kernels are csrc/graph_simplify.hip.  torch does the plumbing: the sort of the edges by
(src, dst) and the row pointer for the mark kernel; degrees, the unique successor and the in-edge lists of the kept edges for the tip
kernels; the gathers and the renumbering.  Unitig compaction and the GFA writer are unitigs.py; simple bubbles are bubbles.py, which
simplify_graph(bubbles=) runs after the tips."""
import ctypes

import torch

from . import _lib
from .ops import _on, _ptr, _stream
from .overlapper import _Stages

EDGE_KEYS = ("overlap_length", "prefix_length", "overlap_similarity", "y")
_LIMIT = 1 << 31


def transitive_tile_size():
    """Out-edges of one node the mark kernel holds in LDS at a time; results do not depend on it, the tests place their hub by it."""
    tile = ctypes.c_int(0)
    _lib.check(_lib.load().gnnome_transitive_tile_size(ctypes.byref(tile)), "transitive_tile_size")
    return int(tile.value)


def _graph(g, device):
    """-> (src, dst, prefix int64 on the device, N); refuses what the kernels do not take."""
    for f in ("src", "dst", "num_nodes", "prefix_length"):
        if g.get(f) is None:
            raise ValueError(f"the graph dict carries no {f}")
    N = int(g["num_nodes"])
    src = torch.as_tensor(g["src"])
    if device is None:
        device = src.device if src.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    src, dst, p = (torch.as_tensor(g[f]).to(device, torch.int64).reshape(-1).contiguous() for f in ("src", "dst", "prefix_length"))
    E = int(src.numel())
    if dst.numel() != E or p.numel() != E:
        raise ValueError(f"src, dst and prefix_length have {E}, {dst.numel()} and {p.numel()} entries")
    if N < 0 or N % 2 or N >= _LIMIT or E >= _LIMIT:
        raise ValueError(f"num_nodes={N} (even, below 2^31) and {E} edges (below 2^31) expected")
    if E:
        lo, hi, pmax = torch.stack([torch.minimum(src.min(), dst.min()), torch.maximum(src.max(), dst.max()), p.abs().max()]).tolist()
        if lo < 0 or hi >= N:
            raise ValueError(f"node ids {lo} .. {hi} outside [0, {N})")
        if pmax >= (1 << 30):
            raise ValueError("prefix lengths of 2^30 and more are not taken")
    return src, dst, p, N, device


def _transitive(src, dst, p, N, fuzz, stages):
    E, dev = int(src.numel()), src.device
    if int(fuzz) != fuzz or fuzz < 0 or fuzz >= (1 << 30):
        raise ValueError(f"fuzz={fuzz}: an absolute number of bases, an int >= 0")
    mark = torch.zeros(E, dtype=torch.uint8, device=dev)
    if E:
        # plumbing: the edges by (src, dst) and where every row starts
        order = torch.sort(src * N + dst, stable=True).indices
        row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(src, minlength=N), 0, out=row_ptr[1:])
        s_dst, s_p, s_eid = dst[order].to(torch.int32), p[order].to(torch.int32), order.to(torch.int32)
        stages.mark("transitive_sort")
        with _on(dev):
            _lib.check(_lib.load().gnnome_transitive_edges(_ptr(row_ptr), _ptr(s_dst), _ptr(s_p), _ptr(s_eid), N, E, int(fuzz), _ptr(mark),
                                                           _stream(dev)), "transitive_edges")
        stages.mark("transitive_mark")
    return mark.bool()


def _tips(src, dst, p, N, keep, max_tip, stages):
    dev = src.device
    if int(max_tip) != max_tip or max_tip < 1:
        raise ValueError(f"max_tip={max_tip}: an int >= 1")
    if keep is not None:
        keep = torch.as_tensor(keep).to(dev).reshape(-1)
        if keep.dtype != torch.bool or keep.numel() != src.numel():
            raise ValueError(f"keep: expected bool[{src.numel()}]")
        src, dst, p = src[keep], dst[keep], p[keep]
    tip = torch.zeros(N, dtype=torch.uint8, device=dev)
    if int(src.numel()) and N:
        # plumbing: degrees, the successor of the nodes that have one, the in-edge lists
        out_deg, in_deg = torch.bincount(src, minlength=N), torch.bincount(dst, minlength=N)
        only = out_deg[src] == 1
        succ, succ_p = torch.full((N,), -1, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
        succ[src[only]] = dst[only].to(torch.int32)          # one writer per slot
        succ_p[src[only]] = p[only].to(torch.int32)
        in_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        torch.cumsum(in_deg, 0, out=in_ptr[1:])
        in_src = src[torch.sort(dst, stable=True).indices].to(torch.int32)
        out_deg, in_deg = out_deg.to(torch.int32), in_deg.to(torch.int32)
        lib = _lib.load()
        need = ctypes.c_size_t(0)
        _lib.check(lib.gnnome_tip_nodes_workspace_bytes(N, ctypes.byref(need)), "tip_nodes_workspace_bytes")
        ws = torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=dev)
        stages.mark("tip_lists")
        with _on(dev):
            _lib.check(lib.gnnome_tip_nodes(_ptr(in_deg), _ptr(out_deg), _ptr(succ), _ptr(succ_p), _ptr(in_ptr), _ptr(in_src), N, int(max_tip),
                                            _ptr(tip), _ptr(ws), ws.numel(), _stream(dev)), "tip_nodes")
        stages.mark("tip_mark")
    return tip.bool()


def transitive_edges(g, fuzz=10, device=None, stats=None):
    """-> bool[E] on the device: edge e = (v, x) is transitive iff a node w, w != v and w != x, has edges e1 = (v, w) and e2 = (w, x)
    with |p(e1) + p(e2) - p(e)| <= fuzz.  All edges are judged on the input graph at once.  fuzz: an absolute number of bases (no
    relative part: p of an edge and of its mate differ, the residual does not, so an edge is transitive iff its mate is).  stats: a
    dict that receives transitive_sort_ms (torch) and transitive_mark_ms (the kernel)."""
    src, dst, p, N, dev = _graph(g, device)
    stages = _Stages(stats, dev)
    mark = _transitive(src, dst, p, N, fuzz, stages)
    stages.finish()
    return mark


def tip_nodes(g, keep=None, max_tip=4, device=None, stats=None):
    """-> bool[N] on the device, on the graph restricted to the edges of `keep` (bool[E]; None: all).  A chain of at most max_tip nodes
    that starts at a node of in-degree 0, follows unique out-edges through nodes of in-degree <= 1 and ends at a junction (in-degree
    >= 2) is a tip, unless every in-edge of the junction comes from such a chain and this one has the largest summed p (ties: the
    smallest last node).  A tip's nodes and their complements are marked.  stats: tip_lists_ms (torch), tip_mark_ms (two launches)."""
    src, dst, p, N, dev = _graph(g, device)
    stages = _Stages(stats, dev)
    tip = _tips(src, dst, p, N, keep, max_tip, stages)
    stages.finish()
    return tip


def mates_closed(src, dst, num_nodes):
    """The edge multiset equals the multiset of its mates (v ^ 1, u ^ 1)."""
    return bool(torch.equal(torch.sort(src * num_nodes + dst).values, torch.sort((dst ^ 1) * num_nodes + (src ^ 1)).values))


def _renumber_table(table, new_node):
    """A host name table of a graph dict under the renumbering new_node (list: old node -> new node or -1)."""
    if not isinstance(table, dict):
        return table
    out = {}
    for k, v in table.items():
        if isinstance(v, tuple) and len(v) == 2 and all(isinstance(x, int) for x in v):    # name -> (node, complement)
            if new_node[v[0]] >= 0:
                out[k] = (new_node[v[0]], new_node[v[1]])
        elif isinstance(k, int):                                                              # node -> name(s) / sequence
            if new_node[k] >= 0:
                out[new_node[k]] = v
        else:
            out[k] = v
    return out


def _kept_graph(g, src, dst, N, keep, removed, compact, check_mates, dev):
    """The tail simplify_graph and bubbles.pop_bubbles share: the edges of `keep` (bool[E]) in their old order, with compact the reads
    left without an edge removed and the others renumbered, every column of `g` gathered -> the new dict; `removed` gains "reads"."""
    E, R = int(src.numel()), N // 2
    origin = torch.nonzero(keep).squeeze(1)
    src, dst = src[origin], dst[origin]
    if check_mates and not mates_closed(src, dst, N):
        raise ValueError("the kept edges are not closed under mates: the prefix lengths of the mates do not agree (p = len(src) - overlap)")
    if compact:
        touched = torch.zeros(N, dtype=torch.bool, device=dev)
        touched[src] = True
        touched[dst] = True
        reads = torch.nonzero(touched[0::2] | touched[1::2]).squeeze(1)
    else:
        reads = torch.arange(R, device=dev)
    new_read = torch.full((R,), -1, dtype=torch.int64, device=dev)
    new_read[reads] = torch.arange(int(reads.numel()), device=dev)
    nodes = torch.stack([2 * reads, 2 * reads + 1], 1).reshape(-1)
    out = dict(g)
    out.update(src=2 * new_read[src >> 1] + (src & 1), dst=2 * new_read[dst >> 1] + (dst & 1), num_nodes=2 * int(reads.numel()),
               kept_reads=reads, edge_origin=origin, removed=dict(removed, reads=R - int(reads.numel())))

    def gather(value, index, count):
        t = torch.as_tensor(value)
        if t.dim() == 0 or t.shape[0] != count:
            raise ValueError(f"expected {count} entries, got shape {tuple(t.shape)}")
        return t[index.to(t.device)]

    for f in EDGE_KEYS:
        if g.get(f) is not None:
            out[f] = gather(g[f], origin, E)
    for f, value in g.items():
        if f.startswith("read_") and value is not None and (torch.is_tensor(value) or hasattr(value, "__array__")):
            out[f] = gather(value, nodes, N)
    if g.get("contained") is not None:
        out["contained"] = gather(g["contained"], reads, R)
    if compact:
        if g.get("reads") is not None:
            from .textscan import pack
            data, off = (t.to(dev).contiguous() for t in g["reads"])
            if int(off.numel()) != R + 1:
                raise ValueError(f"reads: {int(off.numel()) - 1} packed reads for {R} reads of the graph")
            out["reads"] = pack(_lib.load(), data, off[:-1][reads], (off[1:] - off[:-1])[reads], dev)
        new_node = torch.stack([2 * new_read, 2 * new_read + 1], 1).reshape(-1)
        new_node = torch.where(new_node < 0, torch.full_like(new_node, -1), new_node).tolist()
        for f in ("node_to_read", "read_to_node", "read_to_node2", "read_seqs"):
            if isinstance(g.get(f), dict):
                out[f] = _renumber_table(g[f], new_node)
    return out


def simplify_graph(g, fuzz=10, max_tip=4, tips=True, compact=True, check_mates=True, device=None, stats=None, bubbles=None):
    """-> a new graph dict: the transitive edges (transitive_edges(g, fuzz)) and, with tips=True, the tip nodes of what is kept
    (tip_nodes(g, ~mark, max_tip)) are found, and every marked edge and every edge at a tip node is dropped; the edges keep their
    relative order.  compact=True also removes the reads both of whose nodes are left without an edge (contained reads, clipped tips,
    reads that never overlapped) and renumbers the others 2r', 2r' + 1 in the old order; compact=False keeps num_nodes.  Gathered
    where present: src, dst, overlap_length, prefix_length, overlap_similarity, y per edge; read_length and every other tensor-valued
    read_* column per node; contained per read; reads = the packed (data, off); the name tables (node_to_read, read_to_node,
    read_to_node2, read_seqs).  Any other key is carried over as it is.  New keys: kept_reads int64[R'] (the old read of each new
    one), edge_origin int64[E'] (the old edge of each new one), removed = {"transitive_edges", "tip_nodes", "reads"} (counts).
    check_mates: ValueError when the input's edges, or the kept ones, are not closed under mates.  bubbles: True, or a dict of
    bubbles.bubble_nodes' keywords (weight, max_dist, max_diff, grid) and `rounds` - after the tips the simple bubbles of what is kept
    are popped (bubbles.pop_bubbles' rounds; the dict then needs overlap_length and read_length), before the one compaction, and
    `removed` gains "bubble_nodes" and "bubble_rounds"; None, the default, changes nothing.  stats: a dict that receives the
    device-event times mates_ms, transitive_sort_ms, transitive_mark_ms, tip_lists_ms, tip_mark_ms, compact_ms, and with bubbles
    pop_bubbles' entries."""
    if bubbles is not None and bubbles is not True and not isinstance(bubbles, dict):
        raise ValueError(f"bubbles={bubbles!r}: expected None, True or a dict of bubble_nodes' keywords and rounds")
    src, dst, p, N, dev = _graph(g, device)
    if bubbles is None:
        stages = _Stages(stats, dev)
    else:
        from . import bubbles as bubbles_mod
        from .unitigs import _columns
        kw = {"rounds": 4, "weight": None, "max_dist": 50000, "max_diff": 1000, "grid": 0}
        given = bubbles if isinstance(bubbles, dict) else {}
        if set(given) - set(kw):
            raise ValueError(f"bubbles: unknown keywords {sorted(set(given) - set(kw))}; expected some of {sorted(kw)}")
        kw.update(given)
        ol, rl = _columns(g, dev)[3:5]
        stages = bubbles_mod._SummedStages(stats, dev)
    if check_mates:
        if not mates_closed(src, dst, N):
            raise ValueError("the edge set is not closed under mates: some edge (u, v) lacks (v ^ 1, u ^ 1)")
        stages.mark("mates")
    mark = _transitive(src, dst, p, N, fuzz, stages)
    if tips:
        tip = _tips(src, dst, p, N, ~mark, max_tip, stages)
    else:
        if int(max_tip) != max_tip or max_tip < 1:
            raise ValueError(f"max_tip={max_tip}: an int >= 1")
        tip = torch.zeros(N, dtype=torch.bool, device=dev)
    keep = ~mark & ~tip[src] & ~tip[dst]
    removed = {"transitive_edges": int(mark.sum()), "tip_nodes": int(tip.sum())}
    if bubbles is not None:
        popped, rounds, keep = bubbles_mod._pop(src, dst, p, ol, rl, N, keep, kw["rounds"], kw["weight"], kw["max_dist"], kw["max_diff"],
                                                stages, kw["grid"])
        removed.update(bubble_nodes=int(popped.sum()), bubble_rounds=rounds)
    out = _kept_graph(g, src, dst, N, keep, removed, compact, check_mates, dev)
    stages.mark("compact")
    stages.finish()
    return out
