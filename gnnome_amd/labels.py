"""Ground-truth edge labels for training, on the MI355X (utils/labels.py; graph_parser.py:387-400 with training=True).

    g = gfa.read_gfa("asm.gfa", reads_path="reads.fasta", training=True)     # g["y"]: these labels, computed here
    gt_edge_ids, y = process_graph(g)                                        # y float32[E] in edge-id order
    merged = interval_union(g)                                               # the strand +1 reads' [start, end] union (host)
    islands = interval_union_device(g, by="chr")                             # the same on the device, per chromosome
    report = reference_coverage(g, ref_length={1: 4_600_000})                # covered bases, islands, longest island, fraction

An edge (u, v) is correct - a "class edge" - when both reads come from one chromosome and one genome strand and v starts inside u
(strand +1: start[u] < start[v] < end[u]; strand -1 mirrored).  Per (chromosome, strand) the reference walks the class graph
component by component from the leftmost alive read, keeps the component of the farthest-reaching read if it extends what was
reached before, and labels that component's class edges 1; every other edge is 0.  gnnome_edge_labels (csrc/edge_labels.hip)
does the same loop with one wavefront per (chromosome, strand) and label sets that do not depend on traversal order.

Two differences from the reference, both deliberate:
  * ties: every argmin / argmax takes the smallest node id among equal keys.  The reference takes the first node in a networkx
    node view's order on the first pass and in a Python set's hash order afterwards; that order is an accident of the container
    and is not emulated.  Where no tie decides, the labels are the reference's.
  * a (chromosome, strand) with no class edges contributes nothing; the reference raises ValueError (max() of an empty set), and
    its several-chromosome path (process_graph_combo) raises AttributeError on the plain-int chromosome codes its own parser
    stores.  Here any number of chromosomes works.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .ops import _on, _ptr, _stream

STATS_FIELDS = ("chr", "strand", "nodes", "class_edges", "passes", "accepted", "forward_pops", "backward_pops")
_I32 = (-(1 << 31), (1 << 31) - 1)


def _host_checks(src, dst, num_nodes, read_strand, read_start, read_end, read_chr):
    n, E = int(num_nodes), int(src.numel())
    if n < 0 or n >= (1 << 31) or E >= (1 << 31):
        raise ValueError(f"edge_labels: N={n} E={E}: both must be below 2^31")
    if dst.numel() != E:
        raise ValueError(f"edge_labels: src has {E} entries, dst {dst.numel()}")
    for name, t in (("read_strand", read_strand), ("read_start", read_start), ("read_end", read_end), ("read_chr", read_chr)):
        if t.numel() != n:
            raise ValueError(f"edge_labels: {name} has {t.numel()} entries for {n} nodes")
    if E and (int(src.min()) < 0 or int(dst.min()) < 0 or int(src.max()) >= n or int(dst.max()) >= n):
        raise ValueError(f"edge_labels: an edge has a node outside [0, {n})")
    if n and not bool(((read_strand == 1) | (read_strand == -1)).all()):
        raise ValueError("edge_labels: read_strand must be -1 or +1 for every node")
    if n and (int(read_chr.min()) < _I32[0] or int(read_chr.max()) > _I32[1]):
        raise ValueError("edge_labels: read_chr does not fit int32")


def edge_labels(src, dst, num_nodes, read_strand, read_start, read_end, read_chr, device=None, return_stats=False):
    """float32[E] on the device: 1.0 for the edges utils/labels.py labels correct, 0.0 for the rest, in edge-id order.  Inputs are
    checked where they are (lengths, node ids in range, strands in {-1, +1}) before anything is launched.  return_stats=True
    also returns one dict per (chromosome, strand) problem with the STATS_FIELDS counters."""
    _host_checks(src, dst, num_nodes, read_strand, read_start, read_end, read_chr)
    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    n, E = int(num_nodes), int(src.numel())
    i32 = lambda t: t.to(dev, torch.int32).contiguous()   # noqa: E731
    i64 = lambda t: t.to(dev, torch.int64).contiguous()   # noqa: E731
    s_d, d_d = i32(src), i32(dst)
    strand, start, end, chrom = i32(read_strand), i64(read_start), i64(read_end), i32(read_chr)
    y = torch.empty(E, dtype=torch.float32, device=dev)
    rows = 0
    if return_stats and n:
        rows = int(torch.unique(chrom.to(torch.int64) * 2 + (strand > 0).to(torch.int64)).numel())
    stats = torch.zeros(1 + len(STATS_FIELDS) * rows, dtype=torch.int64, device=dev) if return_stats else None
    need = ctypes.c_size_t(0)
    _lib.check(lib.gnnome_edge_labels_workspace_bytes(n, E, ctypes.byref(need)), "edge_labels_workspace_bytes")
    ws = torch.empty(max(int(need.value), 1), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(lib.gnnome_edge_labels(_ptr(s_d), _ptr(d_d), E, n, _ptr(strand), _ptr(start), _ptr(end), _ptr(chrom), _ptr(y),
                                          _ptr(stats), rows, _ptr(ws), ws.numel(), _stream(dev)), "edge_labels")
    if not return_stats:
        return y
    h = stats.cpu().numpy()
    P = int(h[0])
    table = h[1:1 + len(STATS_FIELDS) * min(P, rows)].reshape(-1, len(STATS_FIELDS))
    return y, [dict(zip(STATS_FIELDS, (int(v) for v in row))) for row in table]


def process_graph(g, device=None):
    """utils/labels.py process_graph / process_graph_combo for a read_gfa(training=True) dict (or any dict with src, dst, num_nodes
    and the four read_* arrays) -> (gt_edge_ids int64, y float32[E]) on the device: the ids of the edges labelled 1 - the
    reference's gt_edges set of pairs, as edge ids - and the labels of every edge."""
    y = edge_labels(g["src"], g["dst"], g["num_nodes"], g["read_strand"], g["read_start"], g["read_end"], g["read_chr"], device=device)
    return torch.nonzero(y, as_tuple=True)[0], y


process_graph_combo = process_graph   # several chromosomes are grouped inside the kernel


def interval_union(g):
    """utils/labels.py:5-20 from the dict instead of a .dgl path: the merged [start, end] intervals of the strand +1 nodes, sorted
    by start (host)."""
    strand = np.asarray(g["read_strand"]).astype(np.int64)
    start = np.asarray(g["read_start"]).astype(np.int64)[strand == 1]
    end = np.asarray(g["read_end"]).astype(np.int64)[strand == 1]
    if start.size == 0:
        raise IndexError("interval_union: no strand +1 node")   # the reference's intervals[0] on an empty list
    order = np.argsort(start, kind="stable")
    result = [[int(start[order[0]]), int(end[order[0]])]]
    for s, e in zip(start[order[1:]].tolist(), end[order[1:]].tolist()):
        if s <= result[-1][1]:
            result[-1][1] = max(result[-1][1], e)
        else:
            result.append([s, e])
    return result


# ---- the union on the device (csrc/interval_union.hip) ---------------------------------------------------------------------------

def interval_union_tile_size():
    """Intervals per tile of the scans (csrc/interval_union.hip); results do not depend on it, the tests place their edges by it."""
    tile = ctypes.c_int(0)
    _lib.check(_lib.load().gnnome_interval_union_tile_size(ctypes.byref(tile)), "interval_union_tile_size")
    return int(tile.value)


class IntervalUnion:
    """The islands of one interval_union_device call, in (group, start) order.  group int32[K], start, end int64[K]: the islands;
    groups int32[G] ascending, covered int64[G] (the sum of end - start over the group's islands), count int64[G] (its islands);
    head uint8[M]: 1 where a selected read, in sorted order, opens an island.  All on the device."""

    def __init__(self, by, group, start, end, groups, covered, count, head):
        self.by, self.group, self.start, self.end = by, group, start, end
        self.groups, self.covered, self.count, self.head = groups, covered, count, head

    def __len__(self):
        return int(self.start.numel())

    def tolist(self):
        """by="all": the reference's list of [start, end]; by="chr": [chromosome, start, end] per island.  One copy to the host."""
        rows = torch.stack([self.group.to(torch.int64), self.start, self.end], 1).tolist()
        return [r[1:] for r in rows] if self.by == "all" else rows


def _as_tensor(t):
    return t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))


def _strand_text(strand):
    return "no node" if strand is None else f"no strand {int(strand):+d} node"


def interval_union_device(g, by="all", strand=1, device=None):
    """utils/labels.py:5-20 on the device -> IntervalUnion.  by="all" is the reference: the chromosome is ignored and .tolist() equals
    interval_union(g); by="chr" merges within each read_chr value, groups in ascending chromosome code.  strand: +1 (the reference),
    -1, or None for the reads of both strands, each interval taken as stored.  An interval opens a new island iff its start lies
    beyond every end before it in its group; start == that end merges.  Lengths and end >= start are checked on the
    device before the launch; no selected read raises the host function's IndexError."""
    if by not in ("all", "chr"):
        raise ValueError(f"interval_union: by={by!r}: expected 'all' or 'chr'")
    if strand not in (1, -1, None):
        raise ValueError(f"interval_union: strand={strand!r}: expected 1, -1 or None")
    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    names = ("read_strand", "read_start", "read_end") + (("read_chr",) if by == "chr" else ())
    cols = [_as_tensor(g[k]).reshape(-1).to(dev, torch.int64) for k in names]
    for k, t in zip(names[1:], cols[1:]):
        if t.numel() != cols[0].numel():
            raise ValueError(f"interval_union: {k} has {t.numel()} entries, read_strand {cols[0].numel()}")
    if cols[0].numel() >= (1 << 31):
        raise ValueError(f"interval_union: {cols[0].numel()} nodes: must be below 2^31")
    node = torch.arange(cols[0].numel(), device=dev) if strand is None else torch.nonzero(cols[0] == strand, as_tuple=True)[0]
    M = int(node.numel())
    if M == 0:
        raise IndexError(f"interval_union: {_strand_text(strand)}")   # the reference's intervals[0] on an empty list
    start, end = cols[1][node], cols[2][node]
    bad = torch.nonzero(end < start, as_tuple=True)[0]
    if bad.numel():
        i = int(bad[0])
        raise ValueError(f"interval_union: node {int(node[i])} ends at {int(end[i])}, before its start {int(start[i])}")
    order = torch.sort(start, stable=True).indices
    if by == "chr":
        chrom = cols[3][node]
        if int(chrom.min()) < _I32[0] or int(chrom.max()) > _I32[1]:
            raise ValueError("interval_union: read_chr does not fit int32")
        order = order[torch.sort(chrom[order], stable=True).indices]
        group = chrom[order].to(torch.int32)
        G = int(torch.unique_consecutive(group).numel())
    else:
        group, G = torch.zeros(M, dtype=torch.int32, device=dev), 1
    start, end = start[order].contiguous(), end[order].contiguous()
    head = torch.empty(M, dtype=torch.uint8, device=dev)
    isl_group = torch.empty(M, dtype=torch.int32, device=dev)
    isl_start, isl_end = (torch.empty(M, dtype=torch.int64, device=dev) for _ in range(2))
    grp_code = torch.empty(G, dtype=torch.int32, device=dev)
    grp_covered, grp_count = (torch.empty(G, dtype=torch.int64, device=dev) for _ in range(2))
    need = ctypes.c_size_t(0)
    _lib.check(lib.gnnome_interval_union_workspace_bytes(M, ctypes.byref(need)), "interval_union_workspace_bytes")
    ws = torch.empty(max(int(need.value), 1), dtype=torch.uint8, device=dev)
    result = (ctypes.c_int64 * 2)()
    with _on(dev):
        _lib.check(lib.gnnome_interval_union(_ptr(start), _ptr(end), _ptr(group), M, _ptr(head), _ptr(isl_group), _ptr(isl_start),
                                             _ptr(isl_end), G, _ptr(grp_code), _ptr(grp_covered), _ptr(grp_count), result, _ptr(ws),
                                             ws.numel(), _stream(dev)), "interval_union")
    K = int(result[0])
    return IntervalUnion(by, isl_group[:K], isl_start[:K], isl_end[:K], grp_code, grp_covered, grp_count, head)


def reference_coverage(g, ref_length=None, device=None):
    """How much of the reference the strand +1 reads can reconstruct, per chromosome (interval_union_device(g, by="chr")) ->
    {"chromosomes": {code: {"covered", "islands", "longest_island"[, "fraction"]}}, "covered", "islands", "longest_island"[,
    "fraction"]}: covered bases (the honest ref_length of calculate_NG50 / quick_evaluation), the number of islands (a lower bound on
    the contigs of a perfect assembly) and the longest one.  ref_length: an int - the whole reference, giving the total's fraction -
    or a dict by chromosome code, giving every chromosome's and, over the sum of the dict, the total's.  One copy to the host."""
    u = interval_union_device(g, by="chr", strand=1, device=device)
    rank = torch.searchsorted(u.groups.to(torch.int64), u.group.to(torch.int64))
    longest = torch.zeros_like(u.covered).scatter_reduce_(0, rank, u.end - u.start, "amax", include_self=False)
    codes, covered, islands, longest = torch.stack([u.groups.to(torch.int64), u.covered, u.count, longest]).tolist()
    per_chr = isinstance(ref_length, dict)
    if per_chr:
        missing = [c for c in codes if c not in ref_length]
        if missing:
            raise ValueError(f"reference_coverage: ref_length has no entry for chromosome {missing[0]}")
    report = {"chromosomes": {}, "covered": sum(covered), "islands": sum(islands), "longest_island": max(longest)}
    for c, cov, n, lng in zip(codes, covered, islands, longest):
        row = {"covered": cov, "islands": n, "longest_island": lng}
        if per_chr:
            row["fraction"] = cov / ref_length[c]
        report["chromosomes"][c] = row
    if ref_length is not None:
        report["fraction"] = report["covered"] / (sum(ref_length.values()) if per_chr else ref_length)
    return report
