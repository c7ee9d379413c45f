"""Ground-truth edge labels for training, on the MI355X (utils/labels.py; graph_parser.py:387-400 with training=True).

    g = gfa.read_gfa("asm.gfa", reads_path="reads.fasta", training=True)     # g["y"]: these labels, computed here
    gt_edge_ids, y = process_graph(g)                                        # y float32[E] in edge-id order
    merged = interval_union(g)                                               # the strand +1 reads' [start, end] union

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
