"""The walk checks of utils/analyze.py on the device: whether a decoded walk switches strand or chromosome, or steps between two reads
that do not overlap on the reference - read off the read positions a training graph carries (read_gfa(training=True): read_strand,
read_start, read_end, read_chr), without an outside aligner.

    audit = analyze.audit_walks(g, walks)          # one gather pass over all walks (csrc/walk_audit.hip)
    audit.counts                                    # int32[W, 3] on the device: strand, chromosome, overlap findings per walk
    audit.overlap.walk, audit.overlap.idx, ...      # the findings as device tensors, ordered by walk, then by idx
    print(audit.text(0).overlap, end="")            # what the reference's assert_overlap(graph, walks[0]) prints

The reference's functions are restated finding for finding, quirks included (tests/walk_audit_statement.py): strand and chromosome are
compared with walk[0], every differing node is a finding, and their printed `walk index` enumerates walk[1:]; assert_overlap reports a
pair only when both strands are 1 (dst_start > src_end) or both are -1 (dst_end < src_start) and never looks at the chromosome.
assert_strand, assert_chromosome and assert_overlap keep the reference's call shape and print its text.

Declined, each before or without touching memory out of range: an empty walk (ValueError; the reference: IndexError on walk[0]), a node
id outside [0, N) (IndexError - Python's wrap-around of a negative index in the reference is NOT reproduced), a graph without one of the
four arrays (KeyError), no GPU (RuntimeError: there is no CPU path).
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from .contigs import _walk_arrays

NODE_ARRAYS = ("read_strand", "read_start", "read_end", "read_chr")
RULE = "-" * 20

NodeFindings = namedtuple("NodeFindings", "walk idx node")                  # analyze.py:6-8, :16-18
OverlapFindings = namedtuple("OverlapFindings", "walk idx src dst end start")   # analyze.py:30-33, :35-38: `end` and `start` as printed
WalkText = namedtuple("WalkText", "strand chromosome overlap")

_STRAND, _CHR, _OVERLAP, _BAD_MAP, _BAD_NODE = 1, 2, 4, 64, 128


def _device(device):
    if device is not None:
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"the walk audit runs on an MI355X only, not on {device}: there is no CPU path")
    if not torch.cuda.is_available():
        raise RuntimeError("the walk audit runs on an MI355X only: no HIP device is visible and there is no CPU path")
    return device if device is not None and device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _node_arrays(g, device):
    """the four int64[N] arrays of a read_gfa(training=True) dict, or of anything with them under `ndata`, on `device`"""
    table = g if isinstance(g, dict) or not hasattr(g, "ndata") else g.ndata
    cols = []
    for name in NODE_ARRAYS:
        try:
            col = table[name]
        except (KeyError, IndexError, TypeError):
            raise KeyError(f"the graph carries no {name} (read_gfa(training=True) adds the read positions)") from None
        if col is None:
            raise KeyError(f"the graph carries no {name} (read_gfa(training=True) adds the read positions)")
        cols.append(torch.as_tensor(col).reshape(-1).to(device, torch.int64).contiguous())
    if any(c.numel() != cols[0].numel() for c in cols):
        raise ValueError("the graph's " + ", ".join(NODE_ARRAYS) + " differ in length: " + ", ".join(str(c.numel()) for c in cols))
    return cols


def _lines(rows):
    return "".join(f"{RULE}\nwalk index: {idx}\nnode index: {node}\n" for idx, node in rows)


class WalkAudit:
    """What audit_walks found.  counts: int32[W, 3] (strand, chromosome, overlap) on the device; strand, chromosome: NodeFindings
    (walk, idx, node); overlap: OverlapFindings (walk, idx, src, dst, end, start) - int64 device tensors, one entry per finding, ordered
    by walk and then by idx: the order in which a loop of the reference's calls over the walks prints.  idx, end and start are the
    numbers the reference prints."""

    def __init__(self, num_walks, counts, strand, chromosome, overlap):
        self.num_walks, self.counts, self.strand, self.chromosome, self.overlap = num_walks, counts, strand, chromosome, overlap
        self._host = None

    def __len__(self):
        return self.num_walks

    def _rows(self):
        """the findings on the host (copied once) with, per list, where each walk's findings begin"""
        if self._host is None:
            host = []
            for found in (self.strand, self.chromosome, self.overlap):
                cols = torch.stack(list(found), 1).cpu().numpy() if found.walk.numel() else np.zeros((0, len(found)), dtype=np.int64)
                host.append((cols, np.searchsorted(cols[:, 0], np.arange(self.num_walks + 1))))
            self._host = host
        return self._host

    def text(self, i):
        """-> WalkText(strand, chromosome, overlap): what assert_strand, assert_chromosome and assert_overlap of the reference print
        for walk i (utils/analyze.py:6-8, :16-18, :30-38); '' where a check finds nothing."""
        if not 0 <= i < self.num_walks:
            raise IndexError(f"walk {i} of {self.num_walks}")
        (s, s_at), (c, c_at), (o, o_at) = self._rows()
        return WalkText(_lines(s[s_at[i]:s_at[i + 1], 1:].tolist()), _lines(c[c_at[i]:c_at[i + 1], 1:].tolist()),
                        "".join(f"{RULE}\nwalk index: {idx}\nnodes not connected: {src}, {dst}\nend: {end}, start: {start}\n"
                                for idx, src, dst, end, start in o[o_at[i]:o_at[i + 1], 1:].tolist()))


def audit_walks(g, walks, device=None):
    """utils/analyze.py:1-38 over all `walks` (lists of node ids, as decode returns them; or (int32 nodes, int64 offsets[W+1])) of the
    graph `g` (a read_gfa(training=True) dict, or anything with the four arrays, also under `.ndata`) -> WalkAudit.  One kernel pass and
    one synchronisation (the check of the flag bytes); the finding lists are torch nonzero + gathers of the flag bytes."""
    dev = _device(device)
    strand, start, end, chrom = cols = _node_arrays(g, dev)
    N = strand.numel()
    try:
        nodes, off = _walk_arrays(walks)
    except OverflowError:
        raise IndexError(f"a walk holds a node id outside [0, {N})") from None
    W, T = off.numel() - 1, nodes.numel()
    lengths = off[1:] - off[:-1]
    if W and int(lengths.min()) <= 0:
        raise ValueError(f"walk {int((lengths <= 0).nonzero()[0])} is empty")
    if T >= 2 ** 31:
        raise ValueError(f"{T} walk positions: the audit takes fewer than 2^31")
    new = lambda n=0: torch.zeros(n, dtype=torch.int64, device=dev)   # noqa: E731
    if W == 0:
        return WalkAudit(0, torch.zeros((0, 3), dtype=torch.int32, device=dev), NodeFindings(new(), new(), new()),
                         NodeFindings(new(), new(), new()), OverlapFindings(*(new() for _ in range(6))))
    nodes = nodes.to(dev, torch.int32).contiguous()
    ptr = off.to(dev, torch.int64)
    walk_id = torch.repeat_interleave(torch.arange(W, dtype=torch.int32, device=dev), ptr[1:] - ptr[:-1], output_size=T)
    flags, counts = ops.walk_audit(ptr.to(torch.int32), nodes, walk_id, *cols)
    worst = int(flags.max())                                        # the one synchronisation
    if worst & _BAD_NODE:
        t = int((flags >= _BAD_NODE).nonzero()[0])
        w = int(walk_id[t])
        raise IndexError(f"walk {w}: node {int(nodes[t])} at position {t - int(ptr[w])} is outside [0, {N})")
    if worst & _BAD_MAP:
        raise _lib.GnnomeHipError("walk_audit: a position lies outside its walk (walk_ptr / walk_id disagree)")

    def positions(bit):
        t = (flags & bit).nonzero().reshape(-1)
        w = walk_id[t].long()
        return t, w, t - ptr[w]

    node = nodes.long()
    t, w, at = positions(_STRAND)
    found_strand = NodeFindings(w, at - 1, node[t])
    t, w, at = positions(_CHR)
    found_chr = NodeFindings(w, at - 1, node[t])
    t, w, at = positions(_OVERLAP)
    src, dst = node[t], node[t + 1]                                 # bit 2 is never set at a walk's last position
    plus = strand[src] == 1
    found_overlap = OverlapFindings(w, at, src, dst, torch.where(plus, end[src], start[src]), torch.where(plus, start[dst], end[dst]))
    return WalkAudit(W, counts, found_strand, found_chr, found_overlap)


def _one(graph, walk):
    return audit_walks(graph, [walk]).text(0)


def assert_strand(graph, walk):
    """utils/analyze.py:1-8 with its call shape and its printed text; graph: the read_gfa dict or a DGL-like object with `ndata`."""
    print(_one(graph, walk).strand, end="")


def assert_chromosome(graph, walk):
    """utils/analyze.py:11-18."""
    print(_one(graph, walk).chromosome, end="")


def assert_overlap(graph, walk):
    """utils/analyze.py:21-38."""
    print(_one(graph, walk).overlap, end="")


def print_graph_info(idx, graph):
    """utils/analyze.py:41-46: the index, node count and edge count of a DGL-like graph (num_nodes(), edges()).  Print only."""
    print("\n---- GRAPH INFO ----")
    for label, value in (("Graph index:", idx), ("Number of nodes:", graph.num_nodes()), ("Number of edges:", len(graph.edges()[0]))):
        print(label, value)


def print_prediction(walk, current, neighbors, actions, choice, best_neighbor):
    """utils/analyze.py:49-57: one step of a walk under construction.  Print only."""
    print("\n-----predicting-----")
    rows = (("previous:\t", walk[-2] if len(walk) >= 2 else None), ("current:\t", current), ("neighbors:\t", neighbors[current]),
            ("actions:\t", actions.tolist()), ("choice:\t\t", choice), ("ground truth:\t", best_neighbor))
    for label, value in rows:
        print(label, value)
