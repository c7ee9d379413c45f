"""Pop the simple bubbles of an overlap graph on the MI355X: the last of the steps hifiasm's r_utg and raven's graph have had done to them
before the reference trains and decodes on them.

    arms = bubble_arms(g)                                 # first, last, source, sink, nodes, weight, overlap, dist per arm
    mark = bubble_nodes(g, keep=None)                     # bool[N]: the nodes of every losing arm, and their complements (one round)
    s = pop_bubbles(g, rounds=4)                          # rounds of it, the edges at marked nodes dropped, the graph compacted

`g`: a graph dict of this package that follows the complement convention and whose kept edges are closed under mates, with prefix_length
= read_length[src] - overlap_length on every edge - as overlapper.overlap_graph and simplify.simplify_graph give it; anything else is a
ValueError before a kernel is launched (unitigs' checks).  The rule is stated in include/gnnome_hip.h and, executable, in
tests/bubble_statement.py; the kernels are csrc/bubbles.hip: the arm records (one lane per chain), the judgement (one wavefront per source
node, its out-row tiled through LDS) and the node mark.  The chains of any length come from the ranking of unitigs.py, so no lane walks
along an arm and no unitig compaction is needed between rounds.  torch does the plumbing: degrees, the prefix sums of weight and
read_length in chain order, the sort of the kept edges by (src, dst) and its row pointer, the gathers.  Not here: bubbles with a
direct-edge arm, bubbles whose arms branch (superbubbles), t == s ^ 1."""
import ctypes

import torch

from . import _lib
from .ops import _on, _ptr, _stream
from .overlapper import _Stages
from .unitigs import _chains, _columns

ARM_KEYS = ("first", "last", "source", "sink", "nodes", "weight", "overlap", "dist")
_ARM_WORDS = 5                                # int64 words of one arm record: {int32 s, t} {int32 key, nodes} weight overlap dist


class _SummedStages(_Stages):
    """_Stages for calls that pass a stage once per round: the times of equal names are added."""

    def finish(self):
        if self.stats is not None:
            self.marks[-1][1].synchronize()
            total = {}
            for (_, a), (name, b) in zip(self.marks, self.marks[1:]):
                total[name + "_ms"] = total.get(name + "_ms", 0.0) + a.elapsed_time(b)
            self.stats.update(total)


def bubble_tile_size():
    """Out-edges of one source the judgement kernel holds in LDS at a time; results do not depend on it, the tests place their hub by it."""
    tile = ctypes.c_int(0)
    _lib.check(_lib.load().gnnome_bubble_tile_size(ctypes.byref(tile)), "bubble_tile_size")
    return int(tile.value)


def _bounds(max_dist, max_diff):
    if int(max_dist) != max_dist or abs(max_dist) >= (1 << 62):
        raise ValueError(f"max_dist={max_dist}: an absolute number of bases, an int")
    if int(max_diff) != max_diff or max_diff < 0 or max_diff >= (1 << 62):
        raise ValueError(f"max_diff={max_diff}: an absolute number of bases, an int >= 0")
    return int(max_dist), int(max_diff)


def _weight(weight, N, dev):
    """-> int64[N] on the device; ValueError unless it is an int column with weight[v] == weight[v ^ 1]."""
    if weight is None:
        return torch.ones(N, dtype=torch.int64, device=dev)
    w = torch.as_tensor(weight)
    if w.is_floating_point() or w.is_complex() or w.dtype == torch.bool or w.dim() != 1 or w.numel() != N:
        raise ValueError(f"weight: expected an int column with {N} entries, one per node")
    w = w.to(dev, torch.int64).contiguous()
    if N and (not bool(torch.equal(w[0::2], w[1::2])) or int(w.abs().max()) >= (1 << 31)):
        raise ValueError("weight: weight[v] == weight[v ^ 1] and entries below 2^31 expected")
    return w


def _keep(keep, E, dev):
    if keep is None:
        return None
    keep = torch.as_tensor(keep).to(dev).reshape(-1)
    if keep.dtype != torch.bool or keep.numel() != E:
        raise ValueError(f"keep: expected bool[{E}]")
    return keep


def _arms(src, dst, ol, rl, w, N, c, stages, grid):
    """The arm records of the chains `c` on the (kept) edges src, dst -> int64[U, 5], one 40-byte record per chain."""
    dev, E, U = src.device, int(src.numel()), int(c["length"].numel())
    out_deg = torch.bincount(src, minlength=N).to(torch.int32)
    in_deg = torch.bincount(dst, minlength=N).to(torch.int32)
    # plumbing: one segmented pass over chain_nodes, as prefix sums the record kernel takes differences of
    order = c["chain_nodes"].long()
    cum_w, cum_l = (torch.zeros(N + 1, dtype=torch.int64, device=dev) for _ in range(2))
    torch.cumsum(w[order], 0, out=cum_w[1:])
    torch.cumsum(rl[order], 0, out=cum_l[1:])
    in_edge, out_edge = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2))
    rec = torch.empty((U, _ARM_WORDS), dtype=torch.int64, device=dev)
    circular = c["circular"].to(torch.uint8)
    stages.mark("bubble_lists")
    if N and U:
        with _on(dev):
            _lib.check(_lib.load().gnnome_bubble_arms(_ptr(src), _ptr(dst), _ptr(ol), _ptr(in_deg), _ptr(out_deg), N, E, _ptr(c["chain_off"]),
                                                      _ptr(c["chain_nodes"]), _ptr(circular), _ptr(c["length"]), _ptr(cum_w), _ptr(cum_l), U,
                                                      _ptr(in_edge), _ptr(out_edge), _ptr(rec), int(grid), _stream(dev)), "bubble_arms")
    stages.mark("bubble_arms")
    return rec


def _round(src, dst, p, ol, rl, w, N, max_dist, max_diff, stages, grid):
    """One round on the edges given -> bool[N]."""
    dev, E = src.device, int(src.numel())
    c = _chains(src, dst, p, ol, rl, N, stages, grid)
    U = int(c["length"].numel())
    rec = _arms(src, dst, ol, rl, w, N, c, stages, grid)
    mark = torch.zeros(N, dtype=torch.uint8, device=dev)
    if N and U and E >= 2:
        # plumbing: the edges by (src, dst) and where every row starts
        s_dst = dst[torch.sort(src * N + dst, stable=True).indices].to(torch.int32)
        row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(src, minlength=N), 0, out=row_ptr[1:])
        loser = torch.empty(U, dtype=torch.uint8, device=dev)
        stages.mark("bubble_sort")
        lib = _lib.load()
        with _on(dev):
            _lib.check(lib.gnnome_bubble_judge(_ptr(row_ptr), _ptr(s_dst), _ptr(c["unitig"]), _ptr(c["rank"]), _ptr(rec), N, E, U, max_dist,
                                               max_diff, _ptr(loser), int(grid), _stream(dev)), "bubble_judge")
            stages.mark("bubble_judge")
            _lib.check(lib.gnnome_bubble_mark(_ptr(c["unitig"]), _ptr(loser), N, U, _ptr(mark), int(grid), _stream(dev)), "bubble_mark")
        stages.mark("bubble_mark")
    return mark.bool()


def _pop(src, dst, p, ol, rl, N, keep, rounds, weight, max_dist, max_diff, stages, grid=0):
    """Rounds of the rule on the edges of `keep` (bool[E] or None) -> (bool[N] every node marked, the rounds that marked one, bool[E] the
    edges that are left).  The arguments are checked before the first launch."""
    dev, E = src.device, int(src.numel())
    if int(rounds) != rounds or rounds < 1:
        raise ValueError(f"rounds={rounds}: an int >= 1")
    max_dist, max_diff = _bounds(max_dist, max_diff)
    w = _weight(weight, N, dev)
    keep = torch.ones(E, dtype=torch.bool, device=dev) if keep is None else keep.clone()
    total, done = torch.zeros(N, dtype=torch.bool, device=dev), 0
    for _ in range(int(rounds)):
        sel = torch.nonzero(keep).squeeze(1)
        mark = _round(src[sel], dst[sel], p[sel], ol[sel], rl, w, N, max_dist, max_diff, stages, grid)
        if not bool(mark.any()):
            break
        total |= mark
        keep &= ~mark[src] & ~mark[dst]
        done += 1
    if stages.stats is not None:
        stages.stats["bubble_rounds"] = done
    return total, done, keep


def bubble_arms(g, keep=None, weight=None, device=None, stats=None):
    """-> dict of int64 device tensors, one entry per arm, in ascending order of the arm's first node: first, last (a_1, a_k), source, sink
    (s, t), nodes (k), weight, overlap, dist - on the graph restricted to the edges of `keep` (bool[E]; None: all).  weight: an int column
    per node with weight[v] == weight[v ^ 1] (None: 1 per node; on a unitig graph the reads per unitig, chain_off.diff()).  stats: a dict
    that receives unitig_chains' entries and bubble_lists_ms (torch), bubble_arms_ms (two launches)."""
    src, dst, p, ol, rl, N, dev = _columns(g, device)
    keep = _keep(keep, int(src.numel()), dev)
    w = _weight(weight, N, dev)
    if keep is not None:
        src, dst, p, ol = src[keep], dst[keep], p[keep], ol[keep]
    stages = _SummedStages(stats, dev)
    c = _chains(src, dst, p, ol, rl, N, stages)
    rec = _arms(src, dst, ol, rl, w, N, c, stages, 0)
    words = rec.view(torch.int32).reshape(-1, 2 * _ARM_WORDS)
    arm = torch.nonzero(words[:, 0] >= 0).squeeze(1)
    first = c["chain_nodes"].long()[c["chain_off"][:-1][arm]]
    arm = arm[torch.sort(first).indices]
    off, nodes = c["chain_off"], c["chain_nodes"].long()
    out = {"first": nodes[off[:-1][arm]], "last": nodes[off[1:][arm] - 1], "source": words[arm, 0].long(), "sink": words[arm, 1].long(),
           "nodes": words[arm, 3].long(), "weight": rec[arm, 2], "overlap": rec[arm, 3], "dist": rec[arm, 4]}
    stages.mark("bubble_gather")
    stages.finish()
    return out


def bubble_nodes(g, keep=None, weight=None, max_dist=50000, max_diff=1000, device=None, stats=None, grid=0):
    """-> bool[N] on the device, one round of the rule on the graph restricted to the edges of `keep` (bool[E]; None: all): the arms that
    share their source s and sink t are a bubble; its winner has the largest (weight, overlap, -min(a_1, a_k ^ 1)); another arm of it is
    a loser iff dist(winner) <= max_dist, dist(arm) <= max_dist and |dist(arm) - dist(winner)| <= max_diff (absolute numbers of bases, for
    the reason fuzz is); the nodes of every loser and their complements are marked.  All bubbles are judged on the input at once.  stats: a
    dict that receives unitig_chains' entries (the ranking of the kept edges) and bubble_lists_ms (torch), bubble_arms_ms, bubble_sort_ms
    (torch), bubble_judge_ms, bubble_mark_ms.  grid: workgroups per launch (0: by size); no result depends on it, the tests vary it."""
    src, dst, p, ol, rl, N, dev = _columns(g, device)
    keep = _keep(keep, int(src.numel()), dev)
    max_dist, max_diff = _bounds(max_dist, max_diff)
    w = _weight(weight, N, dev)
    if keep is not None:
        src, dst, p, ol = src[keep], dst[keep], p[keep], ol[keep]
    stages = _SummedStages(stats, dev)
    mark = _round(src, dst, p, ol, rl, w, N, max_dist, max_diff, stages, grid)
    stages.finish()
    return mark


def pop_bubbles(g, rounds=4, keep=None, weight=None, max_dist=50000, max_diff=1000, device=None, stats=None, grid=0, compact=True,
                check_mates=True):
    """-> a new graph dict of simplify.simplify_graph's shape: bubble_nodes on the edges of `keep`, the edges at marked nodes dropped, and
    again on what is kept, until a round marks nothing or `rounds` of them have run - a bubble inside an arm of another goes first and
    leaves a longer plain arm.  The edges keep their relative order; compact, the gathered columns, kept_reads and edge_origin are
    simplify_graph's; removed = {"bubble_nodes" (nodes marked by all rounds), "bubble_rounds" (the rounds that marked one), "reads"}.
    check_mates: ValueError when the kept edges are not closed under mates (the input's are checked by every round's ranking).  stats:
    bubble_nodes' entries, added up over the rounds, bubble_rounds and compact_ms."""
    from .simplify import _kept_graph
    src, dst, p, ol, rl, N, dev = _columns(g, device)
    keep = _keep(keep, int(src.numel()), dev)
    stages = _SummedStages(stats, dev)
    total, done, keep = _pop(src, dst, p, ol, rl, N, keep, rounds, weight, max_dist, max_diff, stages, grid)
    out = _kept_graph(g, src, dst, N, keep, {"bubble_nodes": int(total.sum()), "bubble_rounds": done}, compact, check_mates, dev)
    stages.mark("compact")
    stages.finish()
    return out
