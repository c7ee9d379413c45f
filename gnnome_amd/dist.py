"""Whole-graph inference partitioned by destination-node range, one process per GPU.

The reference has no multi-GPU code at all (it scores whole graphs on the CPU "because GPU memory",
inference.py:388).  This is the north_star's scheme:

  * rank p OWNS a contiguous node range [lo_p, hi_p), chosen so that every rank has about the same
    number of incident edges;
  * it stores every edge INCIDENT to an owned node - in-edges and out-edges - plus the far endpoints
    of those edges as HALO nodes.  Local node ids put owned nodes first, so after the usual
    destination sort the in-edges of owned nodes are a PREFIX of the local edge storage;
  * a cut edge lives on two ranks; both compute the identical e' (it depends only on h[src], h[dst]
    and e), so edge state never travels;
  * once per layer the owners send the h rows their peers hold as halo: a packed all_to_all_single
    over RCCL/xGMI (direct peer-to-peer, per-link bound), received straight into the halo rows of h.
    The node projection of the owned rows runs while the exchange is in flight;
  * the scorer writes the logits of owned in-edges (every global edge exactly once) as one contiguous piece in
    sorted order; ONE all_gather of the pieces (E*4/G bytes each, padded to the largest) and one index_select
    through a map built with the plan put them into global edge-id order (SURVEY.md 8e "Scorer").

Every sequence on a partition - eval or training step, whichever model - reads what its rank scores from part.scored (ScoredRows: the rows,
the views that segment them, the score views, count and total), ends in engine.score_tail (PartitionedGraph.logits_finish says how: alone,
or padded piece + assembly) and makes its node projection with engine.project_rows; what a partition refuses is check_shard's to say.

GatedGCNModel runs on the in-edge-only form of the partition (engine_gated.py) - with directed=False on the in-edge-only partition of the
DOUBLED edge list (full_graph.py:47-51; from_global(..., in_edges_only=True, doubled=True) over the original edges): the reverse copy of
edge k, id E + k, lives with the owner of src[k], both copies carry edge k's features (enc_rows), the stack and bn_e's statistics run over
the 2E rows, and only the copies with ids below E are scored (score_rows), each by the owner of its dst; a rank all of whose in-edges are
reverse copies scores nothing and still enters every collective.  Run over gloo and on ranks sharing one GPU - never on two devices.
Still refused for this model on partitions: CapturedPartitionedForward, training_step = "symmetric", bf16 storage and recompute_gate.
GCNModel and SAGEModel on the default one, with one
exchange of h and one forward-direction exchange of its gradient per layer and neighbour sums bit-equal to the single-rank run
(engine_baselines.py, "destination-range partitions"); GATModel on the default one too, through GATPartitionedRunner: one exchange of h
per layer forward, the halo rows of the projection made locally, and two forward-direction exchanges per layer backward - dA's halo rows
and the 64-byte work rows between the two phases of the attention sum's backward (engine_gat.py, "destination-range partitions").
PartitionedRunner itself keeps refusing GATModel and names that class.  The GAT path has run as processes sharing one GPU and as CPU
ranks over gloo only - never on two devices.

SymGatedGCNModel's pass over dgl.reverse(g) (train.py:159-170, the symmetry loss) runs on the same plan with reverse=True: owned nodes,
scored edges, BatchNorm rows and the halo plan do not depend on the orientation, only the roles of the projection's column blocks and of
the two lists do ("Symmetry step").  Run over gloo and on ranks sharing one GPU - never on two devices.

All tensor math goes through an `ops` namespace exactly like engine.run_stack: the product passes
gnnome_amd.ops (HIP); the CPU/gloo tests pass the checker backend to exercise this host logic.
"""
import functools
import os

import torch
import torch.distributed as dist

from . import engine, engine_gated
from . import ops as hip_ops


def force_collectives():
    """GNNOME_FORCE_COLLECTIVES=1: a single-rank process group still ISSUES every collective of the partitioned path (halo
    all_to_all both ways, BatchNorm statistics all_gather, BatchNorm-backward and gradient all_reduce, logits all_gather) instead
    of taking the world == 1 shortcuts - the way a one-GPU box runs this module's RCCL calls (tests/test_hip_partition.py).
    A one-rank collective is the identity, so the results must equal the plain path bit for bit - in training too: one rank's statistics
    are the whole graph's, so the step keeps the single-rank BatchNorm kernels and sends their moments and backward sums through the
    collectives (PartitionShard.sync_moments, sum_ranks) instead of merging them on the host."""
    return os.environ.get("GNNOME_FORCE_COLLECTIVES", "0") == "1"


def _alone(world):
    """True when the world == 1 shortcuts apply."""
    return world == 1 and not force_collectives()


def split_by_incident_edges(src, dst, num_nodes, world):
    """Node-range boundaries [b_0=0, ..., b_world=N] balancing in-degree + out-degree per range."""
    deg = torch.bincount(dst.long(), minlength=num_nodes) + torch.bincount(src.long(), minlength=num_nodes)
    return split_by_degree(deg, num_nodes, world)


def split_by_degree(deg, num_nodes, world):
    """The same boundaries from the per-node incident-edge counts (from_slices all-reduces them over the ranks' slices)."""
    csum = torch.cumsum(deg + 1, 0)  # +1: isolated nodes still cost a node update
    total = int(csum[-1]) if num_nodes > 0 else 0
    bounds = [0]
    for p in range(1, world):
        target = total * p // world
        b = int(torch.searchsorted(csum, torch.tensor(target, device=csum.device), right=False))
        bounds.append(max(bounds[-1], min(b, num_nodes)))
    bounds.append(num_nodes)
    return bounds


def _checked_bounds(bounds, num_nodes, world):
    bounds = [int(b) for b in bounds]
    if len(bounds) != world + 1 or bounds[0] != 0 or bounds[-1] != num_nodes or any(a > b for a, b in zip(bounds[:-1], bounds[1:])):
        raise ValueError(f"bounds={bounds}: expected {world + 1} ascending node ids from 0 to {num_nodes}")
    return bounds


def partition_census(src, dst, num_nodes, world, bounds=None):
    """What PartitionedGraph.from_global would give every rank of a `world`-way destination-range partition, computed in one
    process without a process group (planning: which world size a graph wants; tools/partition_stats.py):
    per rank the owned nodes, local edges (incident to an owned node), owned in-edges (the ones it scores), halo rows it
    receives and rows it sends per layer.  Pure index arithmetic over the edge list, O(E) per rank.
    The `in_edge_*` counts are those of from_global(..., in_edges_only=True), the partition a GatedGCNModel runs on: its local edges
    are the owned in-edges, its halo the distinct non-owned SOURCES of those."""
    src, dst = torch.as_tensor(src).long(), torch.as_tensor(dst).long()
    bounds = split_by_incident_edges(src, dst, num_nodes, world) if bounds is None else list(bounds)
    bt = torch.tensor(bounds[1:-1], device=src.device, dtype=torch.long)
    rs, rd = torch.bucketize(src, bt, right=True), torch.bucketize(dst, bt, right=True)   # owner rank of each endpoint
    cut = rs != rd
    ranks = []
    owned_in = torch.bincount(rd, minlength=world)
    local = owned_in + torch.bincount(rs[cut], minlength=world)
    # halo rows of rank p = distinct far endpoints of its cut edges: (p, node) pairs, counted once
    pair = torch.cat([rd[cut] * num_nodes + src[cut], rs[cut] * num_nodes + dst[cut]])
    pair = torch.unique(pair)
    holder, node = pair // num_nodes, pair % num_nodes
    owner = torch.bucketize(node, bt, right=True)
    recv = torch.bincount(holder, minlength=world)
    send = torch.bincount(owner, minlength=world)
    link = torch.bincount(owner * world + holder, minlength=world * world).view(world, world)   # rows owner -> holder
    pair_in = torch.unique(rd[cut] * num_nodes + src[cut])        # in-edge-only partition: (holder, source) pairs of the cut in-edges
    recv_in = torch.bincount(pair_in // num_nodes, minlength=world)
    send_in = torch.bincount(torch.bucketize(pair_in % num_nodes, bt, right=True), minlength=world)
    for p in range(world):
        ranks.append({"rank": p, "owned_nodes": bounds[p + 1] - bounds[p], "local_edges": int(local[p]), "owned_in_edges": int(owned_in[p]),
                      "halo_rows": int(recv[p]), "rows_sent_per_layer": int(send[p]), "largest_link_rows": int(link[p].max()),
                      "in_edge_local_edges": int(owned_in[p]), "in_edge_halo_rows": int(recv_in[p]),
                      "in_edge_rows_sent_per_layer": int(send_in[p])})
    e = int(src.numel())
    return {"world": world, "num_nodes": num_nodes, "num_edges": e, "bounds": bounds, "cut_edges": int(cut.sum()),
            "cut_fraction": float(cut.sum()) / max(e, 1), "edge_replication": float(local.sum()) / max(e, 1),
            "imbalance_local_edges": float(local.max()) * world / max(float(local.sum()), 1.0), "ranks": ranks}


class PartitionedGraph:
    """Rank-local piece of a destination-range partition plus its halo-exchange plan."""

    def __init__(self):
        self.rank = self.world = 0
        self.in_edges_only = False  # True: the local graph holds the in-edges of the owned nodes only (the partition of a one-direction model)
        self.lo = self.hi = self.n_own = self.n_local = self.num_edges_global = 0
        self.bounds = None
        self.node_gid = None        # int64 [n_local]  global id of local node (owned first, then halo ascending)
        self.edge_gid = None        # int64 [e_local]  global edge id of local edge (local edge-id order)
        self.views = None           # ops.GraphViews of the local graph
        self.n_score = 0            # in-edges of owned nodes = prefix of sorted positions
        self.srt_geid = None        # int32 [n_score]  global edge id of sorted position p
        self.send_idx = None        # int32 [sum(send_counts)] owned local rows to pack, grouped by peer
        self.send_counts = None     # python list, rows to send to each peer
        self.recv_counts = None     # python list, halo rows received from each peer (in halo order)
        self.node_perm = self.node_gather = None   # optional renumbering the ranges were cut in (caller's id -> internal id, and back)
        self.score_pad = 0          # rows of the padded logits piece every rank contributes to the all_gather
        self.score_index = None     # int64 [E_global]: where global edge id k sits in the flattened [world, score_pad] gather
        self._baseline = {}         # directed -> engine_baselines.PartitionPlan (scales of all local rows, lists, interior / boundary rows)
        # doubled=True: the plan of GatedGCNModel(directed=False), an in-edge-only partition of engine_gated.doubled_edge_list(src, dst)
        self.doubled = False
        self.num_edges_original = 0  # E of the caller's edge list; num_edges_global is then 2E, global id E + k the reverse copy of edge k
        self.enc_rows = None        # int64 [e_local]  the ORIGINAL edge whose features local edge row r carries (doubled_row_maps' enc_gather)
        self.score_rows = None      # int64 [n_score_original]  ascending sorted positions of the prefix whose global id is < E (score_gather)
        self.n_score_original = 0   # how many of them: the edges this rank scores; 0 is legal (every owned in-edge a reverse copy)
        self.scored = None          # ScoredRows: what this rank scores, as the scorer, its backward and the assembly read it - every plan has one

    @classmethod
    def from_global(cls, src, dst, num_nodes, rank, world, device, ops=hip_ops, group=None, node_perm=None, in_edges_only=False,
                    bounds=None, doubled=False):
        """Build from the full edge list (every rank holds it in this harness, as inference.py holds the
        whole DGLGraph).  The plan is computed on `device` (masks, unique, searchsorted over the E-sized edge list: 0.9 s per
        rank on the host at 10M edges) + one all_to_all of halo requests.
        node_perm (int64[N], the same on every rank; gnnome_amd.node_order.locality_order): the RANGES are cut in the renumbered
        node order - for graphs whose ids do not follow the layout; local_node_rows still takes rows in the caller's numbering.
        in_edges_only: the partition of a ONE-DIRECTION model (GatedGCNModel): the local graph holds the owned nodes, their in-edges -
        in global edge-id order within each destination run, so every owned node's sum has the whole graph's association - and as
        halo the distinct non-owned sources; no out-edge of an owned node into another range is kept, so every local edge is scored
        here (n_score = all of them) and halo nodes have empty in-lists.
        bounds: the range boundaries [0, ..., N] (the same on every rank) instead of split_by_incident_edges's.
        doubled (with in_edges_only=True only): the plan of GatedGCNModel(directed=False), full_graph.py:47-51.  src, dst stay the ORIGINAL
        E edges; the plan is the in-edge-only one of engine_gated.doubled_edge_list(src, dst) - edge k goes to the owner of dst[k], its
        reverse copy E + k to the owner of src[k], default bounds are split_by_incident_edges of the doubled list - and records enc_rows,
        score_rows and n_score_original; local_edge_rows takes the [E, ...] table of the original edges."""
        self = cls()
        self.in_edges_only = bool(in_edges_only)
        _check_doubled_flag(doubled, in_edges_only)
        src, dst = torch.as_tensor(src).to(device).long(), torch.as_tensor(dst).to(device).long()
        if node_perm is not None:
            self._set_node_perm(node_perm, num_nodes, device)
            src, dst = self.node_perm[src], self.node_perm[dst]
        if doubled:
            self.doubled, self.num_edges_original = True, int(src.numel())
            src, dst = engine_gated.doubled_edge_list(src, dst)
        self.rank, self.world, self.num_edges_global = rank, world, int(src.numel())
        self.bounds = split_by_incident_edges(src, dst, num_nodes, world) if bounds is None else _checked_bounds(bounds, num_nodes, world)
        lo, hi = self.bounds[rank], self.bounds[rank + 1]
        keep = (dst >= lo) & (dst < hi)
        if not self.in_edges_only:
            keep |= (src >= lo) & (src < hi)
        self.edge_gid = torch.nonzero(keep).squeeze(1)
        return self._build(src[keep], dst[keep], device, ops, group)

    @classmethod
    def from_slices(cls, src_slice, dst_slice, num_nodes, rank, world, device, ops=hip_ops, group=None, node_perm=None, in_edges_only=False,
                    bounds=None, doubled=False):
        """Build from a rank's SLICE of the edge list: rank r holds the edges with global ids [off_r, off_r + m_r), the slices in
        rank order making up the whole list (a reader that splits its input file G ways; no rank ever holds all E endpoints).
        Degrees are all-reduced ([N] int64) for the range boundaries, then every edge travels once to the owner of its
        destination and, when that is another rank, once to the owner of its source (one all_to_all of (src, dst, id) triples).
        The ids a rank receives arrive ascending - peer blocks in rank order, each ascending - so the local edge order, and with
        it every later array, equals from_global's.  The same route moves edge features: shuffle_edge_rows(e_slice).
        in_edges_only, bounds: as for from_global; an edge then travels to the owner of its destination only.
        doubled: as for from_global, from slices of the ORIGINAL edge list: edge k travels to the owner of dst[k] and its reverse copy, id
        E + k, to the owner of src[k].  A peer's block then holds ids below and above E, so the received records are put into ascending
        id order here; shuffle_edge_rows follows.  global_degrees, and with them local_degree_features, stay the ORIGINAL graph's:
        full_graph.py computes x before add_edges."""
        self = cls()
        self.in_edges_only = bool(in_edges_only)
        _check_doubled_flag(doubled, in_edges_only)
        src = torch.as_tensor(src_slice).to(device).long()
        dst = torch.as_tensor(dst_slice).to(device).long()
        if node_perm is not None:   # (as from_global: ranges over renumbered nodes; the permutation itself needs the whole graph once)
            self._set_node_perm(node_perm, num_nodes, device)
            src, dst = self.node_perm[src], self.node_perm[dst]
        self.rank, self.world = rank, world
        alone = _alone(world)
        m = torch.tensor([src.numel()], dtype=torch.int64, device=device)
        counts = m.view(1, 1) if alone else all_gather_rows(m, world, group)
        counts = counts.view(-1).tolist()
        self.num_edges_global = int(sum(counts))
        offset = int(sum(counts[:rank]))
        deg = torch.stack([torch.bincount(dst, minlength=num_nodes), torch.bincount(src, minlength=num_nodes)])   # in | out, this slice
        if not alone:
            all_reduce_sum(deg, group)
        self.global_degrees = deg        # [2, N] int64 of the WHOLE graph: what inference.py:416-420 z-scores into x
        incident = (deg[0] + deg[1]) * (2 if doubled else 1)   # (the doubled list: every edge counts at both ends twice)
        self.bounds = split_by_degree(incident, num_nodes, world) if bounds is None else _checked_bounds(bounds, num_nodes, world)
        bt = torch.tensor(self.bounds[1:-1], device=device, dtype=torch.long)
        gid = torch.arange(offset, offset + src.numel(), device=device)
        slice_row = torch.arange(src.numel(), device=device)      # the slice row whose features a record carries
        if doubled:
            self.doubled, self.num_edges_original = True, self.num_edges_global
            self.num_edges_global *= 2
            src, dst = engine_gated.doubled_edge_list(src, dst)
            gid, slice_row = torch.cat([gid, gid + self.num_edges_original]), torch.cat([slice_row, slice_row])
        owner_d, owner_s = torch.bucketize(dst, bt, right=True), torch.bucketize(src, bt, right=True)
        second = (owner_s != owner_d) if not self.in_edges_only else torch.zeros_like(owner_s, dtype=torch.bool)
        to_rank = torch.cat([owner_d, owner_s[second]])
        which = torch.cat([torch.arange(src.numel(), device=device), torch.nonzero(second).squeeze(1)])
        order = torch.argsort(to_rank * (self.num_edges_global + 1) + gid[which])     # by receiving rank, then by global id
        sent = which[order]
        self._slice_rows = slice_row[sent]                                             # slice row of every record sent
        self._slice_send = torch.bincount(to_rank, minlength=world).tolist()
        sc = torch.tensor(self._slice_send, dtype=torch.int64, device=device)
        rc = torch.empty(world, dtype=torch.int64, device=device)
        if alone:
            rc.copy_(sc)
        else:
            all_to_all_rows(rc, sc, None, None, group)
        self._slice_recv = rc.tolist()
        triples = torch.stack([src, dst, gid], 1)[sent].contiguous()
        got = torch.empty((sum(self._slice_recv), 3), dtype=torch.int64, device=device)
        if alone:
            got.copy_(triples)
        else:
            all_to_all_rows(got, triples, self._slice_recv, self._slice_send, group)
        self._slice_sort = None
        if doubled:   # a peer's block is ascending below E and again above it: one sort puts the whole list into from_global's order
            self._slice_sort = torch.argsort(got[:, 2])
            got = got[self._slice_sort]
        self.edge_gid = got[:, 2].contiguous()
        assert self.edge_gid.numel() < 2 or bool((self.edge_gid[1:] > self.edge_gid[:-1]).all()), "edge ids must arrive ascending"
        return self._build(got[:, 0].contiguous(), got[:, 1].contiguous(), device, ops, group)

    def shuffle_edge_rows(self, rows_slice):
        """[m_r, F] rows of this rank's edge slice (features, labels) -> the rows of its LOCAL edges, in local edge-id order (the
        route from_slices sent the endpoints along)."""
        if not hasattr(self, "_slice_rows"):
            raise RuntimeError("shuffle_edge_rows needs a plan built by from_slices")
        rows_slice = torch.as_tensor(rows_slice)
        flat = rows_slice.reshape(rows_slice.shape[0], -1).to(self._slice_rows.device)
        out = torch.empty((sum(self._slice_recv), flat.shape[1]), dtype=flat.dtype, device=flat.device)
        packed = flat[self._slice_rows].contiguous()
        if _alone(self.world):
            out.copy_(packed)
        else:
            all_to_all_rows(out, packed, self._slice_recv, self._slice_send, self._group)
        if self._slice_sort is not None:
            out = out[self._slice_sort]
        return out.reshape((out.shape[0],) + tuple(rows_slice.shape[1:]))

    def local_degree_features(self, reverse=False):
        """x rows of this rank's owned + halo nodes, [zscore(in_degree) | zscore(out_degree)] of the WHOLE graph (inference.py:416-420;
        mean and unbiased std in fp64, applied in fp32 like gnnome_degree_features_f32), from the degrees from_slices all-reduced.
        reverse: the two columns swapped - the x of the reversed pass (train.py:112-122,165-166; ops.degree_features): the degrees stay
        those of the original graph, dgl.reverse copies ndata and does not recompute it."""
        if not hasattr(self, "global_degrees"):
            raise RuntimeError("local_degree_features needs a plan built by from_slices")
        d = self.global_degrees.double()
        mean, std = d.mean(1, keepdim=True), d.std(1, keepdim=True)
        local = self.global_degrees[:, self.node_gid].float()
        z = (local - mean.float()) / std.float()
        return (z.flip(0) if reverse else z).t().contiguous()

    def _build(self, ls, ld, device, ops, group):
        """Everything after the rank knows its local edges (ls, ld: global endpoints, ascending global edge id)."""
        rank, world = self.rank, self.world
        self._group = group
        lo, hi = self.bounds[rank], self.bounds[rank + 1]
        self.lo, self.hi, self.n_own = lo, hi, hi - lo
        own_d = (ld >= lo) & (ld < hi)
        ends = torch.cat([ls, ld])
        halo = torch.unique(ends[(ends < lo) | (ends >= hi)])  # ascending => grouped by owner rank
        self.node_gid = torch.cat([torch.arange(lo, hi, device=halo.device), halo])
        self.n_local = int(self.node_gid.numel())

        def to_local(g):
            own = (g >= lo) & (g < hi)
            pos = torch.searchsorted(halo, g.clamp(min=0)) if halo.numel() else torch.zeros_like(g)
            return torch.where(own, g - lo, self.n_own + pos)

        l_src, l_dst = to_local(ls).int(), to_local(ld).int()
        self.views = ops.GraphViews(l_src, l_dst, self.n_local)
        in_ptr = self.views.in_ptr
        self.n_score = int(in_ptr[self.n_own]) if self.n_own > 0 else 0
        assert self.n_score == int(own_d.sum())
        srt_eid = self.views.srt_eid[:self.n_score].long()
        self.srt_geid = self.edge_gid[srt_eid].int()
        self.scored = ScoredRows(None, self.views, self.srt_geid, self.num_edges_global)   # the sorted prefix as it lies
        if self.doubled:
            # the ORIGINAL graph is scored (full_graph.py:51): the rows of the prefix with ids below E, every one on the owner of its destination
            E = self.num_edges_original
            self.enc_rows = torch.where(self.edge_gid >= E, self.edge_gid - E, self.edge_gid)
            self.score_rows = rows = torch.nonzero(self.srt_geid < E).squeeze(1)
            self.n_score_original = int(rows.numel())
            # views of the scored edges alone over the local nodes: the sub-list is already sorted by destination and the sort is stable
            seg = ops.GraphViews(self.views.srt_src[rows].contiguous(), self.views.srt_dst[rows].contiguous(), self.n_local)
            assert torch.equal(seg.srt_eid.long().cpu(), torch.arange(self.n_score_original)), "the scored rows must keep their order"
            self.scored = ScoredRows(rows.int(), seg, self.srt_geid[rows].contiguous(), E)

        # halo-exchange plan: tell each owner which of its rows I hold as halo
        bounds_t = torch.tensor(self.bounds, device=halo.device)
        owner = torch.searchsorted(bounds_t, halo, right=True) - 1
        self.recv_counts = torch.bincount(owner, minlength=world).tolist() if halo.numel() else [0] * world
        # (the plan travels on `device` tensors: RCCL moves device memory only, gloo takes either)
        req_counts = torch.tensor(self.recv_counts, dtype=torch.int64, device=device)
        got_counts = torch.empty(world, dtype=torch.int64, device=device)
        if not _alone(world):
            all_to_all_rows(got_counts, req_counts, None, None, group)
        else:
            got_counts.copy_(req_counts)
        self.send_counts = got_counts.tolist()
        wanted = torch.empty(sum(self.send_counts), dtype=torch.int64, device=device)
        if not _alone(world):
            all_to_all_rows(wanted, halo.contiguous(), self.send_counts, self.recv_counts, group)
        assert wanted.numel() == 0 or (int(wanted.min()) >= lo and int(wanted.max()) < hi)
        self.send_idx = (wanted - lo).int()
        self._plan_logits(device, group)
        return self

    def _plan_logits(self, device, group):
        """Assembly of the logits: every rank scores its owned in-edges (a prefix of its sorted positions) into one piece;
        the pieces are all-gathered (padded to the largest) and un-permuted with one index_select.  The map from global
        edge id to its slot in the gathered buffer is exchanged here, once."""
        world = self.world
        n_scored, ids, total = self.scored.count, self.scored.score_views.srt_eid, self.scored.total
        if _alone(world):
            self.score_pad, self.score_index = n_scored, None
            return
        counts = all_gather_rows(torch.tensor([n_scored], dtype=torch.int64, device=device), world, group).view(-1).tolist()
        self.score_pad = pad = max(max(counts), 1)
        mine = torch.full((pad,), -1, dtype=torch.int64, device=device)
        mine[:n_scored] = ids.long()
        every = all_gather_rows(mine, world, group).view(-1)                 # [world * pad] global edge ids, -1 = padding
        slots = torch.nonzero(every >= 0).squeeze(1)
        index = torch.full((total,), -1, dtype=torch.int64, device=device)
        index[every[slots]] = slots
        assert sum(counts) == total and (total == 0 or int(index.min()) >= 0), "every edge must be scored exactly once"
        self.score_index = index

    def assemble_logits(self, piece, group=None):
        """piece[score_pad] (this rank's owned in-edges in sorted order, tail unused) -> logits[E_global] in edge-id order,
        complete on every rank."""
        if _alone(self.world):
            raise RuntimeError("single rank: the scorer writes edge-id order itself")
        gathered = all_gather_rows(piece, self.world, group).view(-1)
        return gathered.index_select(0, self.score_index)

    def logits_finish(self, group=None):
        """How engine.score_tail ends on this plan, as its keyword arguments: nothing - a lone process scatters to the edge ids itself -
        or the padded piece every rank contributes and its assembly."""
        if _alone(self.world):
            return {}
        return dict(pad=self.score_pad, assemble=functools.partial(self.assemble_logits, group=group))

    def _set_node_perm(self, node_perm, num_nodes, device):
        self.node_perm = torch.as_tensor(node_perm).to(device=device, dtype=torch.int64)
        if self.node_perm.numel() != num_nodes:
            raise ValueError(f"node_perm has {self.node_perm.numel()} entries for {num_nodes} nodes")
        self.node_gather = torch.empty(num_nodes, dtype=torch.int64, device=device)
        self.node_gather[self.node_perm] = torch.arange(num_nodes, device=device)

    def local_node_rows(self, x_global):
        """Rows of this rank's owned + halo nodes out of a table in the CALLER's node numbering."""
        gid = self.node_gid if self.node_gather is None else self.node_gather[self.node_gid]
        return x_global[gid.to(x_global.device)]

    def local_edge_rows(self, e_global):
        """Rows of this rank's local edges, in local edge-id order.  A doubled plan takes the table of the ORIGINAL edges, [E, ...], and
        feeds a row to both copies of its edge (enc_rows)."""
        return e_global[(self.enc_rows if self.doubled else self.edge_gid).to(e_global.device)]


def _check_doubled_flag(doubled, in_edges_only):
    if doubled and not in_edges_only:
        raise ValueError("doubled=True is the plan of GatedGCNModel(directed=False), a one-direction model: it needs in_edges_only=True")


class ScoredRows:
    """What a rank scores, the one description the scorer, its backward and the assembly of the logits read (PartitionedGraph._build):
    `rows` - the sorted positions the scorer reads, int32, or None: the owned in-edges, the sorted prefix as it lies; `views` - graph views
    whose sorted order IS the scored rows' order, so their in- / out-lists segment the scorer's rows; `score_views` - their srt_src /
    srt_dst with, as srt_eid, the scored rows' ids in the complete logits; `count` rows are scored here (0 is legal on a doubled plan:
    every owned in-edge a reverse copy) and the complete logits have `total` entries."""

    def __init__(self, rows, views, ids, total):
        self.rows, self.views, self.score_views = rows, views, _ScoreViews(views, ids)
        self.count, self.total = int(ids.numel()), int(total)


def _staged(t, group):
    """gloo moves host memory only: device tensors take a round trip through the host under it.  That is the
    two-processes-on-one-GPU test configuration; RCCL ("nccl") works on device memory directly."""
    return t.is_cuda and dist.get_backend(group) == "gloo"


def all_to_all_rows(out, inp, out_counts, in_counts, group=None, async_op=False):
    """out <- row blocks from every peer (out_counts rows each), inp's blocks (in_counts) go out."""
    if _staged(out, group):
        o, i = torch.empty(out.shape, dtype=out.dtype), inp.cpu()
        dist.all_to_all_single(o, i, output_split_sizes=out_counts, input_split_sizes=in_counts, group=group)
        out.copy_(o)
        return None
    return dist.all_to_all_single(out, inp, output_split_sizes=out_counts, input_split_sizes=in_counts, group=group, async_op=async_op)


def all_reduce_sum(t, group=None):
    if _staged(t, group):
        c = t.cpu()
        dist.all_reduce(c, op=dist.ReduceOp.SUM, group=group)
        t.copy_(c)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def broadcast_from(t, src=0, group=None):
    """t <- the t of the group's rank `src`, in place (trainer.train_partitioned: what rank 0 drew)."""
    if group is not None:
        src = dist.get_global_rank(group, src)
    if _staged(t, group):
        c = t.cpu()
        dist.broadcast(c, src=src, group=group)
        t.copy_(c)
    else:
        dist.broadcast(t, src=src, group=group)
    return t


def all_gather_rows(t, world, group=None):
    """[world, *t.shape]: every rank's t."""
    out = torch.empty(world * t.numel(), dtype=t.dtype, device="cpu" if _staged(t, group) else t.device)
    dist.all_gather_into_tensor(out, (t.cpu() if _staged(t, group) else t).reshape(-1).contiguous(), group=group)
    return out.to(t.device).view((world,) + tuple(t.shape))


class HaloExchange:
    """h[n_own:] <- owners' rows, via one packed all_to_all_single (RCCL on GPUs, gloo in the CPU tests)."""

    def __init__(self, part, ops, group=None):
        self.part, self.ops, self.group, self.work, self._keep, self._bwd = part, ops, group, None, None, None
        self._into = None   # the strided halo rows a dense receive buffer is copied into by finish() (see start)

    def start(self, h):
        p = self.part
        if _alone(p.world):
            return
        packed = self.ops.gather_rows(h, p.send_idx)
        into, self._into = h[p.n_own:], None
        if not into.is_contiguous():
            # a column block of a wider table (SAGEModel's h | m, dT): all_to_all_single writes dense memory only, so the rows are received
            # into a dense [halo, H] buffer and finish() copies them in - one more [halo, H] read + write per such exchange
            self._into, into = into, torch.empty(into.shape, dtype=h.dtype, device=h.device)
        self._keep = (packed, into)   # (both stay alive until the collective is done)
        self.work = all_to_all_rows(into, packed, p.recv_counts, p.send_counts, self.group, async_op=True)

    def finish(self):
        if self.work is not None:
            self.work.wait()
        if self._into is not None:
            self._into.copy_(self._keep[1])
        self.work, self._keep, self._into = None, None, None

    def transpose(self, dh):
        """Backward of start/finish: the halo rows of dh return to their owners, which add them to their own rows
        (one peer's block at a time: within a block the rows are distinct, so the sum order is fixed), then
        dh[n_own:] = 0."""
        self.transpose_start(dh)
        self.transpose_finish(dh)

    def transpose_start(self, dh):
        """First half of `transpose`: the halo rows leave (RCCL: asynchronously, on the collective's stream).  Nothing may WRITE dh until
        transpose_finish; kernels that do not touch dh - the layer's weight gradients - run underneath."""
        p = self.part
        if _alone(p.world):
            return
        got = torch.empty((int(p.send_idx.numel()), dh.shape[1]), dtype=torch.float32, device=dh.device)
        sent = dh[p.n_own:].contiguous()   # (a view: dh is contiguous)
        work = all_to_all_rows(got, sent, p.send_counts, p.recv_counts, self.group, async_op=True)
        self._bwd = (work, got, sent)

    def transpose_finish(self, dh):
        p = self.part
        if _alone(p.world) or getattr(self, "_bwd", None) is None:
            return
        work, got, _ = self._bwd
        self._bwd = None
        if work is not None:
            work.wait()
        at = 0
        for cnt in p.send_counts:
            if cnt:
                self.ops.scatter_add_rows(got[at:at + cnt], p.send_idx[at:at + cnt], dh)
            at += cnt
        dh[p.n_own:].zero_()


def check_forward_plan(part):
    """The PLAN is always the forward orientation's; the reversed pass of SymGatedGCNModel is asked for with reverse=True on that plan."""
    if part.views.transposed:
        raise NotImplementedError("partitioned training runs on the forward orientation of the graph")


def check_shard(part):
    """What a PartitionShard refuses; every runner and engine_baselines / engine_gat.check_partition raise the same through here, before
    they allocate anything."""
    check_forward_plan(part)
    if part.n_own == 0 or part.n_score == 0:
        raise NotImplementedError("a rank without owned nodes or owned in-edges (graph too small for this world size)")


class PartitionShard:
    """One rank's rows of a training step over a destination-range partition (see gnnome_amd.train.WholeGraph for
    the interface; SURVEY.md 8e "Training additions"):
      * BatchNorm batch statistics: every rank reduces its OWNED rows (each edge / node of the graph exactly once),
        the per-rank (count, mean, M2) are all-gathered and merged with the parallel-variance formula;
      * backward: per-channel BatchNorm sums and, at the end, all parameter gradients are all-reduced (one flat
        buffer); halo rows of dh are scatter-added back to their owners once per layer."""

    def __init__(self, part, ops=hip_ops, group=None, reverse=False):
        """reverse: the shard of the pass over dgl.reverse(g) (gated_gcn_full.py:99,117-127; train.py:165) - SymGatedGCNModel's step only.
        The rows a rank owns do not depend on the orientation: the same owned nodes, the same n_score scored edges (the sorted prefix,
        whose FORWARD destination is owned), the same halo plan, the same assembly of the logits.  Only `views` changes - the plan's own
        arrays with the flag flipped (GraphViews.reversed: nothing is sorted or copied) - and with it the roles train._roles deals out."""
        check_shard(part)
        self.part, self.ops, self.group, self.world = part, ops, group, part.world
        self.alone = _alone(part.world)     # False under GNNOME_FORCE_COLLECTIVES=1: one rank, every collective issued
        self.reverse = bool(reverse)
        self.views = part.views.reversed() if self.reverse else part.views
        self.n_own, self.n_local = part.n_own, part.n_local
        self.e_own, self.e_local = part.n_score, part.views.num_edges
        self.n_global, self.e_global = part.bounds[-1], part.num_edges_global
        # what the scorer reads (part.scored): every owned in-edge as it lies, its node gathers transposed over the local lists - or, on a
        # doubled plan, the score_rows alone (e_scored of them, possibly none) under the views of those edges; e_own / e_global stay the
        # DOUBLED counts, the rows bn_e's statistics run over
        sc = part.scored
        self.score_views, self.score_rows, self.e_scored = sc.score_views, sc.rows, sc.count
        self.seg_views = sc.views.reversed() if self.reverse else sc.views
        self.logits_finish = part.logits_finish(group)   # engine.score_tail's ending: {} when alone
        self._xchg = HaloExchange(part, ops, group)

    def halo_start(self, h):
        self._xchg.start(h)

    def halo_finish(self):
        self._xchg.finish()

    def halo_bwd(self, dh):
        self._xchg.transpose(dh)

    def halo_bwd_start(self, dh):
        self._xchg.transpose_start(dh)

    def halo_bwd_finish(self, dh):
        self._xchg.transpose_finish(dh)

    def combine_stats(self, mean, var, rows):
        if self.alone:
            return mean, var
        H = mean.numel()
        mine = torch.cat([torch.full((1,), float(rows), dtype=torch.float64, device=mean.device), mean.double(), var.double() * rows])
        every = all_gather_rows(mine, self.world, self.group)           # [world, 1+2H], identical on every rank
        n, mu, m2 = every[:, :1], every[:, 1:1 + H], every[:, 1 + H:]
        total = n.sum()
        mean_all = (n * mu).sum(0) / total
        m2_all = (m2 + n * (mu - mean_all) ** 2).sum(0)
        return mean_all.float().contiguous(), (m2_all / total).float().contiguous()

    def sync_moments(self, moments):
        """(d1, d2, center, rows) of a single-rank BatchNorm call (train._bn_train_fused; train._can_fuse_bn admits world == 1 only) through
        the statistics' all_gather: one rank's own row comes back, the same bits, and the collective has been issued."""
        if self.alone:
            return moments
        d1, d2, center, rows = moments
        H = d1.numel()
        row = all_gather_rows(torch.cat([d1.reshape(-1), d2.reshape(-1), center.reshape(-1)]), self.world, self.group)[0]
        return row[:H], row[H:2 * H], row[2 * H:], rows

    def sum_ranks(self, tensors):
        if self.alone:
            return tensors
        flat = torch.cat([t.reshape(-1) for t in tensors])
        all_reduce_sum(flat, self.group)
        out, at = [], 0
        for t in tensors:
            out.append(flat[at:at + t.numel()].view(t.shape))
            at += t.numel()
        return out



def check_doubled(gated, directed, part, what):
    """Model and plan must agree on the doubled edge list of full_graph.py:47-51: GatedGCNModel(directed=False) runs on a doubled plan and
    nothing else does.  Raised before anything is allocated or exchanged; `what` names a model that is no GatedGCNModel."""
    doubled = bool(getattr(part, "doubled", False))
    if gated and not directed and not doubled:
        raise NotImplementedError("GatedGCNModel with directed=False runs on a partition of the doubled edge list, and this plan is not one: "
                                  "build it with PartitionedGraph.from_global(src, dst, ..., in_edges_only=True, doubled=True) over the "
                                  "original edges")
    if doubled and not gated:
        raise ValueError(f"a doubled plan (doubled=True) serves GatedGCNModel with directed=False only; got {what}")
    if doubled and directed:
        raise ValueError("a doubled plan (doubled=True) serves GatedGCNModel with directed=False only; this model has directed=True and "
                         "would run the stack on edges it does not have: build the plan with doubled=False")


def _check_partition_kind(prep, part):
    """True for a GatedGCNModel's weights.  The one-direction model runs on the in-edge-only partition - the doubled one with
    directed=False - the symmetric model on the one that also keeps the out-edges of the owned nodes: any other combination would silently
    drop or double terms, so it raises."""
    gated = isinstance(prep, engine_gated.Prepared)
    check_doubled(gated, not gated or prep.directed, part, "a SymGatedGCNModel")
    if gated != bool(getattr(part, "in_edges_only", False)):
        raise ValueError("GatedGCNModel runs on PartitionedGraph.from_global(..., in_edges_only=True), SymGatedGCNModel on the default "
                         f"partition; got in_edges_only={getattr(part, 'in_edges_only', False)}")
    return gated


def run_partitioned(ops, prep, part, x_local, e_local, group=None, reverse=False):
    """The rank-local kernel sequence.  x_local: [n_local, F] features of owned+halo nodes, e_local:
    [e_local, F] features of local edges in local edge-id order.  Returns logits[E_global], complete on every rank.
    reverse (SymGatedGCNModel only): the pass over dgl.reverse(g) (gated_gcn_full.py:99,117-127; train.py:165) on the SAME plan - x_local
    then holds the swapped degree columns.  Owned nodes, scored edges (the sorted prefix), halo exchange and the assembly of the logits are
    the forward pass's; the column blocks of P change roles (A2 <-> A3, B1 <-> B2, as engine.layer_step does on a whole graph) and the
    scorer's node halves change places (engine.score_step).
    prep = engine_gated.Prepared (a GatedGCNModel): engine_gated's eval sequence per layer - the [n_local,4H] projection, the same gate,
    gnnome_node_aggregate_in_f32 over the owned rows - on an in-edge-only partition (PartitionedGraph.from_global(..., in_edges_only=True)).
    With directed=False the plan is the doubled one (doubled=True): the same sequence over the local rows of the doubled list, the scorer
    over part.score_rows alone, logits[E] at the ORIGINAL edge ids."""
    from . import engine_baselines
    if isinstance(prep, engine_baselines.Prepared):   # GCNModel / SAGEModel: engine_baselines' sequence on the default partition
        if reverse:
            raise NotImplementedError("GCNModel / SAGEModel on a partition runs on the forward orientation of the graph")
        return engine_baselines.run_partitioned(ops, prep, part, x_local, e_local, group)
    gated = _check_partition_kind(prep, part)
    if gated and reverse:
        raise NotImplementedError("GatedGCNModel on an in-edge-only partition runs on the forward orientation of the graph")
    check_forward_plan(part)   # (the plan itself is never flipped: reverse= selects the pass)
    views, n_own = (part.views.reversed() if reverse else part.views), part.n_own
    xchg = HaloExchange(part, ops, group)
    H = prep.hidden
    h = ops.encode(x_local, *prep.enc_node)  # halo rows of layer 0 come straight from the input features
    e = engine.encode_edges(ops, prep, views, e_local)   # None: layer 0's gate encodes the edge tile itself
    scratch = {}
    for li, lw in enumerate(prep.layers):
        if li > 0:
            xchg.start(h)
        P = engine.project_rows(functools.partial(engine.project, ops, lw), h, n_own, xchg.finish, lw.Wcat.shape[0])
        if gated:   # A1h|A2h|B1h|B2h: no A_3 block, no out-edge half (the halo rows of h' are written by the next exchange)
            A1, A2, B1, B2 = (P[:, i * H:(i + 1) * H] for i in range(4))
            e = engine.gate(ops, lw, views, e, B1, B2, (e_local, prep.enc_edge), scratch)
            h = ops.node_aggregate_in(e, A1, A2, views, h, lw.norm, lw.scale_h, lw.shift_h, num_nodes_out=n_own)
            continue
        A1, A2, A3, B1, B2 = (P[:, i * H:(i + 1) * H] for i in range(5))
        if reverse:   # src <-> dst: an owned node's contiguous by-dst run holds its OUT-edges now, its out_pos run its in-edges
            A2, A3, B1, B2 = A3, A2, B2, B1
        e = engine.gate(ops, lw, views, e, B1, B2, (e_local, prep.enc_edge), scratch)
        h = ops.node_aggregate(e, A1, A2, A3, views, h, lw.norm, lw.scale_h, lw.shift_h, num_nodes_out=n_own)
    xchg.start(h)
    pw = prep.predictor
    hs = pw["hs"]
    xchg.finish()
    PQ = ops.linear(h, pw["W_nodes"], pw["b_nodes"], planes=pw.get("planes"))
    Ps, Qd = (PQ[:, hs:], PQ[:, :hs]) if reverse else (PQ[:, :hs], PQ[:, hs:])   # x[src'] | x[dst'] = x[dst] | x[src]; b1 enters once either way
    # what is scored here: the owned in-edges as they lie - or, on a doubled plan, the ORIGINAL graph (full_graph.py:51): the rows of the
    # prefix with ids below E, gathered as run_stack gathers score_gather; a rank whose in-edges are all reverse copies scores nothing
    sc = part.scored
    return engine.score_tail(ops, engine.scored_rows(ops, e, sc.rows, sc.count), Ps, Qd, engine.tail_weights(pw), sc.score_views,
                             sc.count, sc.total, **part.logits_finish(group))


class CapturedPartitionedForward:
    """run_partitioned with every stretch of kernels BETWEEN two collectives recorded once as a hipGraph: one forward is then
    L + 1 graph replays + L halo exchanges + the logits all-gather instead of ~55 Python-issued launches - what a rank needs
    when its share of the graph is small enough for the host to become the limit (eight ranks on the 10M-edge graph: ~6 ms
    of kernels per rank).  The collectives themselves stay OUTSIDE the graphs (RCCL / gloo calls between replays, ordered on
    the stream), so nothing depends on capturing a communicator; the price is that the exchange no longer overlaps the
    projection of the owned rows (the halo rows of a layout-ordered graph are a few per cent of a rank's rows).
    Same kernels, same order: the logits equal run_partitioned's bit for bit.  Inputs are the runner's static x / e."""

    def __init__(self, runner, reverse=False):
        if reverse:   # (before anything is allocated or warmed up)
            raise NotImplementedError("CapturedPartitionedForward records the forward orientation only; the reversed pass (reverse=True) runs "
                                      "the eager PartitionedRunner.forward(reverse=True)")
        if runner.prep is None:
            raise RuntimeError("CapturedPartitionedForward is for eval-mode inference")
        ops, prep, part = runner.ops, runner.prep, runner.part
        if isinstance(prep, engine_gated.Prepared):
            raise NotImplementedError("CapturedPartitionedForward is built for SymGatedGCNModel; a GatedGCNModel runs the eager forward()")
        if not isinstance(prep, engine.Prepared):
            raise NotImplementedError("CapturedPartitionedForward is built for SymGatedGCNModel; a GCNModel / SAGEModel runs the eager forward()")
        self.part, self.group, self.ops = part, runner.group, ops
        self.alone = alone = _alone(part.world)
        dev = runner.x.device
        with torch.no_grad():
            for _ in range(2):   # eager warm-up: weight preparation, allocator pools, the aggregation's hub scratch
                run_partitioned(ops, prep, part, runner.x, runner.e, runner.group)
        torch.cuda.synchronize(dev)
        views, n_own, H = part.views, part.n_own, prep.hidden
        pool = torch.cuda.graph_pool_handle()
        self.graphs, self.h, self.packed = [], [], []
        state = {"h": None, "e": None, "scratch": {}}

        def layer(li):
            lw = prep.layers[li]
            if li == 0:
                state["h"] = ops.encode(runner.x, *prep.enc_node)
                state["e"] = engine.encode_edges(ops, prep, views, runner.e)
            h = state["h"]
            P = engine.project(ops, lw, h)
            A1, A2, A3, B1, B2 = (P[:, i * H:(i + 1) * H] for i in range(5))
            state["e"] = engine.gate(ops, lw, views, state["e"], B1, B2, (runner.e, prep.enc_edge), state["scratch"])
            state["h"] = ops.node_aggregate(state["e"], A1, A2, A3, views, h, lw.norm, lw.scale_h, lw.shift_h, num_nodes_out=n_own)
            self.h.append(state["h"])
            self.packed.append(None if alone else ops.gather_rows(state["h"], part.send_idx))

        def score():
            pw = prep.predictor
            hs = pw["hs"]
            PQ = ops.linear(state["h"], pw["W_nodes"], pw["b_nodes"], planes=pw.get("planes"))
            # the complete logits when alone; otherwise this rank's piece as it is: every replay assembles it (__call__), no collective is recorded
            sc = part.scored
            finish = {} if alone else dict(pad=part.score_pad, assemble=lambda piece: piece)
            self.piece = engine.score_tail(ops, engine.scored_rows(ops, state["e"], sc.rows, sc.count), PQ[:, :hs], PQ[:, hs:],
                                           engine.tail_weights(pw), sc.score_views, sc.count, sc.total, **finish)

        with torch.no_grad():
            for fn in [lambda li=li: layer(li) for li in range(len(prep.layers))] + [score]:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool):
                    fn()
                self.graphs.append(g)
        self._keep = state   # the recorded kernels read and write these tensors at their recorded addresses

    def __call__(self):
        p = self.part
        for i, g in enumerate(self.graphs):
            g.replay()
            if i < len(self.h) and not self.alone:
                all_to_all_rows(self.h[i][p.n_own:], self.packed[i], p.recv_counts, p.send_counts, self.group)
        return (self.piece if self.alone else p.assemble_logits(self.piece, self.group)).unsqueeze(1)


class _ScoreViews:
    """The scorer only reads srt_src / srt_dst / srt_eid."""

    def __init__(self, views, srt_geid):
        self.srt_src, self.srt_dst, self.srt_eid = views.srt_src, views.srt_dst, srt_geid


def _local_rows(select, whole, local, device):
    """A runner's input on its device: select(whole) - this rank's rows of the whole graph's table - or `local`, those rows already selected."""
    rows = select(whole) if local is None else local
    return rows.to(device=device, dtype=torch.float32).contiguous()


class PartitionedRunner:
    """Holds one rank's partition, weights and inputs on its GPU; forward() = one whole-graph scoring pass."""

    def __init__(self, model, part, x_global, e_global, device, ops=hip_ops, group=None, x_local=None, e_local=None, split=None,
                 x_rev_global=None, x_rev_local=None):
        """x_global[N,F]: the node features of the whole graph (this rank keeps its owned + halo rows), or x_local: those rows
        already selected (part.local_node_rows), for callers that never hold the [N,F] table on this device; e_global[E,F] or
        e_local (part.local_edge_rows / part.shuffle_edge_rows) likewise.
        split (GCNModel / SAGEModel only): True = the neighbour sums as interior rows under the halo exchange + boundary rows after it,
        False = one launch after it, None = engine_baselines.PARTITION_SPLIT; equal bits either way.
        x_rev_global / x_rev_local (SymGatedGCNModel only): the node features of the REVERSED pass - the degree columns swapped
        (train.py:165-166; part.local_degree_features(reverse=True)) - which forward(reverse=True) / train_forward(reverse=True) read.  One
        plan, one set of views, one copy of the edge features serve both passes."""
        self.ops, self.part, self.group, self.model = ops, part, group, model
        from . import engine_baselines
        from .models import GatedGCNModel
        kind = getattr(model, "kind", None)             # GCNModel "gcn", SAGEModel "sage", GATModel "gat" (engine_baselines.py, engine_gat.py)
        self.baseline = kind in engine_baselines.KINDS
        self.gated = isinstance(model, GatedGCNModel)   # (engine_gated.py): the in-edge-only partition, its own kernel sequences
        if not self.gated:
            check_doubled(False, True, part, f"a {type(model).__name__}")
        if kind == "gat":
            raise NotImplementedError("GATModel is not served on partitions by PartitionedRunner: its backward makes a second exchange per "
                                      "layer and it takes no split= - use dist.GATPartitionedRunner (same inputs, same forward() / "
                                      "train_forward())")
        if split is not None and not self.baseline:
            raise ValueError("split= selects the launch form of GCNModel / SAGEModel's neighbour sums; the gated models have none")
        self.split = split
        if self.baseline:
            engine_baselines.check_partition(model, part)
        elif self.gated:
            check_doubled(True, bool(model.directed), part, None)
            if not part.in_edges_only:
                raise ValueError("GatedGCNModel runs on an in-edge-only partition: PartitionedGraph.from_global(..., in_edges_only=True)")
        elif part.in_edges_only:
            raise ValueError("an in-edge-only partition serves GatedGCNModel; SymGatedGCNModel needs the out-edges of the owned nodes too")
        else:   # the reversed pass is selected by reverse=, never by flipping the plan
            check_forward_plan(part)
        if (x_rev_global is not None or x_rev_local is not None) and (self.baseline or self.gated):
            raise NotImplementedError(f"{type(model).__name__} on a partition runs on the forward orientation of the graph: it takes no x_rev")
        prepared = engine_baselines.Prepared if self.baseline else engine_gated.Prepared if self.gated else engine.Prepared
        self.prep = None if model.training else engine.prepared_for(model, device, prepared)
        self.x = _local_rows(part.local_node_rows, x_global, x_local, device)
        self.e = _local_rows(part.local_edge_rows, e_global, e_local, device)
        self.x_rev = None
        if x_rev_global is not None or x_rev_local is not None:
            self.x_rev = _local_rows(part.local_node_rows, x_rev_global, x_rev_local, device)

    def capture(self, reverse=False):
        """Record the forward as hipGraph segments between the collectives (CapturedPartitionedForward); forward() replays them.
        reverse=True is refused there: the reversed pass stays eager."""
        self._captured = CapturedPartitionedForward(self, reverse=reverse)
        return self

    def _reversed_inputs(self):
        """x of the reversed pass, or the refusal of a model / runner that has none."""
        if self.baseline or self.gated:
            raise NotImplementedError(f"{type(self.model).__name__} on a partition runs on the forward orientation of the graph")
        if self.x_rev is None:
            raise ValueError("reverse=True reads the node features of the reversed pass: build the runner with x_rev_global= or x_rev_local=")
        return self.x_rev

    def forward(self, reverse=False):
        """eval mode: logits[E,1] of one whole-graph scoring pass.  reverse=True (SymGatedGCNModel): the pass over dgl.reverse(g) on the
        runner's x_rev - the `rev` logits of train.py:165-167, [E,1] in edge-id order, identical on every rank; always eager."""
        if self.prep is None:
            raise RuntimeError("built from a model in train mode: use train_forward()")
        if reverse:
            x_rev = self._reversed_inputs()
            with torch.no_grad():
                return run_partitioned(self.ops, self.prep, self.part, x_rev, self.e, self.group, reverse=True).unsqueeze(1)
        if getattr(self, "_captured", None) is not None:
            return self._captured()
        with torch.no_grad():
            if self.baseline:
                from . import engine_baselines
                run = functools.partial(engine_baselines.run_partitioned, split=self.split)
                return engine_baselines.forward_partitioned(self.ops, self.model, self.prep, self.part, self.x, self.e, self.group, run).unsqueeze(1)
            return run_partitioned(self.ops, self.prep, self.part, self.x, self.e, self.group).unsqueeze(1)

    def check_train_step(self):
        """What train_forward() refuses about the MODEL, raised without running a kernel or a collective (trainer.train_partitioned asks
        before epoch 0): the symmetric-step adapter of GatedGCNModel (zero A_3) is not served on partitions."""
        if self.gated and engine_gated.training_step_of(self.model) != "in_edge":
            raise NotImplementedError('a partitioned GatedGCNModel trains with training_step = "in_edge"; this model has training_step = '
                                      f'{self.model.training_step!r}')

    def train_forward(self, reverse=False):
        """train mode: logits[E,1] with autograd history; after loss.backward() every rank holds the whole graph's
        parameter gradients (already summed over ranks), so identical optimizers stay in step without a DDP wrapper.
        reverse=True (SymGatedGCNModel): the `rev` logits.  One symmetry step (train.py:159-170) is
            loss.symmetry_loss(r.train_forward().squeeze(-1), r.train_forward(reverse=True).squeeze(-1), y, pw, alpha).backward()
        - two autograd nodes, each with its own shard and its own saved activations, both alive until backward(); the gradients of the two
        passes are all-reduced per pass and accumulate in .grad, bn_e's running statistics advance four times per layer, bn_h's twice.
        Every rank must call the two passes, and backward(), in the same order: each issues collectives."""
        from .train import train_forward_on
        if reverse:
            x_rev = self._reversed_inputs()
            return train_forward_on(self.model, PartitionShard(self.part, self.ops, self.group, reverse=True), x_rev, self.e)
        if self.baseline:   # GCNModel / SAGEModel: engine_baselines' step on the shard (one exchange of h and one of its gradient per layer)
            from . import engine_baselines
            return engine_baselines.train_forward_on(self.model, PartitionShard(self.part, self.ops, self.group), self.x, self.e,
                                                     split=self.split)
        if self.gated:
            self.check_train_step()
            return engine_gated.train_forward_in_edge_on(self.model, PartitionShard(self.part, self.ops, self.group), self.x, self.e)
        return train_forward_on(self.model, PartitionShard(self.part, self.ops, self.group), self.x, self.e)


class GATPartitionedRunner:
    """PartitionedRunner for GATModel: one rank's default partition, weights and inputs on its GPU; the same inputs, the same forward()
    and train_forward().  A class of its own because the sequence is: no split= (the interior / boundary launch was never measured to
    pay), two exchanges per layer in the backward, the halo rows of the projection made locally (engine_gat.py, "destination-range
    partitions").  directed=False is served: the partition keeps both lists of every owned node and the kernels take `both`."""

    def __init__(self, model, part, x_global, e_global, device, ops=hip_ops, group=None, x_local=None, e_local=None):
        """x_global / e_global, or x_local / e_local already selected: as for PartitionedRunner.  Every refusal is raised before anything
        is allocated on the device."""
        from . import engine_gat
        check_doubled(False, True, part, f"a {type(model).__name__}")
        engine_gat.check_partition(model, part)
        self.ops, self.part, self.group, self.model = ops, part, group, model
        self.prep = None if model.training else engine.prepared_for(model, device, engine_gat.Prepared)
        self.x = _local_rows(part.local_node_rows, x_global, x_local, device)
        self.e = _local_rows(part.local_edge_rows, e_global, e_local, device)

    def capture(self):
        raise NotImplementedError("CapturedPartitionedForward is built for SymGatedGCNModel; a GATModel runs the eager forward()")

    def check_train_step(self):
        """PartitionedRunner.check_train_step: GATModel has one training step, and check_partition has passed."""

    def forward(self):
        """eval mode: logits[E,1] of one whole-graph scoring pass, complete on every rank."""
        from . import engine_baselines, engine_gat
        if self.prep is None:
            raise RuntimeError("built from a model in train mode: use train_forward()")
        with torch.no_grad():
            return engine_baselines.forward_partitioned(self.ops, self.model, self.prep, self.part, self.x, self.e, self.group,
                                                        engine_gat.run_partitioned).unsqueeze(1)

    def train_forward(self):
        """train mode: logits[E,1] with autograd history; after loss.backward() every rank holds the whole graph's parameter gradients
        (already summed over ranks)."""
        from . import engine_gat
        return engine_gat.train_forward_on(self.model, PartitionShard(self.part, self.ops, self.group), self.x, self.e)
