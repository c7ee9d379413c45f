"""Helpers of the partitioned GCNModel / SAGEModel tests (test_dist_baseline_gloo.py, test_hip_baseline_partition.py): the graphs of
tests/gated_partition_graphs.py, one hub graph of this module's, the FULL shard of a rank restated without a process group, models."""
import torch

import baseline_graphs as bg
import gated_partition_graphs as gpg
from gated_partition_graphs import GRAPHS, HIDDEN, LAYERS, SCORE_HIDDEN  # noqa: F401

KINDS = ("gcn", "sage")


def hub_on_the_boundary():
    """A few thousand edges: node 2500 - the FIRST node of rank 1's range at world 2 - has 4200 in-edges and 4150 out-edges, both lists above
    the 4096-item threshold and both crossing the range boundary, so the fixed 128-item blocks run in the part entries over owned and halo
    rows; a light random background so that the other rows have lists too."""
    n, hub = 5000, 2500
    g = torch.Generator().manual_seed(17)
    others = [v for v in range(n) if v != hub]
    src = others[:4200] + [hub] * 4150 + torch.randint(0, n, (1500,), generator=g).tolist()
    dst = [hub] * 4200 + others[-4150:] + torch.randint(0, n, (1500,), generator=g).tolist()
    return gpg._finish("hub", src, dst, n, {2: [0, 2500, 5000]}, seed=4)


def full_shard_of(gr, world, rank):
    """Rank `rank`'s local graph of the DEFAULT partition (what PartitionedGraph.from_global builds): the owned nodes, every edge with an
    owned end in ascending global id, halo = the other ends ascending; -> edge_gid, node_gid, local endpoints, n_own, lo, hi."""
    src, dst = gr["src"].long(), gr["dst"].long()
    lo, hi = gr["bounds"][world][rank], gr["bounds"][world][rank + 1]
    edge_gid = torch.nonzero(((dst >= lo) & (dst < hi)) | ((src >= lo) & (src < hi))).squeeze(1)
    ls, ld = src[edge_gid], dst[edge_gid]
    ends = torch.cat([ls, ld])
    halo = torch.unique(ends[(ends < lo) | (ends >= hi)])
    node_gid = torch.cat([torch.arange(lo, hi), halo])
    local_of = torch.full((gr["num_nodes"],), -1, dtype=torch.int64)
    local_of[node_gid] = torch.arange(node_gid.numel())
    return dict(edge_gid=edge_gid, node_gid=node_gid, src=local_of[ls].int(), dst=local_of[ld].int(), n_own=hi - lo, lo=lo, hi=hi)


def whole_scales(gr, directed):
    """(din'^-1/2, dout'^-1/2, 1/din') of the whole graph, float32 - engine_baselines.Scales' formulas on bincount degrees."""
    n = gr["num_nodes"]
    din, dout = torch.bincount(gr["dst"].long(), minlength=n).float(), torch.bincount(gr["src"].long(), minlength=n).float()
    if directed:
        din, dout = din + 1.0, dout + 1.0
    else:
        din = dout = din + dout + 1.0
    return din.pow(-0.5), dout.pow(-0.5), 1.0 / din


def model(kind, directed=True, dropout=0.0, seed=8):
    from gnnome_amd.models import GCNModel, SAGEModel
    m = (GCNModel if kind == "gcn" else SAGEModel)(2, 2, HIDDEN, 16, LAYERS, SCORE_HIDDEN, "batch", dropout=dropout, directed=directed)
    m.load_state_dict(bg.random_state_dict(m, seed=seed))
    return m


def known_masks(gr, dropout, seed=5):
    """One scaled keep-mask [N, HIDDEN] per layer for the WHOLE graph; a rank's masks are its rows [lo, hi)."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(gr["num_nodes"], HIDDEN, generator=g) >= dropout).float() / (1.0 - dropout) for _ in range(LAYERS)]


class HandedMasks:
    """Stands in for train.dropout_mask: hands out the rows [lo, hi) of the known masks, one layer per call, again from the first
    after the last (a forward that is run again draws again)."""

    def __init__(self, masks, lo, hi):
        self.masks, self.lo, self.hi, self.calls = masks, lo, hi, 0

    def __call__(self, rows, cols, p, device):
        m = self.masks[self.calls % len(self.masks)][self.lo:self.hi]
        self.calls += 1
        assert m.shape == (rows, cols)
        return m.to(device).contiguous()
