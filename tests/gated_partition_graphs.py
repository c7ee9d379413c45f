"""Synthetic graphs for the partitioned GatedGCNModel tests (test_dist_gated_gloo.py, test_hip_gated_partition.py), each with the range
boundaries it is cut at.  Between them they hold what an in-edge-only destination-range partition can get wrong:

  mixed  (60 nodes, bounds uneven)   edges between every ordered pair of ranks, a node with in-degree 0, an owned node all of whose
                                     sources are remote, a triple parallel edge, a self-loop, a destination with 70 in-edges (more
                                     than one 64-item batch) fed from every rank
  island (48 nodes)                  rank 0's nodes are fed from rank 0 alone: its halo is EMPTY (and it still sends rows)
  star   (4200 nodes)                one node with an in-edge from every other node - 4199 > 4096 items, the two-level path - whose
                                     sources lie on every rank, so its in-list crosses the halo; a light random background
"""
import torch

HIDDEN, LAYERS, SCORE_HIDDEN = 64, 2, 32


def _finish(name, src, dst, n, bounds, seed):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.tensor(src, dtype=torch.int64), torch.tensor(dst, dtype=torch.int64)
    perm = torch.randperm(src.numel(), generator=g)        # edge ids carry no order
    src, dst = src[perm], dst[perm]
    E = src.numel()
    x = torch.stack([torch.log1p(torch.bincount(dst, minlength=n).float()), torch.log1p(torch.bincount(src, minlength=n).float())], 1)
    e = torch.stack([torch.randn(E, generator=g), 0.9 + 0.1 * torch.rand(E, generator=g)], 1)
    y = (torch.rand(E, generator=g) < 0.6).float()
    return dict(name=name, src=src.int(), dst=dst.int(), num_nodes=n, x=x, e=e, y=y, pos_weight=torch.tensor(1.5), bounds=bounds)


def mixed():
    n, bounds = 60, {2: [0, 25, 60], 3: [0, 14, 37, 60]}
    g = torch.Generator().manual_seed(11)
    src = torch.randint(0, n - 1, (360,), generator=g).tolist()     # (node 59 is fed below)
    dst = torch.randint(0, n - 1, (360,), generator=g).tolist()     # node 59: in-degree 0
    keep = [(s, d) for s, d in zip(src, dst) if d != 3]               # node 3 (rank 0 at both world sizes) is fed from outside its range only
    keep += [(30, 3), (45, 3), (58, 3)]
    keep += [(20, 5)] * 3                                             # parallel edges, cut at world 3
    keep += [(16, 16)]                                                # a self-loop
    keep += [(int(s), 40) for s in torch.randint(0, n, (70,), generator=g)]   # 70 in-edges from every rank
    for a in (2, 20, 50):                                             # every ordered pair of ranks, whatever the random part gave
        for b in (4, 22, 52):
            keep.append((a, b))
    keep.append((59, 0))
    return _finish("mixed", [s for s, _ in keep], [d for _, d in keep], n, bounds, seed=1)


def island():
    n, bounds = 48, {2: [0, 16, 48], 3: [0, 16, 30, 48]}
    g = torch.Generator().manual_seed(12)
    src = torch.randint(0, 16, (80,), generator=g).tolist() + torch.randint(0, n, (220,), generator=g).tolist()
    dst = torch.randint(0, 16, (80,), generator=g).tolist() + torch.randint(16, n, (220,), generator=g).tolist()
    return _finish("island", src, dst, n, bounds, seed=2)


def star():
    n, hub, bounds = 4200, 2100, {2: [0, 2000, 4200], 3: [0, 1500, 2600, 4200]}
    g = torch.Generator().manual_seed(13)
    src = [s for s in range(n) if s != hub] + torch.randint(0, n, (2 * n,), generator=g).tolist()
    dst = [hub] * (n - 1) + torch.randint(0, n, (2 * n,), generator=g).tolist()
    return _finish("star", src, dst, n, bounds, seed=3)


GRAPHS = {"mixed": mixed, "island": island, "star": star}


def properties(gr, world):
    """What the module docstring promises, measured on the graph: used by the tests to assert that the cases are what they claim."""
    src, dst, n = gr["src"].long(), gr["dst"].long(), gr["num_nodes"]
    bt = torch.tensor(gr["bounds"][world][1:-1])
    rs, rd = torch.bucketize(src, bt, right=True), torch.bucketize(dst, bt, right=True)
    indeg = torch.bincount(dst, minlength=n)
    remote_only = torch.ones(n, dtype=torch.bool)
    remote_only[dst[rs == rd]] = False
    key = src * n + dst
    halo = [int(torch.unique(src[(rd == p) & (rs != p)]).numel()) for p in range(world)]
    return dict(zero_in_degree=int((indeg == 0).sum()), all_sources_remote=int((remote_only & (indeg > 0)).sum()),
                parallel=int(key.numel() - torch.unique(key).numel()), self_loops=int((src == dst).sum()),
                rank_pairs=int(torch.unique(rs * world + rd).numel()), max_in_degree=int(indeg.max()), halo_rows=halo)


def shard_of(gr, world, rank):
    """Rank `rank`'s local graph of the in-edge-only partition, restated without a process group (what PartitionedGraph.from_global(...,
    in_edges_only=True) builds): edge_gid (the owned in-edges, ascending global id), node_gid (owned nodes, then the distinct non-owned
    sources ascending), the local endpoints, n_own."""
    src, dst = gr["src"].long(), gr["dst"].long()
    lo, hi = gr["bounds"][world][rank], gr["bounds"][world][rank + 1]
    edge_gid = torch.nonzero((dst >= lo) & (dst < hi)).squeeze(1)
    ls, ld = src[edge_gid], dst[edge_gid]
    halo = torch.unique(ls[(ls < lo) | (ls >= hi)])
    node_gid = torch.cat([torch.arange(lo, hi), halo])
    local_of = torch.full((gr["num_nodes"],), -1, dtype=torch.int64)
    local_of[node_gid] = torch.arange(node_gid.numel())
    return dict(edge_gid=edge_gid, node_gid=node_gid, src=local_of[ls].int(), dst=local_of[ld].int(), n_own=hi - lo, lo=lo, hi=hi)
