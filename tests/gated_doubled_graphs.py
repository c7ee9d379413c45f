"""The fixed graph of the doubled-plan tests (test_dist_gated_doubled_host.py, test_dist_gated_doubled_gloo.py,
test_dist_gated_doubled_gpu.py): GatedGCNModel(directed=False) on the in-edge-only partition of the doubled edge list.  48 nodes, about 160
edges, cut at [0, 20, 48] and [0, 18, 40, 48].  It holds what that plan can get wrong:

  * (5, 30) and its like: ends owned by different ranks at both world sizes, so the reverse copy lives on the other rank;
  * (7, 7): a self-loop - copies k and E + k are both in-edges of node 7 on one rank, and only k is scored;
  * (3, 25) twice: a parallel pair;
  * nodes 40..47: original in-degree 0, out-degree > 0 - in the doubled graph all their in-edges are reverse copies; at world 3 they are
    exactly rank 2's range, so that rank scores nothing (n_score_original == 0) and still owns in-edges.
"""
import torch

N, HIDDEN, LAYERS, SCORE_HIDDEN = 48, 64, 2, 64
BOUNDS = {1: [0, 48], 2: [0, 20, 48], 3: [0, 18, 40, 48]}
CROSS, LOOP, PARALLEL = (5, 30), (7, 7), (3, 25)


def graph():
    g = torch.Generator().manual_seed(31)
    src = torch.randint(0, N, (140,), generator=g).tolist()
    dst = torch.randint(0, 40, (140,), generator=g).tolist()           # nobody points at nodes 40..47
    pairs = list(zip(src, dst)) + [CROSS, LOOP, PARALLEL, PARALLEL]
    pairs += [(40 + i, 5 * i) for i in range(8)]                        # every one of them has an out-edge, into rank 0 and rank 1
    pairs += [(44, 19), (2, 39), (21, 1)]
    src, dst = torch.tensor([s for s, _ in pairs]), torch.tensor([d for _, d in pairs])
    perm = torch.randperm(src.numel(), generator=g)                     # edge ids carry no order
    src, dst = src[perm], dst[perm]
    E = src.numel()
    # x from the ORIGINAL graph's degrees: full_graph.py computes x before add_edges
    x = torch.stack([torch.log1p(torch.bincount(dst, minlength=N).float()), torch.log1p(torch.bincount(src, minlength=N).float())], 1)
    e = torch.stack([torch.randn(E, generator=g), 0.9 + 0.1 * torch.rand(E, generator=g)], 1)
    y = (torch.rand(E, generator=g) < 0.6).float()
    return dict(src=src.int(), dst=dst.int(), num_nodes=N, x=x, e=e, y=y, pos_weight=torch.tensor(1.5), bounds=BOUNDS)


def owner(node, world):
    return int(torch.bucketize(torch.tensor(node), torch.tensor(BOUNDS[world][1:-1]), right=True))


def properties(gr):
    """What the module docstring promises, measured on the graph."""
    src, dst = gr["src"].long(), gr["dst"].long()
    indeg, outdeg = torch.bincount(dst, minlength=N), torch.bincount(src, minlength=N)
    key = src * N + dst
    out = dict(edges=int(src.numel()), self_loops=int((src == dst).sum()), parallel=int(key.numel() - torch.unique(key).numel()),
               sources_only=int(((indeg == 0) & (outdeg > 0)).sum()))
    for world in (2, 3):
        bt = torch.tensor(BOUNDS[world][1:-1])
        rs, rd = torch.bucketize(src, bt, right=True), torch.bucketize(dst, bt, right=True)
        out[f"cut{world}"] = int((rs != rd).sum())
        out[f"scored{world}"] = torch.bincount(rd, minlength=world).tolist()                    # original edges per owner of dst
        out[f"in_edges{world}"] = (torch.bincount(rd, minlength=world) + torch.bincount(rs, minlength=world)).tolist()   # doubled list
    return out
