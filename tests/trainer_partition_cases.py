"""The datasets and hyperparameters tests/test_dist_trainer_gloo.py and tests/test_hip_trainer_partition.py share: two training graphs and
one validation graph of gnnome_amd.synth (banded, 300-400 nodes, 2 000-3 000 edges), one of them with a hub in the middle of the node range
whose in-list and out-list both reach across every range boundary of a two- or three-way partition."""
import torch

from gnnome_amd.synth import make_graph

HP = {"dim_latent": 64, "num_gnn_layers": 2, "hidden_edge_scores": 32, "num_epochs": 2, "num_nodes_per_cluster": 1000}
HUB = 150


def with_hub(g, hub=HUB, seed=3):
    """`g` plus 43 out-edges and 43 in-edges of node `hub`, their far ends spread over the whole node range."""
    n = g["num_nodes"]
    gen = torch.Generator().manual_seed(seed)
    to, frm = torch.arange(0, n, 7, dtype=torch.int32), torch.arange(3, n, 7, dtype=torch.int32)
    k = to.numel() + frm.numel()
    src = torch.cat([g["src"], torch.full_like(to, hub), frm])
    dst = torch.cat([g["dst"], to, torch.full_like(frm, hub)])
    e = torch.cat([g["e"], torch.cat([torch.randn(k, 1, generator=gen), 0.9 + 0.1 * torch.rand(k, 1, generator=gen)], 1)])
    y = torch.cat([g["y"], (torch.rand(k, generator=gen) < 0.3).float()])
    return {"src": src, "dst": dst, "num_nodes": n, "e": e, "y": y}


def datasets():
    a = with_hub(make_graph(300, 2400, seed=11))
    b = make_graph(400, 3000, seed=12)
    v = make_graph(300, 2000, seed=13)
    strip = lambda g: {k: g[k] for k in ("src", "dst", "num_nodes", "e", "y")}  # noqa: E731
    return [strip(a), strip(b)], [strip(v)]


def tiny_graph():
    """Four nodes, every edge between nodes 0 and 1: whatever the boundaries, a rank of a three-way partition owns no node or no in-edge."""
    return {"src": torch.tensor([0, 1, 0, 1], dtype=torch.int32), "dst": torch.tensor([1, 0, 1, 0], dtype=torch.int32), "num_nodes": 4,
            "e": torch.tensor([[0.5, 0.9], [-0.5, 0.95], [1.0, 0.99], [-1.0, 0.92]]), "y": torch.tensor([1.0, 0.0, 1.0, 0.0])}


def two_node_graph():
    """One read, every edge 0 -> 1: the balanced cut of a two-way partition leaves rank 0 without a node."""
    return {"src": torch.zeros(4, dtype=torch.int32), "dst": torch.ones(4, dtype=torch.int32), "num_nodes": 2,
            "e": torch.tensor([[0.5, 0.9], [-0.5, 0.95], [1.0, 0.99], [-1.0, 0.92]]), "y": torch.tensor([1.0, 0.0, 1.0, 0.0])}
