"""Seeded graphs and inputs for the one-direction GatedGCN tests (tests/test_aggregate_in.py, test_gated_model.py, test_gated_training.py,
test_gated_host.py), and the plain-torch restatement of the model the tests compare with (written from the formulas of
layers/gated_gcn_full.py:182-230 and models/full_graph.py:42-53, not copied from them)."""
import numpy as np
import torch
import torch.nn.functional as F

HUB_THRESHOLD = 4096      # gnnome_amd/csrc/node_aggregate.hip: in + out items above which the symmetric kernel splits a node's list


def lane_groups(hidden):
    return 64 // (hidden // 4)


def in_degrees(hidden):
    """The in-list lengths the kernel's paths turn on: empty, short, the lane-group count G and its neighbours, the 64-item batch and its
    neighbours, two batches and one."""
    g = lane_groups(hidden)
    return sorted({0, 1, 2, g - 1, g, g + 1, 63, 64, 65, 129})


def degree_graph(hidden, halo=0, seed=3):
    """One node per length of in_degrees(hidden), fed from a pool of 48 low-degree nodes (drawn WITH replacement: parallel edges), plus
    a node with two self-loops among three other in-edges, a node whose only in-edge is a self-loop, a triplicate parallel edge, and
    `halo` extra nodes at the END of the numbering that only ever appear as sources (rows beyond num_nodes_out of a partition).
    -> dict(src, dst int32 in shuffled edge order, n, n_out, in_degree int64[n])."""
    rng = np.random.default_rng(seed + hidden)
    lens = in_degrees(hidden)
    n_pool = 48
    special = len(lens) + 3
    n_out = special + n_pool
    n = n_out + halo
    pool = np.arange(special, n_out)
    sources = np.concatenate([pool, np.arange(n_out, n)]) if halo else pool
    src, dst = [], []
    for node, d in enumerate(lens):
        src += rng.choice(sources, size=d, replace=True).tolist()
        dst += [node] * d
    a, b, c = len(lens), len(lens) + 1, len(lens) + 2
    src += [a, a] + rng.choice(sources, size=3).tolist()        # two self-loops among other edges
    dst += [a] * 5
    src += [b]                                                   # nothing but a self-loop
    dst += [b]
    src += [int(pool[0])] * 3                                    # a triplicate parallel edge
    dst += [c] * 3
    for v in pool:                                               # the pool nodes get a few in-edges of their own
        k = int(rng.integers(0, 4))
        src += rng.choice(sources, size=k, replace=True).tolist()
        dst += [int(v)] * k
    if halo:                                                     # every halo row is referenced at least once
        src += list(range(n_out, n))
        dst += rng.choice(pool, size=halo).tolist()
    order = rng.permutation(len(src))
    src, dst = np.asarray(src, dtype=np.int32)[order], np.asarray(dst, dtype=np.int32)[order]
    din = np.bincount(dst, minlength=n)
    assert (din + np.bincount(src, minlength=n)).max() <= HUB_THRESHOLD
    return dict(src=torch.from_numpy(src), dst=torch.from_numpy(dst), n=n, n_out=n_out, in_degree=torch.from_numpy(din))


def hub_graph(in_edges=5000, ordinary=200, seed=5):
    """A node (the last id) with `in_edges` in-edges among `ordinary` ordinary nodes of in-degree ~6."""
    rng = np.random.default_rng(seed)
    hub = ordinary
    src = rng.integers(0, ordinary, size=in_edges).tolist()
    dst = [hub] * in_edges
    for v in range(ordinary):
        k = int(rng.integers(3, 10))
        src += rng.integers(0, ordinary, size=k).tolist()
        dst += [v] * k
    order = rng.permutation(len(src))
    return dict(src=torch.from_numpy(np.asarray(src, dtype=np.int32)[order]), dst=torch.from_numpy(np.asarray(dst, dtype=np.int32)[order]),
                n=ordinary + 1, hub=hub)


def model_graph(n, e, seed):
    """A seeded graph of n nodes and e edges with every kind of node the model meets: random edges, a few parallel ones, a self-loop,
    a node without in-edges and one without out-edges.  -> (src, dst) int32, x[n,2] (in / out degree), e[e,2]."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(1, n, (e,), generator=g)          # node 0 has no out-edges
    dst = torch.randint(0, n - 1, (e,), generator=g)      # node n - 1 has no in-edges
    src[:3], dst[:3] = 5, 6                                # parallel edges
    src[3] = dst[3] = 7                                    # a self-loop
    x = torch.stack([torch.bincount(dst, minlength=n), torch.bincount(src, minlength=n)], 1).float()
    ef = torch.stack([torch.randn(e, generator=g), 0.9 + 0.1 * torch.rand(e, generator=g)], 1)
    return src.int(), dst.int(), x, ef


def doubled_edge_list(src, dst):
    """dgl.add_reverse_edges: src|dst -> dst|src, the reverse copy of edge k has id E + k."""
    return torch.cat([src, dst]), torch.cat([dst, src])


def random_gated_state_dict(model, seed):
    """A state dict for `model` with weights that keep every activation O(1) and BatchNorm buffers away from their initial values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(v.shape, generator=g)
        elif ".bn_" in k and k.endswith("weight"):
            sd[k] = 0.75 + 0.5 * torch.rand(v.shape, generator=g)
        elif v.dim() == 2:
            sd[k] = torch.randn(v.shape, generator=g) / (v.shape[1] ** 0.5)
        else:
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
    return sd


# ---------------------------------------------------------------------------------------------- the restatement

def _norm(sd, pfx, x, training, updates=None):
    w, b = sd[pfx + ".weight"], sd[pfx + ".bias"]
    if pfx + ".running_mean" not in sd:
        return F.layer_norm(x, (x.shape[1],), w, b, 1e-5)
    if training:
        return F.batch_norm(x, None, None, w, b, True, 0.1, 1e-5)
    return F.batch_norm(x, sd[pfx + ".running_mean"], sd[pfx + ".running_var"], w, b, False, 0.1, 1e-5)


def gated_layer(sd, pfx, src, dst, n, h, e, training=False):
    """h' = relu(norm_h(A1 h + sum_in sigma(e') A2 h[src] / (sum_in sigma(e') + 1e-6))) + h,  e' = relu(norm_e(B1 h[src] + B2 h[dst] + B3 e)) + e."""
    lin = lambda name, t: F.linear(t, sd[pfx + name + ".weight"], sd[pfx + name + ".bias"])  # noqa: E731
    e_new = torch.relu(_norm(sd, pfx + "bn_e", lin("B_1", h)[src] + lin("B_2", h)[dst] + lin("B_3", e), training)) + e
    sig = torch.sigmoid(e_new)
    num = torch.zeros_like(h).index_add(0, dst, sig * lin("A_2", h)[src])
    den = torch.zeros_like(h).index_add(0, dst, sig)
    h_new = torch.relu(_norm(sd, pfx + "bn_h", lin("A_1", h) + num / (den + 1e-6), training)) + h
    return h_new, e_new


def gated_model(sd, src, dst, n, x, e, num_layers, directed=True, training=False):
    """Logits [E,1] of the one-direction model from a state dict (a dict of tensors, or of Parameters for autograd)."""
    src, dst = src.long(), dst.long()
    enc = lambda p, t: F.linear(torch.relu(F.linear(t, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])), sd[p + ".linear2.weight"],  # noqa: E731
                                sd[p + ".linear2.bias"])
    h, ee = enc("node_encoder", x), enc("edge_encoder", e)
    E = src.numel()
    gs, gd = (src, dst) if directed else doubled_edge_list(src, dst)
    if not directed:
        ee = torch.cat([ee, ee], 0)
    for i in range(num_layers):
        h, ee = gated_layer(sd, f"gnn.convs.{i}.", gs, gd, n, h, ee, training)
    ee = ee[:E]
    z = torch.relu(F.linear(torch.cat([h[src], h[dst], ee], 1), sd["predictor.W1.weight"], sd["predictor.W1.bias"]))
    z = torch.relu(F.linear(z, sd["predictor.W2.weight"], sd["predictor.W2.bias"]))
    return F.linear(z, sd["predictor.W3.weight"], sd["predictor.W3.bias"])
