"""Helpers of the GCNModel / SAGEModel tests (tests/test_baseline_statement.py, test_neighbour_sum.py, test_baseline_models.py): a
plain-torch fp32 restatement of both models, an fp64 statement of the neighbour sum with its error bound, graphs and seeded state dicts.
Written from the formulas of DGL 0.8.1's GraphConv(norm='both') and SAGEConv('mean') on g' = add_self_loop(g) /
add_self_loop(add_reverse_edges(g)) (models/full_graph.py:65-75, :109-119; layers/processor.py:35-46, :73-84), not copied from them."""
import torch
import torch.nn.functional as F

from gated_graphs import degree_graph, hub_graph, in_degrees, model_graph  # noqa: F401  (the graphs of the in-edge aggregation's tests)

EPS32 = 2.0 ** -23


def random_state_dict(model, seed):
    """A state dict for `model` (anything with state_dict()) with weights that keep every activation O(1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if v.dim() == 2:
            sd[k] = torch.randn(v.shape, generator=g) / (v.shape[1] ** 0.5)
        else:
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
    return sd


# ---------------------------------------------------------------------------------------------- graphs of the kernel tests

def mixed_graph(hidden, seed=3):
    """gated_graphs.degree_graph - in-degrees 0, 1, 2, 63, 64, 65, 129 (and the lane-group counts), parallel edges, self-loops among other
    edges and alone - followed by its own transpose on a second copy of the nodes, so that the OUT-degrees cover the same set as well.
    -> (src, dst int32, n)."""
    gr = degree_graph(hidden, seed=seed)
    n = gr["n"]
    src = torch.cat([gr["src"], gr["dst"] + n])
    dst = torch.cat([gr["dst"], gr["src"] + n])
    din, dout = torch.bincount(dst.long(), minlength=2 * n), torch.bincount(src.long(), minlength=2 * n)
    for d in (0, 1, 2, 63, 64, 65, 129):
        assert (din == d).any() and (dout == d).any(), d
    return src.int(), dst.int(), 2 * n


def hub_edges(in_edges=5000, ordinary=200):
    gr = hub_graph(in_edges, ordinary)
    return gr["src"], gr["dst"], gr["n"]


# ---------------------------------------------------------------------------------------------- the fp64 statement of the kernel

def neighbour_lists(src, dst, n, both):
    """g' as an edge list: every in-edge, the reverse copy of every edge (both), one loop per node."""
    src, dst = src.long(), dst.long()
    loops = torch.arange(n)
    if both:
        return torch.cat([src, dst, loops]), torch.cat([dst, src, loops])
    return torch.cat([src, loops]), torch.cat([dst, loops])


def neighbour_sum_f64(h, src, dst, n, sscale=None, dscale=None, both=False):
    """-> (out, bound) in fp64: out[i] = dscale[i] * sum_{j in N'(i)} sscale[j] h[j], and the standard bound of ANY summation order of
    fp32 terms with one rounding per scale multiply, bound[i] = (|N'(i)| + 2) * 2^-23 * sum_j |dscale[i] sscale[j] h[j]|."""
    gs, gd = neighbour_lists(src, dst, n, both)
    h64 = h.double()
    terms = h64[gs] if sscale is None else h64[gs] * sscale.double()[gs, None]
    if dscale is not None:
        terms = terms * dscale.double()[gd, None]
    out = torch.zeros_like(h64).index_add_(0, gd, terms)
    mag = torch.zeros_like(h64).index_add_(0, gd, terms.abs())
    count = torch.bincount(gd, minlength=n).double()
    return out, (count[:, None] + 2.0) * EPS32 * mag


# ---------------------------------------------------------------------------------------------- the fp32 restatement of the models

def _degrees(src, dst, n, directed):
    """(din', dout') of g', float32."""
    din, dout = torch.bincount(dst, minlength=n).float(), torch.bincount(src, minlength=n).float()
    if directed:
        return din + 1, dout + 1
    return din + dout + 1, din + dout + 1


def gcn_layer(sd, pfx, src, dst, n, h, directed):
    """a[i] = din'[i]^-1/2 sum_{j in N'(i)} dout'[j]^-1/2 h[j];  h' = a weight + bias   (weight is [in, out])."""
    din, dout = _degrees(src, dst, n, directed)
    gs, gd = neighbour_lists(src, dst, n, not directed)
    a = torch.zeros_like(h).index_add_(0, gd, (h * dout.pow(-0.5)[:, None])[gs]) * din.pow(-0.5)[:, None]
    return a @ sd[pfx + "weight"] + sd[pfx + "bias"]


def sage_layer(sd, pfx, src, dst, n, h, directed):
    """m[i] = 1/din'[i] sum_{j in N'(i)} h[j];  h' = h fc_self^T + m fc_neigh^T + bias."""
    din, _ = _degrees(src, dst, n, directed)
    gs, gd = neighbour_lists(src, dst, n, not directed)
    m = torch.zeros_like(h).index_add_(0, gd, h[gs]) / din[:, None]
    return F.linear(h, sd[pfx + "fc_self.weight"]) + F.linear(m, sd[pfx + "fc_neigh.weight"]) + sd[pfx + "bias"]


def baseline_model(kind, sd, src, dst, n, x, e, num_layers, directed=True):
    """Logits [E,1] of GCNModel (kind "gcn") or SAGEModel ("sage") from a state dict, in eval mode."""
    src, dst = src.long(), dst.long()
    enc = lambda p, t: F.linear(torch.relu(F.linear(t, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])), sd[p + ".linear2.weight"],  # noqa: E731
                                sd[p + ".linear2.bias"])
    h, ee = enc("node_encoder", x), enc("edge_encoder", e)
    layer = gcn_layer if kind == "gcn" else sage_layer
    for i in range(num_layers):
        h = layer(sd, f"gnn.convs.{i}.", src, dst, n, h, directed)
        if i + 1 < num_layers:
            h = torch.relu(h)
    z = torch.relu(F.linear(torch.cat([h[src], h[dst], ee], 1), sd["predictor.W1.weight"], sd["predictor.W1.bias"]))
    z = torch.relu(F.linear(z, sd["predictor.W2.weight"], sd["predictor.W2.bias"]))
    return F.linear(z, sd["predictor.W3.weight"], sd["predictor.W3.bias"])


def prob_diff(got, want):
    return (torch.sigmoid(got.detach().cpu().double()) - torch.sigmoid(want.double())).abs().max().item()


