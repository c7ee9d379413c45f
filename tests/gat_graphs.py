"""Helpers of the GATModel tests (tests/test_gat_statement.py, test_attention_sum.py, test_gat_model.py): an fp64 statement of the
edge-softmax attention sum with its error bound, and a plain-torch fp32 restatement of the whole model (NOT folded: el and er are computed
from feat as DGL does).  Written from the formulas of DGL 0.8.1's GATConv(in, out, num_heads=3) on g' = add_self_loop(g) /
add_self_loop(add_reverse_edges(g)) (models/full_graph.py:78-97; layers/processor.py:49-70), not copied from them."""
import torch
import torch.nn.functional as F

from baseline_graphs import (EPS32, hub_edges, mixed_graph, model_graph, neighbour_lists, prob_diff,  # noqa: F401  (the graphs of the
                             random_state_dict)                                                       # neighbour sum's tests)

HEADS = 3


# ---------------------------------------------------------------------------------------------- the fp64 statement of the kernel

def _segment_max(values, index, n):
    """max over the rows of values[., K] that share index -> [n, K] (-inf where a segment is empty)."""
    out = torch.full((n, values.shape[1]), float("-inf"), dtype=values.dtype)
    return out.scatter_reduce(0, index[:, None].expand_as(values), values, "amax", include_self=True)


def attention_sum_f64(feat, el, er, src, dst, n, slope=0.2, bias=None, both=False):
    """-> (out, bound), both [n, 3H] in fp64 from the fp32 inputs feat[n, 3H], el / er [n, >= 3] (columns 0..2: the heads):
        out[i,k,:] = sum_{p in N'(i)} a_p feat[nbr_p,k,:] + bias[k,:],   a = softmax over N'(i) of leaky_relu(el[nbr_p,k] + er[i,k], slope)
    over g' of baseline_graphs.neighbour_lists (in-edges, `both`: the reverse copies too, one loop per node), and the DERIVED bound
        bound[i,k,:] = (2 |N'(i)| + 4 + 2 (4 + 4 S_ik)) * 2^-23 * sum_p a_p |feat_p|,     S_ik = max_p |el_p + er_i|
    of an fp32 evaluation that takes the maximum first, then exp(s - max), an fp32 numerator and denominator and one division:
      * numerator and denominator each carry the standard (n + 1) 2^-23 error of an n-term fp32 sum in ANY order: 2 n + 2, and 2 more for
        the division (or reciprocal and product) - 2 |N'| + 4;
      * a weight exp(s - max) has a relative error of at most (4 + 4 S) 2^-23: the add el + er, the slope multiply and the subtraction of
        the maximum leave an absolute error of at most 4 S 2^-24 * 2 in the exponent's argument (|s|, |max| <= S, |s - max| <= 2 S), which
        is the weight's relative error; exp's own ulp or two and the |x| 2^-24 of an exp2(x log2 e) fast path with |x| <= 2 S are in the 4 and
        the rest of 4 S;
      * a quotient of two sums of such weights at most doubles the weight term.
    Nothing in it is measured.  The bias is added in fp64 and has no term in the bound: the kernel adds it as a rounding of its own, which the
    tests check exactly (out with a bias == out without + bias), so the bound is asserted on calls without one."""
    H = feat.shape[1] // HEADS
    gs, gd = neighbour_lists(src, dst, n, both)
    f64, l64, r64 = feat.double().view(n, HEADS, H), el.double()[:, :HEADS], er.double()[:, :HEADS]
    x = l64[gs] + r64[gd]
    s = torch.where(x > 0, x, slope * x)
    w = torch.exp(s - _segment_max(s, gd, n)[gd])
    a = w / torch.zeros(n, HEADS, dtype=torch.float64).index_add_(0, gd, w)[gd]
    out = torch.zeros(n, HEADS, H, dtype=torch.float64).index_add_(0, gd, a[:, :, None] * f64[gs])
    mag = torch.zeros(n, HEADS, H, dtype=torch.float64).index_add_(0, gd, a[:, :, None] * f64[gs].abs())
    if bias is not None:
        out = out + bias.double().view(1, HEADS, H)
    count = torch.bincount(gd, minlength=n).double()[:, None]
    S = _segment_max(x.abs(), gd, n)
    bound = ((2.0 * count + 4.0 + 2.0 * (4.0 + 4.0 * S)) * EPS32)[:, :, None] * mag
    return out.view(n, HEADS * H), bound.view(n, HEADS * H)


# ---------------------------------------------------------------------------------------------- the fp32 restatement of the model

def gat_conv(sd, pfx, src, dst, n, h, directed, slope=0.2):
    """DGL's GATConv on g': feat = fc(h) as [n, 3, H]; el = (feat * attn_l).sum(-1), er = (feat * attn_r).sum(-1); per in-edge j -> i of g'
    s = leaky_relu(el[j] + er[i]); a = softmax of s over the in-edges of i; rst[i] = sum a feat[j] + bias.  -> [n, 3H]."""
    H = h.shape[1]
    gs, gd = neighbour_lists(src, dst, n, not directed)
    feat = F.linear(h, sd[pfx + "fc.weight"]).view(n, HEADS, H)
    el, er = (feat * sd[pfx + "attn_l"]).sum(-1), (feat * sd[pfx + "attn_r"]).sum(-1)
    s = F.leaky_relu(el[gs] + er[gd], slope)
    w = torch.exp(s - _segment_max(s, gd, n)[gd])
    a = w / torch.zeros(n, HEADS).index_add_(0, gd, w)[gd]
    rst = torch.zeros(n, HEADS, H).index_add_(0, gd, a[:, :, None] * feat[gs])
    return (rst + sd[pfx + "bias"].view(1, HEADS, H)).reshape(n, HEADS * H)


def gat_model(sd, src, dst, n, x, e, num_layers, directed=True):
    """Logits [E,1] of GATModel from a state dict, in eval mode."""
    src, dst = src.long(), dst.long()
    enc = lambda p, t: F.linear(torch.relu(F.linear(t, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])), sd[p + ".linear2.weight"],  # noqa: E731
                                sd[p + ".linear2.bias"])
    h, ee = enc("node_encoder", x), enc("edge_encoder", e)
    for i in range(num_layers):
        heads = gat_conv(sd, f"gnn.convs.{i}.", src, dst, n, h, directed)
        h = F.linear(heads, sd[f"gnn.linears.{i}.weight"], sd[f"gnn.linears.{i}.bias"])
        if i + 1 < num_layers:
            h = torch.relu(h)
    z = torch.relu(F.linear(torch.cat([h[src], h[dst], ee], 1), sd["predictor.W1.weight"], sd["predictor.W1.bias"]))
    z = torch.relu(F.linear(z, sd["predictor.W2.weight"], sd["predictor.W2.bias"]))
    return F.linear(z, sd["predictor.W3.weight"], sd["predictor.W3.bias"])
