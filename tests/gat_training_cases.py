"""Helpers of the GATModel training tests (tests/test_gat_training_statement.py, test_attention_sum_bwd.py, test_gat_training.py): an
fp64 statement of the attention sum's gradient with a derived error bound, and a plain-torch, differentiable restatement of the model in
TRAIN mode - gat_graphs.gat_model plus GATConv's feat_drop: one scaled keep-mask per layer on the conv's INPUT (DGL 0.8.1's GATConv:
h_src = h_dst = feat_drop(feat) before fc; attn_drop is 0).  Written from the formulas, as gat_graphs.py is."""
import torch
import torch.nn.functional as F

import gat_graphs as gg
from baseline_graphs import EPS32, neighbour_lists

HEADS = 3


def _add(n, index, values):
    return torch.zeros((n,) + tuple(values.shape[1:]), dtype=torch.float64).index_add_(0, index, values)


def attention_sum_bwd_f64(G, feat, el, er, src, dst, n, slope=0.2, both=False, bias=None):
    """-> ((dfeat [n,3H], del [n,3], der [n,3]), (their bounds, same shapes)), fp64 from the fp32 inputs G = d out [n,3H], feat [n,3H],
    el / er [n, >= 3], over g' of baseline_graphs.neighbour_lists.  Per head and edge p = (j -> i) of g', with a the softmax weights of
    gat_graphs.attention_sum_f64:
        dot_p = G_i . feat_j      D_i = sum_{q -> i} a_q dot_q      dx_p = a_p gate_p (dot_p - D_i),   gate_p = 1 if x_p > 0 else slope
        dfeat[j] = sum_{p: src = j} a_p G[dst_p]      del[j] = sum_{p: src = j} dx_p      der[i] = sum_{p: dst = i} dx_p
    THE BOUND, c * 2^-23 * M per element, of an fp32 evaluation that recomputes a_p = exp2((s_p - m_i) log2e) * (1 / den_i) from the
    forward's fp32 maximum and reciprocal denominator, forms D_i = G_i . (A_i - bias) from the forward's fp32 output A, and sums in ANY
    order.  n_i = |N'(i)| (in-count in g'), n'_j = the out-count of j in g', S_i = max_{p -> i} |x_p|, H = the row width of a head:
      * a weight: exp(s - m) carries (4 + 4 S) 2^-23 relative (attention_sum_f64's derivation); the fp32 denominator is a sum of n such
        weights, (n + 1) more, its reciprocal 1, the product a = w * inv 1:  eps_a(i) = n_i + 3 + 2 (4 + 4 S_i);
      * a dot of H fp32 products in any order: H 2^-23 * sum_c |G_c| |feat_c|  (H u for the sum, the products' roundings inside the
        factor 2 of u = 2^-24 -> 2^-23).  Mdot_p = sum_c |G_i,c| |feat_j,c|;
      * D_i: the forward's A has the error (2 n + 4 + 2 (4 + 4 S)) 2^-23 * F_i, F_i,c = sum_q a_q |feat_q,c|  (attention_sum_f64's
        bound); adding and subtracting the bias are two more roundings of at most 2^-23 (F + 2 |bias|) together; then the dot, H more:
        |dD_i| <= (2 n_i + 6 + 2 (4 + 4 S_i) + H) 2^-23 * MD_i,   MD_i = sum_c |G_i,c| (F_i,c + 2 |bias_c|);
      * dx_p = ag_p (dot_p - D_i): ag = a * gate one more rounding, the subtraction and the product one each, so with
        c_x(i) = (eps_a(i) + 3) + (2 n_i + 6 + 2 (4 + 4 S_i)) + H = 3 n_i + 12 + 16 (1 + S_i) + H:
        |d dx_p| <= c_x(i) 2^-23 * Mx_p,   Mx_p = a_p |gate_p| (Mdot_p + MD_i)  - dot_p - D_i with every product term replaced by its
        absolute value: the cancellation in G . feat - D is NOT counted as accuracy;
      * a sum of k terms in any order adds (k + 1) 2^-23 * sum |term|, and |dx_p| <= Mx_p:
        bound der[i]    = (c_x(i) + n_i + 1) 2^-23 * sum_{p -> i} Mx_p
        bound del[j]    = 2^-23 * sum_{p: src = j} (c_x(dst_p) + n'_j + 1) Mx_p
        bound dfeat[j,c] = 2^-23 * sum_{p: src = j} (eps_a(dst_p) + n'_j + 1) a_p |G[dst_p, c]|
    Nothing in it is measured."""
    H = feat.shape[1] // HEADS
    gs, gd = neighbour_lists(src, dst, n, both)
    f, g = feat.double().view(n, HEADS, H), G.double().view(n, HEADS, H)
    x = el.double()[:, :HEADS][gs] + er.double()[:, :HEADS][gd]
    s = torch.where(x > 0, x, slope * x)
    w = torch.exp(s - gg._segment_max(s, gd, n)[gd])
    a = w / _add(n, gd, w)[gd]
    gate = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))
    dot = (g[gd] * f[gs]).sum(-1)
    D = _add(n, gd, a * dot)
    dx = a * gate * (dot - D[gd])
    dfeat = _add(n, gs, a[:, :, None] * g[gd])
    dl, dr = _add(n, gs, dx), _add(n, gd, dx)
    # ---- the bound
    n_in, n_out = torch.bincount(gd, minlength=n).double()[:, None], torch.bincount(gs, minlength=n).double()[:, None]
    S = gg._segment_max(x.abs(), gd, n)
    eps_a = n_in + 3.0 + 2.0 * (4.0 + 4.0 * S)
    c_x = 3.0 * n_in + 12.0 + 16.0 * (1.0 + S) + H
    Fm = _add(n, gd, a[:, :, None] * f[gs].abs())
    if bias is not None:
        Fm = Fm + 2.0 * bias.double().abs().view(1, HEADS, H)
    MD = (g.abs() * Fm).sum(-1)
    Mx = a * gate.abs() * ((g[gd].abs() * f[gs].abs()).sum(-1) + MD[gd])
    b_der = EPS32 * (c_x + n_in + 1.0) * _add(n, gd, Mx)
    b_del = EPS32 * _add(n, gs, (c_x[gd] + n_out[gs] + 1.0) * Mx)
    b_dfeat = EPS32 * _add(n, gs, ((eps_a[gd] + n_out[gs] + 1.0) * a)[:, :, None] * g[gd].abs())
    return (dfeat.view(n, HEADS * H), dl, dr), (b_dfeat.view(n, HEADS * H), b_del, b_der)


def gat_model_train(leaves, src, dst, n, x, e, layers, directed=True, masks=None):
    """Logits [E,1] of GATModel in train mode from a state dict (leaves that require grad are differentiated through): gat_graphs.gat_model
    with masks[i] ([n, H] or None) multiplied onto conv i's input."""
    sd = leaves
    src, dst = src.long(), dst.long()
    enc = lambda p, t: F.linear(torch.relu(F.linear(t, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])), sd[p + ".linear2.weight"],  # noqa: E731
                                sd[p + ".linear2.bias"])
    h, ee = enc("node_encoder", x), enc("edge_encoder", e)
    for i in range(layers):
        if masks is not None and masks[i] is not None:
            h = h * masks[i]
        heads = gg.gat_conv(sd, f"gnn.convs.{i}.", src, dst, n, h, directed)
        h = F.linear(heads, sd[f"gnn.linears.{i}.weight"], sd[f"gnn.linears.{i}.bias"])
        if i + 1 < layers:
            h = torch.relu(h)
    z = torch.relu(F.linear(torch.cat([h[src], h[dst], ee], 1), sd["predictor.W1.weight"], sd["predictor.W1.bias"]))
    z = torch.relu(F.linear(z, sd["predictor.W2.weight"], sd["predictor.W2.bias"]))
    return F.linear(z, sd["predictor.W3.weight"], sd["predictor.W3.bias"])
