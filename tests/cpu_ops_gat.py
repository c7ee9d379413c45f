"""CHECKER backend for GATModel: tests/cpu_ops_baselines.py plus a torch-CPU statement of the attention-sum entries (include/gnnome_hip.h:
gnnome_node_attention_sum_f32, _stats_f32, _bwd_f32 and their partition forms _part_f32, _stats_part_f32, _bwd_dst_part_f32,
_bwd_src_part_f32).

Test infrastructure only: it lets the host logic of the partitioned GATModel (gnnome_amd/dist.py, engine_gat's partition section) run on CPU
ranks over gloo.  The sums here are index_add sums over the shard's lists: the CONTRACT of the entries - which rows are read, which are
written, that the source phase reads g and work at halo rows - not their association; bit equality with the whole-graph entries is a
property of the kernels and is tested on the device.  Rows an entry must not write are left as they were; rows a caller must fill before
an entry reads them are NaN until it does (fresh tables are made of NaN), so a missing exchange shows."""
import types

import torch

import cpu_ops_baselines

HEADS = 3
Views = cpu_ops_baselines.Views


def _list(ptr, idx, rows):
    """(owner row, entry) of every item of the lists of rows 0 .. rows."""
    p = ptr[:rows + 1].long()
    owner = torch.repeat_interleave(torch.arange(rows), p[1:] - p[:-1])
    entries = idx[int(p[0]):int(p[-1])].long() if rows else idx[:0].long()
    return owner, entries


def _into(views, rows, both):
    """(source, destination) of every edge of g' that ENTERS a row < rows: the loop, the in-list, `both`: the reverse copies of the out-list."""
    own = torch.arange(rows)
    d_in, s_in = _list(views.in_ptr, views.srt_src, rows)
    src, dst = [own, s_in], [own, d_in]
    if both:
        d_out, s_out = _list(views.out_ptr, views.out_dst, rows)
        src.append(s_out)
        dst.append(d_out)
    return torch.cat(src), torch.cat(dst)


def _outof(views, rows, both):
    """(source, destination) of every edge of g' that LEAVES a row < rows: the loop, the out-list, `both`: the reverse copies of the in-list."""
    own = torch.arange(rows)
    s_out, d_out = _list(views.out_ptr, views.out_dst, rows)
    src, dst = [own, s_out], [own, d_out]
    if both:
        s_in, d_in = _list(views.in_ptr, views.srt_src, rows)
        src.append(s_in)
        dst.append(d_in)
    return torch.cat(src), torch.cat(dst)


def _add(rows, index, values):
    return torch.zeros((rows,) + tuple(values.shape[1:]), dtype=values.dtype).index_add_(0, index, values)


def _leaky(x, slope):
    return torch.where(x > 0, x, slope * x)


def _new(rows, cols):
    return torch.full((rows, cols), float("nan"))


def node_attention_sum_stats_part(feat, views, n_own, el, er, bias=None, negative_slope=0.2, both=False, out=None, stats=None):
    n_own, n = int(n_own), views.num_nodes
    assert feat.shape[0] == n and el.shape == (n, 4) and er.shape[0] >= n_own and 0 <= n_own <= n and not views.transposed
    W = feat.shape[1]
    H = W // HEADS
    gs, gd = _into(views, n_own, both)
    s = _leaky(el[gs, :HEADS] + er[gd, :HEADS], negative_slope)
    m = torch.full((n_own, HEADS), float("-inf")).scatter_reduce(0, gd[:, None].expand_as(s), s, "amax", include_self=True)
    w = torch.exp(s - m[gd])
    inv = 1.0 / _add(n_own, gd, w)
    a = w * inv[gd]
    res = _add(n_own, gd, a[:, :, None] * feat[gs].view(-1, HEADS, H)).view(n_own, W)
    if bias is not None:
        res = res + bias
    out = _new(n_own, W) if out is None else out
    stats = _new(n_own, 8) if stats is None else stats
    assert out.shape[0] >= n_own and stats.shape[0] >= n_own
    out[:n_own] = res
    stats[:n_own] = torch.cat([m, torch.zeros(n_own, 1), inv, torch.zeros(n_own, 1)], 1)
    return out, stats


def node_attention_sum_part(feat, views, n_own, el, er, bias=None, negative_slope=0.2, both=False, out=None):
    return node_attention_sum_stats_part(feat, views, n_own, el, er, bias, negative_slope, both, out)[0]


def _weights(x, m, inv, slope):
    a = torch.exp(_leaky(x, slope) - m) * inv
    return a, a * torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))


def node_attention_sum_bwd_dst_part(g, views, n_own, feat, el, er, out, stats, bias=None, negative_slope=0.2, both=False, der=None, work=None):
    n_own, n = int(n_own), views.num_nodes
    assert feat.shape[0] == n and el.shape == (n, 4) and not views.transposed
    assert min(g.shape[0], er.shape[0], out.shape[0], stats.shape[0]) >= n_own
    W = feat.shape[1]
    H = W // HEADS
    gs, gd = _into(views, n_own, both)
    G = g[:n_own].view(n_own, HEADS, H)                                          # (owned rows of g only: its halo rows may still be in flight)
    m, inv = stats[:n_own, :HEADS], stats[:n_own, 4:4 + HEADS]
    A = out[:n_own] if bias is None else out[:n_own] - bias
    D = (G * A.view(n_own, HEADS, H)).sum(-1)
    _, ag = _weights(el[gs, :HEADS] + er[gd, :HEADS], m[gd], inv[gd], negative_slope)
    dx = ag * ((G[gd] * feat[gs].view(-1, HEADS, H)).sum(-1) - D[gd])
    der = _new(n_own, 4) if der is None else der
    work = _new(n, 16) if work is None else work
    assert work.shape == (n, 16) and der.shape[0] >= n_own
    z = torch.zeros(n_own, 1)
    der[:n_own] = torch.cat([_add(n_own, gd, dx), z], 1)
    work[:n_own] = torch.cat([er[:n_own, :HEADS], z, m, z, inv, z, D, z], 1)     # rows >= n_own: not touched
    return der, work


def node_attention_sum_bwd_src_part(g, views, n_own, feat, el, work, negative_slope=0.2, both=False, dfeat=None, del_=None):
    n_own, n = int(n_own), views.num_nodes
    assert g.shape[0] == n and work.shape == (n, 16) and feat.shape[0] >= n_own and el.shape[0] >= n_own and not views.transposed
    W = g.shape[1]
    H = W // HEADS
    gs, gd = _outof(views, n_own, both)
    G = g.view(n, HEADS, H)
    er, m, inv, D = (work[:, 4 * k:4 * k + HEADS] for k in range(4))
    a, ag = _weights(el[gs, :HEADS] + er[gd], m[gd], inv[gd], negative_slope)
    dx = ag * ((G[gd] * feat[gs].view(-1, HEADS, H)).sum(-1) - D[gd])
    dfeat = _new(n_own, W) if dfeat is None else dfeat
    del_ = _new(n_own, 4) if del_ is None else del_
    dfeat[:n_own] = _add(n_own, gs, a[:, :, None] * G[gd]).view(n_own, W)
    del_[:n_own] = torch.cat([_add(n_own, gs, dx), torch.zeros(n_own, 1)], 1)
    return dfeat, del_


# ---- the whole-graph entries: the part forms with every row owned

def node_attention_sum_stats(feat, views, el, er, bias=None, negative_slope=0.2, both=False, out=None, stats=None):
    return node_attention_sum_stats_part(feat, views, views.num_nodes, el, er, bias, negative_slope, both, out, stats)


def node_attention_sum(feat, views, el, er, bias=None, negative_slope=0.2, both=False, out=None):
    return node_attention_sum_stats(feat, views, el, er, bias, negative_slope, both, out)[0]


def node_attention_sum_bwd(g, views, feat, el, er, out, stats, bias=None, negative_slope=0.2, both=False, dP=None):
    n, W = g.shape
    if dP is None:
        dfeat, del_, der = _new(n, W), _new(n, 4), _new(n, 4)
    else:
        dfeat, del_, der = dP[:, :W], dP[:, W:W + 4], dP[:, W + 4:W + 8]
        dP[:, W + 8:].zero_()
    _, work = node_attention_sum_bwd_dst_part(g, views, n, feat, el, er, out, stats, bias, negative_slope, both, der=der)
    node_attention_sum_bwd_src_part(g, views, n, feat, el, work, negative_slope, both, dfeat=dfeat, del_=del_)
    return dfeat, del_, der


BACKEND = types.SimpleNamespace(**vars(cpu_ops_baselines.BACKEND), node_attention_sum=node_attention_sum,
                                node_attention_sum_stats=node_attention_sum_stats, node_attention_sum_bwd=node_attention_sum_bwd,
                                node_attention_sum_part=node_attention_sum_part, node_attention_sum_stats_part=node_attention_sum_stats_part,
                                node_attention_sum_bwd_dst_part=node_attention_sum_bwd_dst_part,
                                node_attention_sum_bwd_src_part=node_attention_sum_bwd_src_part)
