"""CHECKER backend for GatedGCNModel: tests/cpu_ops.py plus a torch-CPU statement of the one-direction aggregation entries
(include/gnnome_hip.h: gnnome_node_aggregate_in_f32, _in_raw_f32, _in_bwd_f32 and the partition forms _in_raw_part_f32 / _in_bwd_part_f32).

Test infrastructure only: it lets the host logic of the partitioned GatedGCNModel (gnnome_amd/dist.py, engine_gated._InEdgeStep on a
shard) run on CPU ranks over gloo, and states the expected value of the two partition entries for the GPU tests (any float dtype: the
fp64 evaluation of the header's formulas is this code on double inputs)."""
import types

import torch

import cpu_ops


def _in_sums(e, A2h, views, rows):
    """(sum_in s * A2h[src], sum_in s) for the destinations < rows; A2h may have more rows than that (halo sources)."""
    s, d = views.srt_src.long(), views.srt_dst.long()
    sig = torch.sigmoid(e)
    zeros = torch.zeros((max(rows, int(d.max()) + 1 if d.numel() else 0), e.shape[1]), dtype=e.dtype)
    return zeros.index_add(0, d, sig * A2h[s])[:rows], zeros.index_add(0, d, sig)[:rows]


def node_aggregate_in(e, A1h, A2h, views, h_in, norm_kind, scale, shift, num_nodes_out=None, node_range=None, out=None):
    n = h_in.shape[0]
    n_out = n if num_nodes_out is None else num_nodes_out
    num, den = _in_sums(e, A2h, views, n)
    y = torch.relu(cpu_ops._norm(A1h + num / (den + 1e-6), norm_kind, scale, shift)) + h_in
    if node_range is not None:
        out[node_range[0]:node_range[1]] = y[node_range[0]:node_range[1]]
        return out
    out = torch.full_like(h_in, float("nan"))   # rows >= n_out are not written by the kernel
    out[:n_out] = y[:n_out]
    return out


def node_aggregate_in_raw(e, A1h, A2h, views, num_nodes=None):
    n = views.num_nodes if num_nodes is None else num_nodes
    num, den = _in_sums(e, A2h, views, n)
    rden = 1.0 / (den + 1e-6)
    return A1h[:n] + num * rden, num * rden, rden


def node_aggregate_in_raw_part(e, A1h, A2h, views, n_own):
    assert A2h.shape[0] == views.num_nodes and int(views.in_ptr[n_own]) == views.num_edges, "every local edge ends in an owned node"
    return node_aggregate_in_raw(e, A1h, A2h, views, n_own)


def node_aggregate_in_bwd(e, Tf, Uf, A2h, views, de, out=None):
    return node_aggregate_in_bwd_part(e, Tf, Uf, A2h, views, de, views.num_nodes, out=out)


def node_aggregate_in_bwd_part(e, Tf, Uf, A2h, views, de, n_own, out=None):
    s, d = views.srt_src.long(), views.srt_dst.long()
    assert Tf.shape[0] == n_own and Uf.shape[0] == n_own and (d.numel() == 0 or int(d.max()) < n_own)
    sig = torch.sigmoid(e)
    de.add_(sig * (1 - sig) * (Tf[d] * A2h[s] - Uf[d]))
    dA2h = torch.zeros((views.num_nodes, e.shape[1]), dtype=e.dtype).index_add(0, s, sig * Tf[d])
    if out is None:
        return dA2h
    out.copy_(dA2h)
    return out


BACKEND = types.SimpleNamespace(**{k: v for k, v in vars(cpu_ops).items() if not k.startswith("_")},
                                node_aggregate_in=node_aggregate_in, node_aggregate_in_raw=node_aggregate_in_raw,
                                node_aggregate_in_raw_part=node_aggregate_in_raw_part, node_aggregate_in_bwd=node_aggregate_in_bwd,
                                node_aggregate_in_bwd_part=node_aggregate_in_bwd_part)
