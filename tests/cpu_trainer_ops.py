"""CHECKER backend of trainer.train_partitioned: a torch restatement of the namespace trainer.hip_backend() builds from the package's kernels.

Test infrastructure only.  `kernels` is what dist.PartitionedRunner / GATPartitionedRunner take as ops=: tests/cpu_ops.py with the entries
the other models add (cpu_ops_gated, cpu_ops_baselines, cpu_ops_gat) - every model class of the loop runs on the one namespace.  The views
are cpu_ops's, cluster_inputs is the plain-torch statement of features.cluster_inputs for ONE cluster (the whole, possibly masked, graph),
loss and counts come from oracle.symgated_oracle.symmetry_loss with round(sigmoid(.))."""
import types

import torch
import torch.nn.functional as F

import cpu_ops_gat
import cpu_ops_gated
from oracle.symgated_oracle import calculate_tfpn, symmetry_loss

_GATED = ("node_aggregate_in", "node_aggregate_in_raw", "node_aggregate_in_raw_part", "node_aggregate_in_bwd", "node_aggregate_in_bwd_part")
KERNELS = types.SimpleNamespace(**vars(cpu_ops_gat.BACKEND), **{k: getattr(cpu_ops_gated.BACKEND, k) for k in _GATED})


def _zscore(d):
    return ((d - d.mean()) / d.std()).unsqueeze(1)          # torch.std: unbiased, as train.py:125-135


def cluster_inputs(parts, full_in_deg, full_out_deg, e, y, outer_nid=None, outer_eid=None, need_rev=True):
    """features.cluster_inputs for one cluster that is the whole graph: the FULL graph's stored degrees of the kept nodes, z-scored over
    those nodes; e and y of the kept edges."""
    (sub,) = parts
    nid = sub.nid.long() if outer_nid is None else torch.as_tensor(outer_nid).long()[sub.nid.long()]
    eid = sub.eid.long() if outer_eid is None else torch.as_tensor(outer_eid).long()[sub.eid.long()]
    din, dout = full_in_deg.float()[nid], full_out_deg.float()[nid]
    x = torch.cat([_zscore(din), _zscore(dout)], 1).contiguous()
    x_rev = torch.cat([_zscore(dout), _zscore(din)], 1).contiguous() if need_rev else None
    return [types.SimpleNamespace(x=x, x_rev=x_rev, e=e.float()[eid].contiguous(), y=None if y is None else y.float()[eid].contiguous())]


def edge_loss(logits, logits_rev, labels, pos_weight, alpha=0.0, need_grad=True, need_counts=False):
    """ops.edge_loss: (loss[1], d loss / d logits, d loss / d logits_rev, int64 (TP, TN, FP, FN) of the org logits)."""
    a = logits.detach().clone().requires_grad_(need_grad)
    b = None if logits_rev is None else logits_rev.detach().clone().requires_grad_(need_grad)
    pw = torch.as_tensor(pos_weight, dtype=torch.float32).reshape(1)
    da = db = None
    with torch.enable_grad():        # (called from inside an autograd.Function's forward, and under no_grad in validation)
        loss = F.binary_cross_entropy_with_logits(a, labels, pos_weight=pw) if b is None else symmetry_loss(a, b, labels, pw, alpha)
        if need_grad:
            loss.backward()
            da, db = a.grad, None if b is None else b.grad
    tfpn = torch.tensor(calculate_tfpn(logits.detach(), labels), dtype=torch.int64) if need_counts else None
    return loss.detach().reshape(1), da, db, tfpn


def stored_degrees(views):
    ind = (views.in_ptr[1:] - views.in_ptr[:-1]).float()
    outd = (views.out_ptr[1:] - views.out_ptr[:-1]).float()
    return ind, outd


def edge_features(overlap_length, overlap_similarity):
    from oracle.symgated_oracle import edge_features as oracle_edge_features
    return oracle_edge_features(overlap_length, overlap_similarity)


BACKEND = types.SimpleNamespace(kernels=KERNELS, GraphViews=KERNELS.GraphViews, cluster_inputs=cluster_inputs, edge_loss=edge_loss,
                                stored_degrees=stored_degrees, edge_features=edge_features)
