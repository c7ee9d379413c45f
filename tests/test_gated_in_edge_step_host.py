"""The host logic of the one-direction training step (engine_gated._InEdgeStep: kernel sequence, the [N,4H] blocks, the doubled graph's
row maps, one bn_e update, the parameter names) on the checker backend tests/cpu_ops.py, against torch autograd over the plain-torch
restatement.  The two entries of csrc/node_aggregate_in_bwd.hip are stated here through the checker's symmetric ones with zero tables.
Runs without a GPU; the kernels themselves are tested in test_aggregate_in_bwd.py and test_gated_training_in_edge.py."""
import types

import pytest
import torch
import torch.nn.functional as F

from gnnome_amd import engine_gated
from gnnome_amd.models import GatedGCNModel

import cpu_ops
import gated_graphs as gg
from test_hip_training import _check_grads


def _node_aggregate_in_raw(e, A1h, A2h, views, num_nodes=None):
    n = views.num_nodes if num_nodes is None else num_nodes
    v, fwd, rdf, _, _ = cpu_ops.node_aggregate_raw(e, A1h, A2h, torch.zeros_like(A2h), views, 1, n)
    return v, fwd, rdf


def _node_aggregate_in_bwd(e, Tf, Uf, A2h, views, de, out=None):
    zero = torch.zeros_like(Tf)
    cpu_ops.agg_edge_bwd(e, Tf, Uf, zero, zero, A2h, torch.zeros_like(A2h), views, de)
    _, dA2h = cpu_ops.node_aggregate_raw(e, None, zero, Tf, views, 2, views.num_nodes)
    return dA2h


BACKEND = types.SimpleNamespace(**{k: v for k, v in vars(cpu_ops).items() if not k.startswith("_")},
                                node_aggregate_in_raw=_node_aggregate_in_raw, node_aggregate_in_bwd=_node_aggregate_in_bwd)


class _CpuDoubled:
    def __init__(self, views, src, dst):
        self.views = cpu_ops.CpuViews(*engine_gated.doubled_edge_list(src, dst), views.num_nodes)
        self.enc_gather, self.score_gather = engine_gated.doubled_row_maps(self.views.srt_eid, views.srt_eid, views.num_edges)


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("norm", ("batch", "layer"))
def test_the_step_on_the_checker_backend_matches_torch_autograd(norm, directed):
    n, e_cnt, hidden, nl = 30, 120, 64, 2
    src, dst, x, e = gg.model_graph(n, e_cnt, seed=5)
    y = (torch.rand(e_cnt, generator=torch.Generator().manual_seed(2)) < 0.6).float()
    m = GatedGCNModel(2, 2, hidden, 16, nl, 64, norm, dropout=0.0, directed=directed)
    sd = gg.random_gated_state_dict(m, seed=8)
    m.load_state_dict(sd)
    leaves = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    want_logits = gg.gated_model(leaves, src, dst, n, x, e, nl, directed=directed, training=True)
    F.binary_cross_entropy_with_logits(want_logits.squeeze(-1), y).backward()

    m.train()
    views = cpu_ops.CpuViews(src, dst, n)
    sg = engine_gated._StepGraph(views, directed, doubled=lambda v: _CpuDoubled(v, src, dst), ops=BACKEND)
    names, params = zip(*m.named_parameters())
    logits = engine_gated._InEdgeStep.apply(m, sg, x, e, list(names), *params)
    F.binary_cross_entropy_with_logits(logits.squeeze(-1), y).backward()
    assert (torch.sigmoid(logits.detach()) - torch.sigmoid(want_logits.detach())).abs().max().item() < 1e-5
    _check_grads({k: p.grad for k, p in m.named_parameters()}, {k: leaves[k].grad for k in names}, rtol=1e-3)
    if norm == "batch":          # ONE momentum update of bn_e and of bn_h per layer and step
        bufs = dict(m.named_buffers())
        assert bufs["gnn.convs.1.bn_e.num_batches_tracked"].item() == 4 and bufs["gnn.convs.1.bn_h.num_batches_tracked"].item() == 4
        assert not torch.equal(bufs["gnn.convs.0.bn_e.running_mean"], sd["gnn.convs.0.bn_e.running_mean"])
    with pytest.raises(RuntimeError, match="released"):
        logits.sum().backward()
