"""Generate tests/golden/g17_baselines_h64.pt from the REFERENCE's own GCNModel and SAGEModel.  Run in the build container only, on the CPU:

    python tests/golden/make_golden_baselines.py            # needs /root/reference (read-only)

It imports the reference's unmodified `models.GCNModel` / `models.SAGEModel` (models/full_graph.py:56-75, :100-119 -> layers/node_encoder.py,
edge_encoder.py -> layers/processor.py:35-46, :73-84 -> layers/score_predictor.py:5-24) with `tests/golden/_dgl_shim` standing in for DGL, runs
them in eval mode on one small seeded graph and stores inputs, state dicts and logits, directed True and False.  The fixture is data; no
reference source is copied.

DGL 0.8.1 is not installed, and the shim (left as it is) has neither the two convolutions nor `add_self_loop` / `add_reverse_edges`: they are
put in place here at run time, BEFORE the reference's modules are imported, as plain-torch statements of DGL 0.8.1's documented semantics:
  add_self_loop(g)        one more edge i -> i per node, appended after g's edges, whether or not g already has one
  add_reverse_edges(g)    src|dst -> dst|src: the reverse copy of edge k gets id E + k
  GraphConv(in, out, norm='both', weight=True, bias=True), in == out (aggregate first):
                          rst = ((sum over in-edges of feat[src] * out_deg[src]^-1/2) @ weight) * in_deg^-1/2 + bias, weight [in, out] Xavier uniform
  SAGEConv(in, out, 'mean', feat_drop), in == out:
                          rst = fc_self(feat) + fc_neigh(sum over in-edges of feat[src] / in_deg) + bias; fc_* without bias, Xavier uniform (ReLU gain)
(degrees clamped to >= 1 as DGL does; on g' they are never zero).
"""
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "_dgl_shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
sys.path.insert(3, os.path.join(ROOT, "tests"))

import dgl  # noqa: E402  (the shim)
import dgl.nn.pytorch.conv as dgl_conv  # noqa: E402


def _add_reverse_edges(g, copy_ndata=True, copy_edata=False, **_):
    src, dst = g.edges()
    return dgl.graph((torch.cat([src, dst]), torch.cat([dst, src])), num_nodes=g.num_nodes())


def _add_self_loop(g, **_):
    src, dst = g.edges()
    loops = torch.arange(g.num_nodes(), dtype=src.dtype)
    return dgl.graph((torch.cat([src, loops]), torch.cat([dst, loops])), num_nodes=g.num_nodes())


def _in_edge_sum(g, rows):
    src, dst = g.edges()
    return torch.zeros_like(rows).index_add_(0, dst, rows[src])


class GraphConv(nn.Module):
    def __init__(self, in_feats, out_feats, norm="both", weight=True, bias=True):
        super().__init__()
        assert norm == "both" and weight and bias and in_feats == out_feats
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats))
        self.bias = nn.Parameter(torch.zeros(out_feats))
        nn.init.xavier_uniform_(self.weight)

    def forward(self, graph, feat):
        src, dst = graph.edges()
        n = graph.num_nodes()
        out_deg = torch.bincount(src, minlength=n).float().clamp(min=1)
        in_deg = torch.bincount(dst, minlength=n).float().clamp(min=1)
        rst = _in_edge_sum(graph, feat * out_deg.pow(-0.5)[:, None])
        rst = torch.matmul(rst, self.weight)
        return rst * in_deg.pow(-0.5)[:, None] + self.bias


class SAGEConv(nn.Module):
    def __init__(self, in_feats, out_feats, aggregator_type, feat_drop=0.0, bias=True):
        super().__init__()
        assert aggregator_type == "mean" and bias and in_feats == out_feats
        self.feat_drop = nn.Dropout(feat_drop)
        self.bias = nn.Parameter(torch.zeros(out_feats))
        self.fc_self = nn.Linear(in_feats, out_feats, bias=False)
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=False)
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)

    def forward(self, graph, feat):
        _, dst = graph.edges()
        feat = self.feat_drop(feat)
        in_deg = torch.bincount(dst, minlength=graph.num_nodes()).float().clamp(min=1)
        h_neigh = _in_edge_sum(graph, feat) / in_deg[:, None]
        return self.fc_self(feat) + self.fc_neigh(h_neigh) + self.bias


dgl.add_reverse_edges, dgl.add_self_loop = _add_reverse_edges, _add_self_loop
dgl_conv.GraphConv, dgl_conv.SAGEConv = GraphConv, SAGEConv

import models  # noqa: E402  (the reference)

from baseline_graphs import model_graph, random_state_dict  # noqa: E402

N, E, HIDDEN, HIDDEN_NE, LAYERS, HS = 40, 200, 64, 16, 2, 64


def main():
    torch.set_num_threads(1)
    src, dst, x, e = model_graph(N, E, seed=17)
    out = dict(src=src, dst=dst, num_nodes=N, x=x, e=e, hidden=HIDDEN, hidden_ne=HIDDEN_NE, layers=LAYERS, hs=HS, cases={})
    for kind, cls, extra in (("gcn", models.GCNModel, {}), ("sage", models.SAGEModel, {"dropout": 0.0})):
        torch.manual_seed(17)
        sd = random_state_dict(cls(2, 2, HIDDEN, HIDDEN_NE, LAYERS, HS, "batch", **extra), seed=17 + len(kind))
        logits = {}
        for directed in (True, False):
            m = cls(2, 2, HIDDEN, HIDDEN_NE, LAYERS, HS, "batch", directed=directed, **extra)
            m.load_state_dict(sd)
            m.eval()
            g = dgl.graph((src.long(), dst.long()), num_nodes=N)
            with torch.no_grad():
                logits[directed] = m(g, x, e).clone()
            assert not g.ndata and not g.edata and logits[directed].shape == (E, 1)
        out["cases"][kind] = dict(state_dict=sd, keys=list(sd), shapes=[tuple(v.shape) for v in sd.values()],
                                  logits_directed=logits[True], logits_undirected=logits[False])
    path = os.path.join(HERE, "g17_baselines_h64.pt")
    torch.save(out, path)
    print(f"g17_baselines_h64.pt: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
