"""Generate tests/golden/g18_gat_h64.pt from the REFERENCE's own GATModel.  Run in the build container only, on the CPU:

    python tests/golden/make_golden_gat.py            # needs /root/reference (read-only)

It imports the reference's unmodified `models.GATModel` (models/full_graph.py:78-97 -> layers/node_encoder.py, edge_encoder.py ->
layers/processor.py:49-70 -> layers/score_predictor.py:5-24) with `tests/golden/_dgl_shim` standing in for DGL, runs it in eval mode on one
small seeded graph and stores inputs, state dict and logits, directed True and False.  The fixture is data; no reference source is copied.

DGL 0.8.1 is not installed, and the shim (left as it is) has neither the convolution nor `add_self_loop` / `add_reverse_edges`: they are
put in place here at run time, BEFORE the reference's modules are imported, as plain-torch statements of DGL 0.8.1's documented semantics
(the recipe of make_golden_baselines.py):
  add_self_loop(g)        one more edge i -> i per node, appended after g's edges, whether or not g already has one
  add_reverse_edges(g)    src|dst -> dst|src: the reverse copy of edge k gets id E + k
  GATConv(in, out, num_heads, feat_drop, attn_drop=0), in == out; negative_slope=0.2, residual=False, activation=None, bias=True:
                          feat = fc(feat_drop(h)).view(N, heads, out);  el = (feat * attn_l).sum(-1), er = (feat * attn_r).sum(-1)
                          per edge j -> i: s = leaky_relu(el[j] + er[i], 0.2);  a = softmax of s over the in-edges of i, per head
                          rst[i] = sum a feat[j] + bias.view(1, heads, out)  -> [N, heads, out]
                          fc: nn.Linear(in, heads * out) without bias; attn_l, attn_r [1, heads, out]; all three Xavier normal with the
                          ReLU gain; bias [heads * out] zeros; res_fc a None buffer (no state-dict entry)
The reference's GAT_processor prints a line at construction; it is left to.
"""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

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


class GATConv(nn.Module):
    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2, residual=False, activation=None,
                 allow_zero_in_degree=False, bias=True):
        super().__init__()
        assert in_feats == out_feats and not attn_drop and not residual and activation is None and bias
        self._num_heads, self._out_feats = num_heads, out_feats
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.feat_drop = nn.Dropout(feat_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.leaky_relu = nn.LeakyReLU(negative_slope)
        self.register_buffer("res_fc", None)
        self.bias = nn.Parameter(torch.zeros(num_heads * out_feats))
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)

    def forward(self, graph, feat):
        src, dst = graph.edges()
        n, heads, out = graph.num_nodes(), self._num_heads, self._out_feats
        assert (torch.bincount(dst, minlength=n) > 0).all()          # DGL raises on a zero in-degree node; g' has none
        feat = self.fc(self.feat_drop(feat)).view(n, heads, out)
        el, er = (feat * self.attn_l).sum(-1), (feat * self.attn_r).sum(-1)
        s = self.leaky_relu(el[src] + er[dst])                          # [E', heads]
        top = torch.full((n, heads), float("-inf")).scatter_reduce(0, dst[:, None].expand_as(s), s, "amax")
        w = torch.exp(s - top[dst])
        a = self.attn_drop(w / torch.zeros(n, heads).index_add_(0, dst, w)[dst])
        rst = torch.zeros(n, heads, out).index_add_(0, dst, a[:, :, None] * feat[src])
        return rst + self.bias.view(1, heads, out)


dgl.add_reverse_edges, dgl.add_self_loop = _add_reverse_edges, _add_self_loop
dgl_conv.GATConv = GATConv

import models  # noqa: E402  (the reference)

from baseline_graphs import model_graph, random_state_dict  # noqa: E402

N, E, HIDDEN, HIDDEN_NE, LAYERS, HS = 40, 200, 64, 16, 2, 64


def main():
    torch.set_num_threads(1)
    src, dst, x, e = model_graph(N, E, seed=18)
    torch.manual_seed(18)
    sd = random_state_dict(models.GATModel(2, 2, HIDDEN, HIDDEN_NE, LAYERS, HS, "batch", dropout=0.0), seed=18)
    logits = {}
    for directed in (True, False):
        m = models.GATModel(2, 2, HIDDEN, HIDDEN_NE, LAYERS, HS, "batch", dropout=0.0, directed=directed)
        m.load_state_dict(sd)
        m.eval()
        g = dgl.graph((src.long(), dst.long()), num_nodes=N)
        with torch.no_grad():
            logits[directed] = m(g, x, e).clone()
        assert not g.ndata and not g.edata and logits[directed].shape == (E, 1)
    out = dict(src=src, dst=dst, num_nodes=N, x=x, e=e, hidden=HIDDEN, hidden_ne=HIDDEN_NE, layers=LAYERS, hs=HS, heads=3,
               state_dict=sd, keys=list(sd), shapes=[tuple(v.shape) for v in sd.values()],
               logits_directed=logits[True], logits_undirected=logits[False])
    path = os.path.join(HERE, "g18_gat_h64.pt")
    torch.save(out, path)
    print(f"g18_gat_h64.pt: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
