"""A stand-in for the DGL graph that inference.py's get_contigs_greedy / get_subgraph / get_contig_length touch, written for
make_golden_decode.py (build machine only).  Only what those three functions use:

    g.to(device)                     the graph itself (everything lives on the CPU)
    g.num_nodes(), g.num_edges()
    g.edges()                        (src, dst) int64 tensors in edge-id order
    g.ndata, g.edata                 dicts of tensors, one row per node / edge
    g.edges[u_list, v_list].data[k]  g.edata[k] at the ids of the pairs (u_list[j], v_list[j]).  Pair -> id rule: the graph must
                                     hold exactly ONE edge u -> v; no edge, or several (parallel edges), raises - what DGL would
                                     return for several is not specified, so fixtures made with this double hold simple graphs
    node_subgraph(g, keep, store_ids=True)
                                     the induced subgraph on the nodes `keep` (ascending): nodes renumbered by their position in
                                     `keep`, the edges with both ends kept in EDGE-ID ORDER, node and edge data carried over,
                                     ndata[NID] = the kept nodes' original ids, edata[EID] = the kept edges' original ids
"""
import types

import torch

NID = "_ID"
EID = "_ID"


class _PairData:
    def __init__(self, graph, ids):
        self.data = {k: v[ids] for k, v in graph.edata.items()}


class _EdgeView:
    def __init__(self, graph):
        self._g = graph

    def __call__(self):
        return self._g._src, self._g._dst

    def __getitem__(self, pair):
        u_list, v_list = pair
        ids = []
        for u, v in zip(list(u_list), list(v_list)):
            found = self._g._pair_ids.get((int(u), int(v)), [])
            if len(found) != 1:
                raise KeyError(f"{len(found)} edges {int(u)} -> {int(v)}: the double answers for exactly one")
            ids.append(found[0])
        return _PairData(self._g, torch.tensor(ids, dtype=torch.int64))


class Graph:
    def __init__(self, src, dst, num_nodes, ndata=None, edata=None):
        self._src, self._dst, self._n = src.long(), dst.long(), int(num_nodes)
        self.ndata, self.edata = dict(ndata or {}), dict(edata or {})
        self._pair_ids = {}
        for k, (s, d) in enumerate(zip(self._src.tolist(), self._dst.tolist())):
            self._pair_ids.setdefault((s, d), []).append(k)
        self.edges = _EdgeView(self)

    def to(self, device):
        return self

    def num_nodes(self):
        return self._n

    def num_edges(self):
        return int(self._src.numel())


def node_subgraph(g, keep, store_ids=True):
    keep = torch.as_tensor(keep).long()
    assert bool((keep[1:] > keep[:-1]).all()), "kept nodes in ascending order"
    new_id = torch.full((g.num_nodes(),), -1, dtype=torch.int64)
    new_id[keep] = torch.arange(keep.numel())
    src, dst = g.edges()
    kept = torch.nonzero((new_id[src] >= 0) & (new_id[dst] >= 0)).squeeze(1)      # ascending: edge-id order
    sub = Graph(new_id[src[kept]], new_id[dst[kept]], keep.numel(), {k: v[keep] for k, v in g.ndata.items()},
                {k: v[kept] for k, v in g.edata.items()})
    if store_ids:
        sub.ndata[NID] = keep
        sub.edata[EID] = kept
    return sub


dgl = types.SimpleNamespace(node_subgraph=node_subgraph, NID=NID, EID=EID)
