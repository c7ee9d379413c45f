"""Generate tests/golden/g16_gated_h64.pt from the REFERENCE's own GatedGCNModel.  Run in the build container only, on the CPU:

    python tests/golden/make_golden_gated.py            # needs /root/reference (read-only)

It imports the reference's unmodified `models.GatedGCNModel` (models/full_graph.py:33-53 -> layers/node_encoder.py, edge_encoder.py ->
layers/processor.py:22-32 -> layers/gated_gcn_full.py:145-230 -> layers/score_predictor.py:5-24) with `tests/golden/_dgl_shim` standing in
for DGL, runs it in eval mode on one small seeded graph and stores inputs, state dicts and logits: batch and layer normalization,
directed True and False.  The fixture is data; no reference source is copied.  The shim has no `add_reverse_edges`
(full_graph.py:48): it is added here at run time - src|dst -> dst|src, the reverse copy of edge k gets id E + k.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "_dgl_shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
sys.path.insert(3, os.path.join(ROOT, "tests"))

import dgl  # noqa: E402  (the shim)

if not hasattr(dgl, "add_reverse_edges"):
    def _add_reverse_edges(g, copy_ndata=True, copy_edata=False, **_):
        src, dst = g.edges()
        return dgl.graph((torch.cat([src, dst]), torch.cat([dst, src])), num_nodes=g.num_nodes())
    dgl.add_reverse_edges = _add_reverse_edges

import models  # noqa: E402  (the reference)

from gated_graphs import model_graph, random_gated_state_dict  # noqa: E402

N, E, HIDDEN, HIDDEN_NE, LAYERS, HS = 40, 200, 64, 16, 2, 64


def main():
    torch.set_num_threads(1)
    src, dst, x, e = model_graph(N, E, seed=16)
    out = dict(src=src, dst=dst, num_nodes=N, x=x, e=e, hidden=HIDDEN, hidden_ne=HIDDEN_NE, layers=LAYERS, hs=HS, cases={})
    for norm in ("batch", "layer"):
        torch.manual_seed(16)
        sd = random_gated_state_dict(models.GatedGCNModel(2, 2, HIDDEN, HIDDEN_NE, LAYERS, HS, norm), seed=16 + len(norm))
        logits = {}
        for directed in (True, False):
            m = models.GatedGCNModel(2, 2, HIDDEN, HIDDEN_NE, LAYERS, HS, norm, directed=directed)
            m.load_state_dict(sd)
            m.eval()
            g = dgl.graph((src.long(), dst.long()), num_nodes=N)
            with torch.no_grad():
                logits[directed] = m(g, x, e).clone()
            assert not g.ndata and not g.edata
        out["cases"][norm] = dict(state_dict=sd, keys=list(sd), logits_directed=logits[True], logits_undirected=logits[False])
    path = os.path.join(HERE, "g16_gated_h64.pt")
    torch.save(out, path)
    print(f"g16_gated_h64.pt: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
