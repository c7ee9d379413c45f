"""Generate tests/golden/walk_audit.json from the REFERENCE's own utils/analyze.py (assert_strand, assert_chromosome, assert_overlap,
:1-38).  Build container only:

    python tests/golden/make_golden_walk_audit.py <path to the reference checkout>

utils/analyze.py imports nothing, so it is loaded from its path as it is; the graph is a stand-in object whose `ndata` is a dict of
int64 tensors (the three functions touch nothing else, so no DGL is needed).  The reference's text runs, none of it is stored.

Stored, data only: the four node arrays, the walks, what each walk is there for, and per walk the text the three functions printed;
and for the two print-only helpers (:41-57) their arguments with the text they printed.
Checked before saving: the reference printed at least one finding of each of the three kinds, and at least one walk printed nothing.
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))

P = 1 << 33   # positions that need more than 32 bits

# node: (strand, start, end, chr)
NODES = [
    (1, 0, 1000, 1), (1, 500, 1500, 1), (1, 1000, 2000, 1), (1, 1500, 2500, 1), (1, 2000, 3000, 1),      # 0-4: a clean + chain
    (-1, 700, 1700, 1), (-1, 900, 1900, 1),                                                              # 5, 6: the other strand
    (1, 1200, 2200, -1),                                                                                 # 7: chromosome X
    (1, 1000, 2000, 1), (1, 1001, 2001, 1),                                                              # 8, 9: start == end[0], == end[0] + 1
    (-1, 5000, 6000, 1), (-1, 4000, 5000, 1), (-1, 4000, 4999, 1),                                       # 10-12: end == start[10], == start[10] - 1
    (-1, 50000, 51000, 1),                                                                               # 13: far away, other strand
    (0, 90000, 91000, 1), (2, 70000, 71000, 1), (2, 80000, 81000, 1),                                    # 14-16: strands that are neither
    (1, P, P + 1000, 1), (1, P + 5000, P + 6000, 1),                                                     # 17, 18: beyond 2^32, a gap
    (1, 3001, 4001, 1),                                                                                  # 19: start == end[4] + 1
    (-1, P + 9000, P + 9500, 2), (-1, P + 100, P + 8999, 2),                                             # 20, 21: - strand beyond 2^32, a gap of 1
]

WALKS = [
    ("clean walk", [0, 1, 2, 3, 4]),
    ("one node", [3]),
    ("strand differs at two later nodes, both against walk[0]", [0, 5, 1, 6, 2]),
    ("chromosome switch to X = -1 and back", [0, 1, 7, 2]),
    ("walk[0] on X: every later node is reported", [7, 1, 2]),
    ("+ pair, dst_start == src_end: silent", [0, 8]),
    ("+ pair, dst_start == src_end + 1", [0, 9]),
    ("- pair, dst_end == src_start: silent", [10, 11]),
    ("- pair, dst_end == src_start - 1", [10, 12]),
    ("mixed-strand pair with a gap: silent in the overlap check", [0, 13]),
    ("strands 0 and 2: reported against walk[0], silent pairs", [0, 14, 15, 16]),
    ("positions beyond 2^32", [17, 18]),
    ("- pair beyond 2^32 on chromosome 2", [20, 21]),
    ("findings at the first and at the last pair", [0, 9, 2, 3, 4, 19]),
    ("a node twice", [1, 1, 0, 1]),
]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GNNOME_REFERENCE", "")
    path = os.path.join(ref, "utils", "analyze.py")
    if not os.path.isfile(path):
        raise SystemExit(f"{path} not found: pass the reference checkout")
    spec = importlib.util.spec_from_file_location("reference_analyze", path)
    analyze = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(analyze)

    names = ("read_strand", "read_start", "read_end", "read_chr")
    cols = {n: [row[k] for row in NODES] for k, n in enumerate(names)}
    graph = types.SimpleNamespace(ndata={n: torch.tensor(v, dtype=torch.int64) for n, v in cols.items()})

    def printed(fn, walk):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            fn(graph, walk)
        return buf.getvalue()

    text = [{"strand": printed(analyze.assert_strand, w), "chromosome": printed(analyze.assert_chromosome, w),
             "overlap": printed(analyze.assert_overlap, w)} for _, w in WALKS]
    for kind in ("strand", "chromosome", "overlap"):
        assert any(t[kind] for t in text), f"the reference printed no {kind} finding"
    assert any(not (t["strand"] or t["chromosome"] or t["overlap"]) for t in text), "no walk without output"
    # the two print-only helpers (:41-57), on arguments that are stored with their text
    edges = [[0, 1, 2], [1, 2, 3]]
    info_graph = types.SimpleNamespace(num_nodes=lambda: len(NODES), edges=lambda: (torch.tensor(edges[0]), torch.tensor(edges[1])))
    steps = [{"walk": [4], "current": 4, "neighbors": {"4": [5, 6]}, "actions": [0.25, 0.5], "choice": 6, "best_neighbor": 5},
             {"walk": [4, 6, 2], "current": 2, "neighbors": {"2": []}, "actions": [], "choice": None, "best_neighbor": None}]
    helpers = {"graph_info": {"idx": 3, "num_nodes": len(NODES), "edges": edges}, "prediction": []}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        analyze.print_graph_info(3, info_graph)
    helpers["graph_info"]["text"] = buf.getvalue()
    for step in steps:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            analyze.print_prediction(step["walk"], step["current"], {int(k): v for k, v in step["neighbors"].items()},
                                     torch.tensor(step["actions"], dtype=torch.float64), step["choice"], step["best_neighbor"])
        helpers["prediction"].append(dict(step, text=buf.getvalue()))
    out = {"nodes": cols, "walks": [w for _, w in WALKS], "purpose": [p for p, _ in WALKS], "text": text, "helpers": helpers}
    with open(os.path.join(HERE, "walk_audit.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"walk_audit.json: {len(NODES)} nodes, {len(WALKS)} walks, "
          f"{sum(t[k].count('walk index') for t in text for k in t)} findings")


if __name__ == "__main__":
    main()
