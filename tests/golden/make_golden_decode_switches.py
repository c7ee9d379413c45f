"""Generate tests/golden/g19_decode_switches.pt from the REFERENCE's own decode functions with early_stopping = True.
Build container only:

    python tests/golden/make_golden_decode_switches.py     # needs /root/reference (read-only)

The method of make_golden_decode.py: inference.py imports DGL, so greedy_forwards (:70-111), greedy_backwards_rc (:114-157),
run_greedy_both_ways (:160-164), and for the outer loop get_contig_length, get_subgraph, sample_edges and get_contigs_greedy
(:167-361), are compiled one at a time from the file's syntax tree and executed here with torch in scope - over the graph double
of _graph_double.py for the outer loop.  The module globals they read are set in that scope: early_stopping = True, p_threshold
per run, RANDOM = False (the reference's random stream is torch's CPU generator, step after step; the device draws differently
on purpose, so there is nothing of RANDOM = True to pin).  The reference's text runs, none of it is stored.

Inputs: the graphs of tests/decode_switch_cases.py.  Stored, data only: the graphs (with visited nodes, start edges and the fp32
log-probabilities the walks ranked - torch's CPU log(sigmoid()) may differ in the last bit from one machine to another), and
  walks   per graph and p_threshold, per start edge: walk_f, walk_b, visited_f, visited_b (sorted); sum_f, sum_b as fp32 rows
  outer   per graph and run: seed, len_threshold, nb_paths, p_threshold and the walks get_contigs_greedy returned
Checked before saving: the run with p_threshold = 1e-30 equals the run with early_stopping = False walk for walk, and some
walk stops early in every other run.
"""
import contextlib
import io
import math
import os
import pickle
import sys
import tempfile
import types
from concurrent.futures import ThreadPoolExecutor
from datetime import datetime

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(1, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(1, HERE)

from _graph_double import Graph, dgl  # noqa: E402
from decode_graphs import adversarial_graph  # noqa: E402
from decode_switch_cases import OUTER_CASES, WALK_CASES  # noqa: E402
from make_golden_decode import dicts, reference_functions  # noqa: E402

NAMES = ["get_contig_length", "get_subgraph", "sample_edges", "greedy_forwards", "greedy_backwards_rc", "run_greedy_both_ways",
         "get_contigs_greedy"]


def stored_graph(g):
    assert g["num_nodes"] < 2 ** 15
    return {"src": g["src"].to(torch.int16), "dst": g["dst"].to(torch.int16), "num_nodes": g["num_nodes"], "scores": g["scores"],
            "prefix_length": g["prefix_length"].to(torch.int32), "read_length": g["read_length"].to(torch.int32)}


def main():
    scope = {"torch": torch, "math": math, "os": os, "pickle": pickle, "dgl": dgl, "datetime": datetime,
             "ThreadPoolExecutor": ThreadPoolExecutor, "utils": types.SimpleNamespace(timedelta_to_str=str),
             "RANDOM": False, "early_stopping": True, "p_threshold": 0.06, "DEBUG": False}
    fns = reference_functions(os.path.join(REF, "inference.py"), NAMES, scope)
    run_greedy_both_ways, get_contigs_greedy = fns[5], fns[6]

    def walks_of(g, succs, preds, edges, logProbs):
        out, sums = [], []
        for k in g["starts"]:
            s, d = int(g["src"][k]), int(g["dst"][k])
            walk_f, walk_b, visited_f, visited_b, sum_f, sum_b = run_greedy_both_ways(s, d, logProbs, succs, preds, edges, set(g["visited"]))
            out.append({"edge": k, "walk_f": walk_f, "walk_b": walk_b, "visited_f": sorted(visited_f), "visited_b": sorted(visited_b)})
            sums.append(torch.cat([sum_f, sum_b]))
        return out, torch.stack(sums)

    walk_cases = []
    for name, make, p_thresholds in WALK_CASES:
        g = make()
        succs, preds, edges = dicts(g["src"], g["dst"], g["num_nodes"])
        logProbs = torch.log(torch.sigmoid(g["scores"]))     # inference.py:184
        scope["early_stopping"] = False
        plain, _ = walks_of(g, succs, preds, edges, logProbs)
        scope["early_stopping"] = True
        runs = []
        for p in p_thresholds:
            scope["p_threshold"] = p
            cands, sums = walks_of(g, succs, preds, edges, logProbs)
            shorter = sum(len(a["walk_f"]) + len(a["walk_b"]) < len(b["walk_f"]) + len(b["walk_b"]) for a, b in zip(cands, plain))
            same = all(a["walk_f"] == b["walk_f"] and a["walk_b"] == b["walk_b"] for a, b in zip(cands, plain))
            assert same if p == 1e-30 else shorter >= 1, (name, p, shorter)
            runs.append({"p_threshold": p, "candidates": cands, "sum_f": sums[:, 0].clone(), "sum_b": sums[:, 1].clone()})
            print(name, "E =", g["src"].numel(), "starts", len(cands), "p_threshold", p, "walks cut short:", shorter)
        walk_cases.append({"name": name, **stored_graph(g), "logp": logProbs, "visited": list(g["visited"]), "starts": list(g["starts"]),
                           "runs": runs})

    outer_cases = []
    for name, kw, runs in OUTER_CASES:
        g = adversarial_graph(**kw)
        succs, preds, edges = dicts(g["src"], g["dst"], g["num_nodes"])
        assert len(edges) == g["src"].numel(), "simple graphs only"
        graph = Graph(g["src"], g["dst"], g["num_nodes"], {"read_length": g["read_length"]},
                      {"score": g["scores"], "prefix_length": g["prefix_length"]})
        out = []
        for seed, threshold, nb_paths, p in runs:
            scope["p_threshold"] = p
            torch.manual_seed(seed)
            with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
                walks = get_contigs_greedy(graph, succs, preds, edges, threshold, nb_paths=nb_paths, checkpoint_dir=tmp)
            walks = [[int(x) for x in w] for w in walks]
            out.append({"seed": seed, "len_threshold": threshold, "nb_paths": nb_paths, "p_threshold": p, "walks": walks})
            print(name, "seed", seed, "threshold", threshold, "paths", nb_paths, "p_threshold", p, "->", len(walks), "walks, lengths",
                  [len(w) for w in walks][:12])
        outer_cases.append({"name": name, **stored_graph(g), "runs": out})
    torch.save({"walks": walk_cases, "outer": outer_cases,
                "made_with": "tests/golden/make_golden_decode_switches.py (reference functions via ast, _graph_double.py)",
                "torch": torch.__version__}, os.path.join(HERE, "g19_decode_switches.pt"))


if __name__ == "__main__":
    main()
