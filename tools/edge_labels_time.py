"""Time the ground-truth edge labels (gnnome_amd/labels.py, csrc/edge_labels.hip) on a synthetic positioned-read graph.

    python tools/edge_labels_time.py [--reads 500000] [--reps 3] [--seed 1]

The graph (tests/label_statement.py positioned_read_graph): reads sampled at positions on 2 chromosomes, both genome strands,
each read linked to its next 11 overlapping successors (transitive edges) with both mates of every link, 1 % false links,
coverage gaps and contained reads - about 1M nodes and 10M edges by default.  Reports, as one JSON line: the device time of
labels.edge_labels from events (the whole entry: checks, sorts, views, the loop, the write - it synchronises once inside) and
its host wall time with the inputs already on the device, the per-problem counters from `stats` (passes, accepted components,
forward and backward queue pops), and the wall time of the host statement (tests/label_statement.py, numpy + Python, linear
time) on the same graph, whose labels must equal the device's.  Needs the MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gnnome_amd import labels  # noqa: E402
from label_statement import positioned_read_graph, statement_labels  # noqa: E402

KEYS = ("read_strand", "read_start", "read_end", "read_chr")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    g = positioned_read_graph(args.reads, num_chr=2, seed=args.seed, transitive=11, gaps=200)
    dev = torch.device("cuda", 0)
    src, dst = (torch.from_numpy(g[k]).to(dev) for k in ("src", "dst"))
    node = [torch.from_numpy(np.asarray(g[k])).to(dev) for k in KEYS]
    y, stats = labels.edge_labels(src, dst, g["num_nodes"], *node, return_stats=True)   # warm-up (library load, allocator)
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(args.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        s.record()
        y2 = labels.edge_labels(src, dst, g["num_nodes"], *node)
        e.record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t) * 1e3)
        dev_ms.append(s.elapsed_time(e))
        assert torch.equal(y2, y)
    t = time.perf_counter()
    want = statement_labels(g["src"], g["dst"], g["num_nodes"], *(g[k] for k in KEYS))
    host_ms = (time.perf_counter() - t) * 1e3
    same = bool(np.array_equal(y.cpu().numpy(), want))
    print(json.dumps({"tool": "edge_labels_time", "nodes": g["num_nodes"], "edges": int(g["src"].size), "labelled": int(want.sum()),
                      "device_ms": [round(x, 2) for x in dev_ms], "device_wall_ms": [round(x, 2) for x in wall_ms],
                      "host_statement_ms": round(host_ms, 1), "equal": same, "problems": stats}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
