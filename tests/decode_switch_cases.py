"""Graphs and runs for the decoder switches (early stopping, random walks): shared by tests/golden/make_golden_decode_switches.py,
which runs the reference's own functions over them, and by tests/test_decode_switches_host.py / test_decode_switches.py.

gadget_graph(): a hand-made graph of 28 reads whose junctions are the boundary cases of early stopping at p_threshold = 0.06,
one per gadget (the numbers are READS: read r is node 2r, its reverse complement 2r + 1; every edge has its mate; HI = likely, LO = improbable, AT = the score whose fp32
log(sigmoid()) EQUALS fp32(log(0.06)) - asserted where the graph is built):

    exact      0 -> 1 -> {2: AT, 3: LO}, 2 -> 4           one successor exactly at the threshold: not "below", the walk goes on to 2
    single     5 -> 6 -> 7 (LO, the only successor) -> 8  a list of length 1 never stops: the walk reaches 8
    masked     9 -> 10 -> {11: HI but visited, 12: LO}    a list of length 2 that masking cuts to one improbable successor: stop at 10
    all_low    13 -> 14 -> {15: LO, 16: LO}               stop at 14
    both       22, 23 -> 18 -> 19 -> {20: LO, 21: LO}     the mates 18^1 -> 22^1, 23^1 are LO: from the start edge (18, 19) both
                                                          halves stop; 17 -> 13 gives a backward half that does not
    two_nodes  24 -> 25                                   a walk of two nodes;  loop  26 -> 26  a self-loop start edge

WALK_CASES: (name, graph, p_thresholds).  The adversarial graphs are those of tests/decode_graphs.py: hubs with more than 64
successors, ties, parallel edges, self-loops.  1e-30 is the threshold so low that nothing stops.
"""
import functools
import math

import numpy as np
import torch

import decode_switch_statement as st
from decode_graphs import adversarial_graph
from oracle import decode_oracle as oracle

AT_006 = float(np.float32(-2.751535415649414))      # log(sigmoid(AT_006)) == fp32(log(0.06)) in torch's fp32 CPU kernels
HI, LO = 3.0, -6.0


def gadget_graph():
    rows = []

    def add(a, b, score, mate_score=None):
        u, v = 2 * a, 2 * b
        rows.append((u, v, score))
        if (v ^ 1, u ^ 1) != (u, v):
            rows.append((v ^ 1, u ^ 1, score if mate_score is None else mate_score))

    add(0, 1, HI), add(1, 2, AT_006), add(1, 3, LO), add(2, 4, HI)
    add(5, 6, HI), add(6, 7, LO), add(7, 8, HI)
    add(9, 10, HI), add(10, 11, HI), add(10, 12, LO)
    add(17, 13, HI), add(13, 14, HI), add(14, 15, LO), add(14, 16, LO - 1)
    add(18, 19, HI), add(19, 20, LO), add(19, 21, LO - 1), add(22, 18, HI, LO), add(23, 18, HI, LO - 1)
    add(24, 25, HI)
    rows.append((52, 52, HI)), rows.append((53, 53, HI))
    reads = 28
    rng = np.random.default_rng(19)
    perm = rng.permutation(len(rows))
    src = torch.tensor([rows[i][0] for i in perm], dtype=torch.int64)
    dst = torch.tensor([rows[i][1] for i in perm], dtype=torch.int64)
    scores = torch.tensor([rows[i][2] for i in perm], dtype=torch.float32)
    at = torch.log(torch.sigmoid(torch.tensor([AT_006], dtype=torch.float32)))
    assert float(at) == float(torch.tensor(math.log(0.06), dtype=torch.float32)) and float(at) < math.log(0.06)
    read_length = torch.from_numpy(np.repeat(rng.integers(5000, 30000, size=reads), 2).astype(np.int64))
    prefix_length = torch.from_numpy(rng.integers(100, 5000, size=len(rows)).astype(np.int64))
    visited = [22, 23]                                 # read 11, both strands
    starts = [k for k in range(len(rows)) if int(src[k]) not in visited and int(dst[k]) not in visited]
    return {"src": src, "dst": dst, "num_nodes": 2 * reads, "scores": scores, "prefix_length": prefix_length, "read_length": read_length,
            "visited": visited, "hubs": [], "starts": starts, "unmated": []}


def _adv(max_starts=160, **kw):
    g = adversarial_graph(**kw)
    g["starts"] = g["starts"][:max_starts]
    return g


WALK_CASES = [
    ("gadgets", gadget_graph, (0.06,)),
    ("small_hubs", lambda: _adv(seed=1901, hubs=("d2", "d3", "d4", "mid"), reads=40, self_loops=3), (0.06, 0.5, 1e-30)),
    ("wide_hubs", lambda: _adv(seed=1902, hubs=("d65", "wide", "d64"), reads=110, self_loops=2), (0.06, 0.95, 1e-30)),
    ("parallel", lambda: _adv(seed=1903, hubs=("mid", "d65"), reads=50, parallel=0.3, hub_parallel=True), (0.06, 0.9)),
    ("wide_open", lambda: _adv(seed=1904, hubs=("wide", "d65"), reads=110, visit=False, max_starts=120), (0.06,)),
]

# (name, graph kwargs (simple graphs: the reference's outer loop looks pairs up in DGL), [(seed, len_threshold, nb_paths, p_threshold)])
OUTER_CASES = [
    ("outer_small", dict(seed=1911, hubs=("d2", "d3", "d4", "mid"), reads=40, self_loops=4, parallel=0.0),
     [(1, 0, 8, 0.06), (2, 30_000, 8, 0.5), (3, 0, 1, 0.95)]),
    ("outer_wide", dict(seed=1912, hubs=("d65", "wide"), reads=60, self_loops=4, parallel=0.0),
     [(4, 0, 30, 0.06), (5, 0, 6, 0.95), (6, 0, 6, 1e-30)]),
]


# (case, early_stopping, p_threshold, seed) of the random-mode comparisons; seeds on both sides of 2^63 (the C entry takes an int64)
RANDOM_RUNS = [("wide_hubs", False, 0.06, 0), ("wide_hubs", True, 0.06, 12345), ("wide_hubs", False, 0.06, 2 ** 63 + 5),
               ("small_hubs", True, 0.5, 7), ("parallel", False, 0.06, 2 ** 64 - 1), ("gadgets", True, 0.06, 3),
               ("wide_open", False, 0.06, 5), ("wide_open", True, 0.06, 2 ** 62)]


@functools.lru_cache(maxsize=None)
def case(name):
    make = {n: m for n, m, _ in WALK_CASES}[name]
    g = make()
    succs, preds, edges = oracle.neighbor_dicts(g["src"], g["dst"], g["num_nodes"])
    return g, succs, preds, edges, torch.log(torch.sigmoid(g["scores"]))


@functools.lru_cache(maxsize=None)
def statement_walks(name, early_stopping, p_threshold, random_walks, seed):
    """Per start edge (candidate index = its position): (walk_f, walk_b, visited_f, visited_b, sum_f, sum_b, events)."""
    g, succs, preds, edges, logp = case(name)
    sw = st.Switches(early_stopping, p_threshold, random_walks, seed)
    out = []
    for c, k in enumerate(g["starts"]):
        events = {"f": [], "b": []}
        r = st.run_greedy_both_ways(int(g["src"][k]), int(g["dst"][k]), logp, succs, preds, edges, set(g["visited"]), sw, c, events)
        out.append(r + (events,))
    return out
