"""Seeded generator of adversarial graphs for the greedy decode (tests/test_decode_adversarial.py; the fixture
tests/golden/g15_decode_outer.pt is made from it by tests/golden/make_golden_decode.py).

`adversarial_graph(seed, ...)` returns the dict of make_golden_decode.decode_graph (src, dst, num_nodes, scores,
prefix_length, read_length) plus what the tests need to aim at the interesting places:

    visited     sorted node ids (whole read pairs) that cut the hubs' unvisited successors to a chosen count
    hubs        the hub nodes
    starts      edge ids to start walks from: every in- and out-edge of a hub and of a hub's mate, the out-edges of the hubs'
                successors (their backward halves enter the hub's mate, so the mate lookup searches the hub's list), every copy of
                a parallel pair, every self-loop, the gadgets, and a random sample of the rest
    unmated     edge ids whose reverse-complement mate was left out (only with unmated > 0); they score high, and the out-edges
                of their tails' mates are start edges, so that backward halves walk them

What it mixes (all optional, all seeded):

    hubs        nodes with a chosen number of DISTINCT successors, by class (HUB_CLASSES): 2, 3, 4, 5-63, exactly 63 / 64 / 65,
                100-200 and more than 256; every edge (u, v) gets its mate (v ^ 1, u ^ 1), so a hub's mate has as many predecessors
    ties        per hub: `k` of its edges saturated (score >= 20: sigmoid rounds to 1.0f and the log-probability is exactly 0),
                or `k` edges sharing one non-saturated maximum, or a unique maximum; k from 2 up to the list length; elsewhere a
                fraction of saturated scores and repeated values
    visited     per hub the number of successors left unvisited is drawn from 0, 1, 2, 3, 62 .. 66 and "all"
    exact       extra hubs (eight predecessors each, no parallel copies) whose unvisited successors number EXACTLY the given counts
                and tie for the maximum: walks that start on an in-edge rank exactly that many candidates (63 / 64 / 65: the two
                sides of the switch of torch.topk's tie rule)
    parallel    2-4 copies of a pair (with hub_parallel in the hubs' lists too), each with its own score and prefix length, scattered in edge-id order
    self-loops  (u, u) with the mate (u ^ 1, u ^ 1)
    backbone    a layout chain with out-degree 0-3 (dead ends), long-range edges and edges back to earlier reads (cycles)
    gadgets     a -> b whose only successor is a again; c -> d whose only successor is c ^ 1
    half_scores scores inside any one successor list are either saturated or distinct multiples of 0.5 in [-80, 10]
"""
import numpy as np
import torch

HUB_CLASSES = {"d2": (2, 2), "d3": (3, 3), "d4": (4, 4), "mid": (5, 63), "d63": (63, 63), "d64": (64, 64), "d65": (65, 65),
               "wide": (100, 200), "huge": (257, 300)}
_UNVISITED_TARGETS = (0, 1, 2, 3, 62, 63, 64, 65, 66)


def adversarial_graph(seed, hubs=("d3", "mid", "d64"), reads=None, parallel=0.12, hub_parallel=False, self_loops=2, unmated=0,
                      visit=True, half_scores=False, saturate=0.1, other_starts=40, exact=()):
    rng = np.random.default_rng(seed)
    degs = [int(rng.integers(HUB_CLASSES[h][0], HUB_CLASSES[h][1] + 1)) for h in hubs]
    degs += [int(u) + int(rng.integers(0, 40)) for u in exact]   # `exact` hubs: exactly u successors stay unvisited, tied maximum
    hubs = tuple(hubs) + tuple(f"exact{u}" for u in exact)
    if reads is None:
        reads = int(rng.integers(30, 90))
    reads = max(reads, 12, (max(degs, default=0) + 1) // 2 + 8, max(degs[len(degs) - len(exact):], default=0) + 16)
    n = 2 * reads
    body = reads - 4                                   # the last four reads belong to the gadgets
    primary = []                                       # (u, v): one strand's edge; the mate follows unless left out
    seen = set()

    def add(u, v):
        if (u, v) in seen or (v ^ 1, u ^ 1) in seen or u == (v ^ 1):
            return False
        seen.add((u, v))
        primary.append((u, v))
        return True

    for r in range(body):                              # backbone: layout chain on a random strand
        for off in range(1, 1 + int(rng.integers(0, 4))):
            t = r + off
            if t < body:
                s = int(rng.integers(0, 2))
                add(2 * r + s, 2 * t + s) if s == 0 else add(2 * t + s, 2 * r + s)
    for _ in range(max(2, body // 8)):                 # long-range edges, in either direction: cycles
        a, b = int(rng.integers(0, body)), int(rng.integers(0, body))
        if a != b:
            add(2 * a + int(rng.integers(0, 2)), 2 * b + int(rng.integers(0, 2)))
    hub_nodes = list(rng.choice(2 * body, size=len(hubs), replace=False)) if hubs else []
    hub_nodes = [int(h) for h in hub_nodes]
    protected = set()
    for h in hub_nodes:
        protected |= {h, h ^ 1}
    for g_ in range(2 * body, n):
        protected.add(g_)
    hub_targets = {}
    for h, deg in zip(hub_nodes, degs):
        have = {v for (u, v) in seen if u == h} | {u ^ 1 for (u, v) in seen if (v ^ 1) == h}
        pool = [x for x in range(2 * body) if x not in (h, h ^ 1) and x not in have]
        if deg - len(have) <= (body - 1 - len(have)):    # distinct reads where the graph is large enough
            rd = rng.permutation(sorted({x >> 1 for x in pool} - {x >> 1 for x in have}))
            pick = [2 * int(r) + int(rng.integers(0, 2)) for r in rd]
            in_pool = set(pool)
            pick = [x for x in pick if x in in_pool]
        else:
            pick = [int(x) for x in rng.permutation(pool)]
        for x in pick:
            if len(have) >= deg:
                break
            if add(h, x):
                have.add(x)
        hub_targets[h] = sorted(have)
        is_exact = exact and h in hub_nodes[len(hub_nodes) - len(exact):]
        target_reads = {x >> 1 for x in have}
        added = 0
        for _ in range(60 if is_exact else int(rng.integers(2, 6))):   # predecessors, so that walks arrive at the hub; some also
            p = int(rng.integers(0, 2 * body))                        # reach a few of its successors directly, which makes the hub
            if p in (h, h ^ 1) or (is_exact and ((p >> 1) in target_reads or p in protected or added >= 8)):   # a jumped-over node
                continue
            if add(p, h):
                added += 1
                for x in rng.choice(hub_targets[h], size=min(3, len(hub_targets[h])), replace=False):
                    if int(x) not in (p, p ^ 1) and not is_exact:
                        add(p, int(x))
    for _ in range(self_loops):
        u = int(rng.integers(0, 2 * body))
        add(u, u)
    a, b, c, d = 2 * body, 2 * body + 2, 2 * body + 4, 2 * body + 6
    gadget = [(a, b), (b, a), (c, d), (d, c ^ 1)]
    for u, v in gadget:
        add(u, v)
    add(int(rng.integers(0, 2 * body)), a)             # a way in

    # copies per pair, mates, which mates are left out
    plain = [k for k, (u, v) in enumerate(primary) if u != v and (u, v) not in gadget]
    copies = np.ones(len(primary), dtype=np.int64)
    if parallel > 0:
        for k in plain:
            if (hub_parallel or not ({primary[k][0], primary[k][1] ^ 1} & set(hub_nodes))) and rng.random() < parallel:
                copies[k] = int(rng.integers(2, 5))
    dropped = set()
    if unmated:
        single = [k for k in plain if copies[k] == 1]
        dropped = {int(k) for k in rng.choice(single, size=min(unmated, len(single)), replace=False)}
    edge_list, lonely = [], []
    for k, (u, v) in enumerate(primary):
        for _ in range(int(copies[k])):
            edge_list.append((u, v))
            if k in dropped:
                lonely.append(len(edge_list) - 1)
            elif (v ^ 1, u ^ 1) != (u, v):
                edge_list.append((v ^ 1, u ^ 1))
    perm = rng.permutation(len(edge_list))
    where = {int(p): i for i, p in enumerate(perm)}
    src = torch.tensor([edge_list[i][0] for i in perm], dtype=torch.int64)
    dst = torch.tensor([edge_list[i][1] for i in perm], dtype=torch.int64)
    e = len(edge_list)
    src_l, dst_l = src.tolist(), dst.tolist()

    # scores, successor list by successor list
    scores = rng.normal(0.0, 4.0, size=e).astype(np.float32)
    hot = rng.random(e) < saturate
    scores[hot] = rng.uniform(20.0, 40.0, size=int(hot.sum())).astype(np.float32)
    rep = rng.random(e) < 0.1                            # repeated non-saturated values anywhere
    scores[rep] = rng.choice(np.array([-2.0, 0.25, 1.5, 3.0], dtype=np.float32), size=int(rep.sum()))
    lists = {}
    for k in range(e):
        lists.setdefault(src_l[k], []).append(k)
    for h in hub_nodes + [h ^ 1 for h in hub_nodes]:
        ids = lists.get(h, [])
        if len(ids) < 2:
            continue
        deg = len(ids)
        mode = ("sat", "rep", "sat", "none")[int(rng.integers(0, 4))]
        width = int(rng.choice([2, 3, int(rng.integers(2, deg + 1)), max(2, deg - 1), deg, max(2, deg // 2)]))
        width = min(width, deg)
        scores[ids] = rng.uniform(-9.0, 2.0, size=deg).astype(np.float32)
        low = rng.random(deg) < 0.2                     # a repeated value below the maximum
        scores[np.asarray(ids)[low]] = -1.0
        if mode != "none":
            tied = rng.choice(np.asarray(ids), size=width, replace=False)
            scores[tied] = rng.uniform(20.0, 40.0, size=width).astype(np.float32) if mode == "sat" else np.float32(2.5)
    read_len = rng.integers(5000, 30000, size=reads)
    read_length = torch.from_numpy(np.repeat(read_len, 2).astype(np.int64))
    prefix_length = torch.from_numpy(rng.integers(100, 30000, size=e).astype(np.int64))   # per COPY: parallel copies differ

    # visited: whole read pairs, chosen among each hub's successors
    visited = set()
    n_exact = len(exact)
    if visit:
        for j, h in enumerate(hub_nodes):
            tg = [t for t in hub_targets[h] if t not in protected and (t ^ 1) not in protected]
            deg = len(hub_targets[h])
            options = [t for t in _UNVISITED_TARGETS if t <= deg] + [deg, deg]
            want = int(options[int(rng.integers(0, len(options)))])
            if j >= len(hub_nodes) - n_exact:
                want = int(exact[j - (len(hub_nodes) - n_exact)])
            for t in rng.permutation(tg):
                left = sum(1 for x in hub_targets[h] if x not in visited)
                if left <= want:
                    break
                visited |= {int(t), int(t) ^ 1}
    for h in hub_nodes[len(hub_nodes) - n_exact:]:      # exact hubs: a tie for the maximum among the UNVISITED successors, of any
        ids = np.asarray(lists[h])                      # width; visited successors score higher still (they must not be ranked)
        live = np.asarray([k for k in ids if dst_l[k] not in visited])
        scores[ids] = rng.uniform(-9.0, 2.0, size=ids.size).astype(np.float32)
        scores[[k for k in ids if dst_l[k] in visited]] = 45.0
        width = int(rng.choice([2, 3, int(rng.integers(2, live.size + 1)), live.size - 1, live.size]))
        tied = rng.choice(live, size=min(max(width, 2), live.size), replace=False)
        scores[tied] = rng.uniform(20.0, 40.0, size=tied.size).astype(np.float32) if rng.random() < 0.5 else np.float32(2.5)
    if half_scores:
        grid = np.arange(-80.0, 10.5, 0.5, dtype=np.float32)
        for u, ids in lists.items():
            ids = np.asarray(ids)
            keep_hot = scores[ids] >= 20.0
            cold = ids[~keep_hot]
            if cold.size > grid.size:                   # more edges than grid values: the surplus saturates
                extra = cold[grid.size:]
                scores[extra] = rng.uniform(20.0, 40.0, size=extra.size).astype(np.float32)
                cold = cold[:grid.size]
            scores[cold] = rng.choice(grid, size=cold.size, replace=False)


    lonely_ids = sorted(where[i] for i in lonely)
    for k in lonely_ids:                                # an edge without a mate is a likely choice of the walks through its tail
        scores[k] = 30.0
        visited -= {src_l[k], src_l[k] ^ 1, dst_l[k], dst_l[k] ^ 1}

    # start edges
    pair_count = {}
    for k in range(e):
        pair_count[(src_l[k], dst_l[k])] = pair_count.get((src_l[k], dst_l[k]), 0) + 1
    near = set()
    for h in hub_nodes:
        near |= {h, h ^ 1}
    succ_of_hub = set()
    for h in hub_nodes:
        succ_of_hub |= set(hub_targets[h])
    starts = []
    for k in range(e):
        u, v = src_l[k], dst_l[k]
        if u in near or v in near or pair_count[(u, v)] > 1 or u == v or u >= 2 * body or v >= 2 * body:
            starts.append(k)
    behind_lonely = {src_l[k] ^ 1 for k in lonely_ids}   # backward halves from these tails start at the lonely edge's tail
    starts += [k for k in range(e) if src_l[k] in behind_lonely]
    taken = set(starts)
    from_succ = [k for k in range(e) if src_l[k] in succ_of_hub and k not in taken]
    taken |= set(from_succ)
    rest = [k for k in range(e) if k not in taken]
    for pool, cnt in ((from_succ, 3 * other_starts), (rest, other_starts)):
        if pool:
            starts += [int(x) for x in rng.choice(pool, size=min(cnt, len(pool)), replace=False)]
    return {"src": src, "dst": dst, "num_nodes": n, "scores": torch.from_numpy(scores), "prefix_length": prefix_length,
            "read_length": read_length, "visited": sorted(visited), "hubs": hub_nodes, "starts": sorted(set(starts)),
            "unmated": lonely_ids}


# The graphs of the device tests (and of the CPU coverage test, which proves that they reach what they are for).
CASES = (
    [dict(seed=100 + i, hubs=h) for i, h in enumerate([
        ("d2", "d3", "d4"), ("d3", "mid", "d64"), ("d63", "d64", "d65"), ("d64", "d65", "mid"), ("d63", "d65", "d4"),
        ("wide", "d64"), ("wide", "mid", "d3"), ("huge",), ("huge", "d65"), ("wide", "wide"), ("d64", "d64", "d64"),
        ("d65", "d65", "mid", "mid"), ("mid", "mid", "mid", "d2"), ("d63", "d63", "wide"), ("huge", "wide"), ()])]
    + [dict(seed=200 + i, hubs=h, parallel=0.3, hub_parallel=True) for i, h in enumerate([
        ("d64", "mid"), ("d65", "d3"), ("wide",), ("mid", "mid", "d4"), ("d63", "d64"), ("huge",)])]
    + [dict(seed=300 + i, hubs=h, visit=False) for i, h in enumerate([("d64", "d65"), ("wide", "d63"), ("mid", "d4", "d2")])]
    + [dict(seed=400 + i, hubs=h, parallel=0.0, self_loops=4) for i, h in enumerate([("d64", "mid"), ("d3", "d4", "mid")])]
    + [dict(seed=450 + i, hubs=h, exact=x) for i, (h, x) in enumerate([
        (("d3",), (63, 64, 65)), (("mid",), (64, 63, 65)), ((), (65, 64, 63, 62, 66)), (("d4",), (63, 64, 65)),
        (("d2", "d3"), (64, 65, 63)), ((), (63, 63, 64, 64, 65, 65))])]
)
UNMATED_CASES = [dict(seed=500 + i, hubs=h, unmated=10, parallel=0.0) for i, h in enumerate([("mid", "d64"), ("d3", "d4"), ("wide",)])]
HALF_SCORE_CASES = [dict(seed=600 + i, hubs=h, half_scores=True, saturate=0.2) for i, h in enumerate(
    [("d64", "mid"), ("wide", "d65"), ("d63", "d3", "d4"), ("huge",)])]


def neighbor_lists(g):
    """succs / preds / edges as graph_parser.py:31-37, :55-58, :77-80 build them (lists in edge-id order, a pair -> its LAST id)."""
    n = g["num_nodes"]
    succs = {i: [] for i in range(n)}
    preds = {i: [] for i in range(n)}
    edges = {}
    for idx, (s, d) in enumerate(zip(g["src"].tolist(), g["dst"].tolist())):
        succs[s].append(d)
        preds[d].append(s)
        edges[(s, d)] = idx
    return succs, preds, edges
