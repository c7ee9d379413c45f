"""Greedy decode on wide, tied and multi-edge graphs: csrc/decode.hip + gnnome_amd/decode.py against oracle/decode_oracle.py, graph
by graph, on the graphs of tests/decode_graphs.py - successor lists longer than one wave, the switch of torch.topk's tie rule at 64
UNVISITED candidates, ties of every width, parallel edges, self-loops, missing mates, small capacities - and the oracle's outer
loop against the reference's own get_contigs_greedy (tests/golden/g15_decode_outer.pt, made by make_golden_decode.py)."""
import functools
import os
import pickle

import pytest
import torch

from conftest import load_golden
from decode_graphs import CASES, HALF_SCORE_CASES, UNMATED_CASES, adversarial_graph, neighbor_lists
from oracle import decode_oracle as oracle


def dev():
    return torch.device("cuda", 0)


class _Lists(dict):
    """succs with a memory: the length of the successor list the walk looked at last (the oracle reads it once per step)."""
    last = 0

    def __getitem__(self, k):
        v = dict.__getitem__(self, k)
        self.last = len(v)
        return v


@functools.lru_cache(maxsize=None)
def _graph(kind, i):
    g = adversarial_graph(**{"cases": CASES, "unmated": UNMATED_CASES, "half": HALF_SCORE_CASES}[kind][i])
    succs, preds, edges = neighbor_lists(g)
    return g, _Lists(succs), preds, edges, torch.log(torch.sigmoid(g["scores"]))


@functools.lru_cache(maxsize=None)
def _oracle_walks(kind, i):
    """Per start edge of the graph: (walk_f, walk_b, sum_f, sum_b, contig_len or None when the contig has a pair without an edge)."""
    g, succs, preds, edges, logp = _graph(kind, i)
    visited = set(g["visited"])
    out = []
    for k in g["starts"]:
        s, d = int(g["src"][k]), int(g["dst"][k])
        walk_f, walk_b, _, _, sum_f, sum_b = oracle.run_greedy_both_ways(s, d, logp, succs, preds, edges, visited)
        walk = walk_b + walk_f
        whole = all((a, b) in edges for a, b in zip(walk[:-1], walk[1:]))
        out.append((walk_f, walk_b, sum_f.clone(), sum_b.clone(),
                    oracle.contig_length(walk, edges, g["prefix_length"], g["read_length"]) if whole else None))
    return out


# ------------------------------------------------------------------------------------------------ CPU: the generator, the oracle

COVERAGE_CLASSES = ("cand_2_3", "cand_4_63", "cand_ge64", "tie_lt64", "tie_ge64", "list_ge64_cand_lt64_tie", "tie_wider_than_5_lt64",
                    "parallel_step", "start_is_earlier_parallel_copy", "self_loop_start", "mate_lookup_list_gt64", "mate_lookup_list_gt128",
                    "single_successor_excluded", "tie_at_63_candidates", "tie_at_64_candidates", "tie_at_65_candidates")


def test_generator_reaches_every_class_of_ranking_step(monkeypatch):
    """The oracle's walks over the graphs and start edges of the device tests, with a counting hook on torch.topk (what it returns
    is unchanged): at least 20 steps in every class the kernel treats differently."""
    counts = dict.fromkeys(COVERAGE_CLASSES, 0)
    real_topk = torch.topk
    lists = {"cur": None}

    def counting_topk(x, k=1, dim=0):
        n, tied = x.numel(), int((x == x.max()).sum())
        counts["cand_2_3"] += 2 <= n <= 3
        counts["cand_4_63"] += 4 <= n <= 63
        counts["cand_ge64"] += n >= 64
        counts["tie_lt64"] += tied > 1 and n < 64
        counts["tie_ge64"] += tied > 1 and n >= 64
        counts["tie_wider_than_5_lt64"] += tied > 5 and n < 64
        for edge in (63, 64, 65):                      # the switch of the tie rule itself, from both sides
            counts[f"tie_at_{edge}_candidates"] += tied > 1 and n == edge
        counts["list_ge64_cand_lt64_tie"] += tied > 1 and n < 64 and lists["cur"].last >= 64
        return real_topk(x, k=k, dim=dim)

    monkeypatch.setattr(torch, "topk", counting_topk)
    for i in range(len(CASES)):
        g, succs, preds, edges, logp = _graph("cases", i)
        lists["cur"] = succs
        src_l, dst_l = g["src"].tolist(), g["dst"].tolist()
        pairs = {}
        for k in range(len(src_l)):
            pairs[(src_l[k], dst_l[k])] = pairs.get((src_l[k], dst_l[k]), 0) + 1
        for k, (walk_f, walk_b, _, _, _) in zip(g["starts"], _oracle_walks.__wrapped__("cases", i)):   # not the cached ones
            walk = walk_b + walk_f
            counts["parallel_step"] += sum(pairs[(a, b)] > 1 for a, b in zip(walk[:-1], walk[1:]) if (a, b) != (src_l[k], dst_l[k]))
            counts["start_is_earlier_parallel_copy"] += edges[(src_l[k], dst_l[k])] != k
            counts["self_loop_start"] += src_l[k] == dst_l[k]
            # the backward half as walked: cur -> nxt on the other strand; its contig edge (nxt ^ 1, cur ^ 1) is searched in succs[nxt ^ 1]
            for a, b in zip(walk_b[:-1], walk_b[1:]):
                counts["mate_lookup_list_gt64"] += len(dict.__getitem__(succs, a)) > 64
                counts["mate_lookup_list_gt128"] += len(dict.__getitem__(succs, a)) > 128
            for end in (walk_f[-1], walk_b[0] ^ 1):
                lst = dict.__getitem__(succs, end)
                counts["single_successor_excluded"] += len(lst) == 1 and lst[0] in (src_l[k], src_l[k] ^ 1, dst_l[k], dst_l[k] ^ 1)
    monkeypatch.undo()
    print("ranking steps per class:", counts)
    short = {k: v for k, v in counts.items() if v < 20}
    assert not short, short


def test_oracle_outer_loop_equals_the_reference_function():
    """oracle.get_contigs_greedy against walks returned by the reference's own get_contigs_greedy / get_subgraph /
    get_contig_length (compiled from inference.py's syntax tree over a graph double, tests/golden/make_golden_decode.py), walk for
    walk, on graphs with hubs of 64 successors and more, ties, a self-loop that gets sampled and jumped-over nodes.  Parallel edges
    are not in this fixture: how DGL resolves g.edges[u, v] for a pair with several edges is not specified, so there the oracle is
    the project's stated rule (a pair maps to its last id, as the `edges` dict of graph_parser.py:77-80 does)."""
    fx = load_golden("g15_decode_outer.pt")
    assert len(fx["cases"]) >= 3
    for c in fx["cases"]:
        src, dst = c["src"].long(), c["dst"].long()
        for run in c["runs"]:
            torch.manual_seed(run["seed"])
            got = oracle.get_contigs_greedy(src, dst, c["num_nodes"], c["scores"], c["prefix_length"].long(), c["read_length"].long(),
                                            run["len_threshold"], nb_paths=run["nb_paths"])
            assert got == run["walks"], (c["name"], run["seed"], run["len_threshold"], run["nb_paths"])


# ------------------------------------------------------------------------------------------------ GPU: walks, one launch per graph

def _decode_graph(g, **kw):
    from gnnome_amd import decode
    dg = decode.DecodeGraph(g["src"], g["dst"], g["num_nodes"], g["prefix_length"], g["read_length"], device=dev())
    return dg.set_scores(g["scores"], **kw)


def _visited_array(g):
    v = torch.zeros(g["num_nodes"], dtype=torch.uint8, device=dev())
    if g["visited"]:
        v[torch.tensor(g["visited"], device=dev())] = 1
    return v


def _launch(kind, i, **kw):
    from gnnome_amd import decode
    g = _graph(kind, i)[0]
    res = decode.greedy_walks(_decode_graph(g, **kw), _visited_array(g), torch.tensor(g["starts"]))
    return g, {k: getattr(res, k).cpu() for k in ("walks_f", "walks_b", "len_f", "len_b", "sum_f", "sum_b", "contig_len", "status")}


def _assert_walks_equal(kind, i, g, res, sums=True):
    bad = []
    for c, (walk_f, walk_b, sum_f, sum_b, clen) in enumerate(_oracle_walks(kind, i)):
        lf, lb = int(res["len_f"][c]), int(res["len_b"][c])
        got_f, got_b = res["walks_f"][c, :lf].tolist(), (torch.flip(res["walks_b"][c, :lb], [0]) ^ 1).tolist()
        ok = got_f == walk_f and got_b == walk_b and lf == len(walk_f) and lb == len(walk_b)
        if clen is not None:
            ok = ok and int(res["contig_len"][c]) == clen
        if sums:   # the same fp32 log-probabilities added in the same order with plain fp32 adds: the same bits
            ok = ok and torch.equal(res["sum_f"][c:c + 1], sum_f) and torch.equal(res["sum_b"][c:c + 1], sum_b)
        if not ok:
            bad.append((g["starts"][c], got_b, got_f, walk_b, walk_f, int(res["contig_len"][c]), clen))
    assert not bad, (len(bad), bad[0])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)))
def test_hip_walks_equal_the_oracle(i):
    """walks, lengths, contig lengths equal; log-probability sums bit-equal; no status bit.  Start edges that are an earlier copy of a
    parallel pair are among them: the contig length takes the pair's LAST id for the start edge as for every other step
    (DecodeGraph.pair_eid), which is what the oracle's - and the reference's - lookup of (src, dst) gives."""
    g, res = _launch("cases", i)
    assert int(res["status"].max()) == 0
    _assert_walks_equal("cases", i, g, res)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(UNMATED_CASES)))
def test_hip_missing_mates_are_reported(i):
    """status & 2 exactly for the candidates whose backward half walks an edge without a mate; the walks are still the oracle's;
    decode_contigs refuses such a graph."""
    from gnnome_amd import decode
    g, res = _launch("unmated", i)
    want = torch.tensor([2 if w[4] is None else 0 for w in _oracle_walks("unmated", i)])
    assert int(want.sum()) > 0
    assert torch.equal(res["status"].long(), want)
    _assert_walks_equal("unmated", i, g, res)
    gone = set(g["visited"])
    remaining = [k for k, (s, d) in enumerate(zip(g["src"].tolist(), g["dst"].tolist())) if s not in gone and d not in gone]
    first = next(remaining.index(k) for k, st in zip(g["starts"], want.tolist()) if st and k in remaining)
    with pytest.raises(RuntimeError, match="mate"):
        decode.decode_contigs(_decode_graph(g), 0, nb_paths=1, sampler=lambda prob, k: torch.tensor([first]), visited=_visited_array(g))


@pytest.mark.gpu
@pytest.mark.parametrize("i,cap", [(1, 3), (5, 2), (7, 2)])
def test_hip_small_capacity_is_reported(i, cap):
    """capacity smaller than a walk: status & 1 and the first `capacity` nodes of the oracle's walk.  (A cut forward half has visited
    less than the oracle's, so the backward half is compared only where the forward half fitted.)"""
    from gnnome_amd import decode
    g = _graph("cases", i)[0]
    res = decode.greedy_walks(_decode_graph(g), _visited_array(g), torch.tensor(g["starts"]), capacity=cap)
    cut = 0
    for c, (walk_f, walk_b, _, _, _) in enumerate(_oracle_walks("cases", i)):
        lf, lb, st = int(res.len_f[c]), int(res.len_b[c]), int(res.status[c])
        assert lf == min(len(walk_f), cap) and res.walks_f[c, :lf].tolist() == walk_f[:cap]
        if len(walk_f) > cap:
            assert st & 1
            cut += 1
        else:
            back = [w ^ 1 for w in reversed(walk_b)]       # as walked
            assert lb == min(len(back), cap) and res.walks_b[c, :lb].tolist() == back[:cap]
            assert bool(st & 1) == (len(back) > cap)
            cut += len(back) > cap
    assert cut >= 10


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(HALF_SCORE_CASES)))
def test_hip_walks_with_logprobs_on_device(i):
    """logprobs_on_device=True: log(sigmoid()) by the device's libm may differ from the CPU's in the last bit, which could reorder a
    near-tie.  So the inputs are restricted: inside any one successor list a score is either saturated (>= 20: exactly 0 on both
    sides) or a distinct multiple of 0.5 in [-80, 10] - gaps of thousands of ulps, no denormal sigmoid.  Then the walks and contig
    lengths are the oracle's; the sums are not compared."""
    g, res = _launch("half", i, logprobs_on_device=True)
    assert int(res["status"].max()) == 0
    _assert_walks_equal("half", i, g, res, sums=False)


# ------------------------------------------------------------------------------------------------ GPU: the outer loop

def _outer(g, threshold, nb_paths, seed, **kw):
    from gnnome_amd import decode
    torch.manual_seed(seed)
    trace = []
    want = oracle.get_contigs_greedy(g["src"], g["dst"], g["num_nodes"], g["scores"], g["prefix_length"], g["read_length"], threshold,
                                     nb_paths=nb_paths, trace=trace)
    torch.manual_seed(seed)
    stats = []
    got = decode.decode_contigs(_decode_graph(g), threshold, nb_paths=nb_paths, sampler=decode.sample_edges, stats=stats, **kw)
    assert got == want
    assert [s["contig_len"] for s in stats] == [t["contig_len"] for t in trace]
    assert [s["walk_len"] for s in stats] == [t["walk_len"] for t in trace]
    return got, trace


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 2, 5, 7, 11, 16, 17, 18, 21, 25, 26, 27, 29])
@pytest.mark.parametrize("nb_paths", [1, 8])
def test_hip_outer_loop_equals_the_oracle_on_adversarial_graphs(i, nb_paths):
    """decode_contigs against oracle.get_contigs_greedy, same seed, the reference's sampler: threshold 0 consumes the graph, 40 000
    stops somewhere in between, 10^9 stops at the first iteration."""
    g = _graph("cases", i)[0]
    got, trace = _outer(g, 0, nb_paths, seed=7 + i)
    assert len(got) == len(trace) >= 3
    _outer(g, 40_000, nb_paths, seed=8 + i)
    got, trace = _outer(g, 10 ** 9, nb_paths, seed=9 + i)
    assert got == [] and len(trace) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("i", [2, 16, 20, 24])
def test_hip_outer_loop_equals_the_oracle_at_100_paths(i):
    g = _graph("cases", i)[0]
    _outer(g, 0, 100, seed=3 + i)
    _outer(g, 60_000, 100, seed=4 + i)


class _G:
    def __init__(self, g, **edata):
        self.g, self.ndata, self.edata = g, {"read_length": g["read_length"]}, {"prefix_length": g["prefix_length"], **edata}

    def edges(self):
        return self.g["src"], self.g["dst"]

    def num_nodes(self):
        return self.g["num_nodes"]


@pytest.mark.gpu
@pytest.mark.parametrize("i", [1, 17, 25])
def test_hip_get_contigs_greedy_with_labels(i):
    """use_labels=True: the scores are 0 / 1 labels floored at 1e-9 (inference.py:178-181), so every list is one wide tie."""
    from gnnome_amd import decode
    g = _graph("cases", i)[0]
    y = (g["scores"] > 0).float()
    for threshold, nb_paths in ((0, 6), (50_000, 20)):
        torch.manual_seed(i)
        want = oracle.get_contigs_greedy(g["src"], g["dst"], g["num_nodes"], y, g["prefix_length"], g["read_length"], threshold,
                                         nb_paths=nb_paths, use_labels=True)
        torch.manual_seed(i)
        got = decode.get_contigs_greedy(_G(g, y=y), None, None, None, threshold, nb_paths=nb_paths, use_labels=True)
        assert got == want and (threshold or len(got) >= 3)


def _largest(prob, k):
    """A sampler that is a function of the remaining probabilities only: the k largest, first index first among equals."""
    return torch.argsort(prob.cpu(), descending=True, stable=True)[:k]


class _Interrupt(Exception):
    pass


@pytest.mark.gpu
def test_hip_resumed_decode_continues_the_interrupted_one(tmp_path):
    """A run interrupted right after the checkpoint of contig 20 was written, then resumed with load_checkpoint=True, returns the
    walks of the uninterrupted run (which are the oracle's)."""
    from gnnome_amd import decode
    g = adversarial_graph(seed=700, hubs=("d64", "mid", "d3", "d4"), reads=400, parallel=0.05)
    want = oracle.get_contigs_greedy(g["src"], g["dst"], g["num_nodes"], g["scores"], g["prefix_length"], g["read_length"], 0,
                                     nb_paths=8, sampler=_largest)
    assert len(want) >= 25
    dg = _decode_graph(g)
    whole = decode.decode_contigs(dg, 0, nb_paths=8, sampler=_largest)
    assert whole == want
    ckpt = tmp_path / "checkpoint.pkl"

    def until_20(prob, k):
        if ckpt.is_file():
            with open(ckpt, "rb") as f:
                if len(pickle.load(f)["walks"]) == 20:
                    raise _Interrupt
        return _largest(prob, k)

    with pytest.raises(_Interrupt):
        decode.decode_contigs(dg, 0, nb_paths=8, sampler=until_20, checkpoint_dir=str(tmp_path))
    with open(ckpt, "rb") as f:
        state = pickle.load(f)
    assert state["walks"] == want[:20] and len(state["all_contigs_len"]) == 20
    calls = []

    def counting(prob, k):
        calls.append(int(prob.numel()))
        return _largest(prob, k)

    resumed = decode.decode_contigs(dg, 0, nb_paths=8, sampler=counting, checkpoint_dir=str(tmp_path), load_checkpoint=True)
    assert resumed == want
    assert len(calls) == len(want) - 20     # it went on from contig 20, it did not start again
    assert not os.path.exists(tmp_path / "checkpoint_tmp.pkl")


# ------------------------------------------------------------------------------------------------ GPU: gnnome_mark_walk_visited

def _marked(walk, succs, preds):
    """inference.py:317-322 with the walk's own nodes: nodes, mates, succs[ss] & preds[dd] for consecutive pairs, their mates."""
    out = set(walk) | {w ^ 1 for w in walk}
    for ss, dd in zip(walk[:-1], walk[1:]):
        t1 = set(succs[ss]) & set(preds[dd])
        out |= t1 | {t ^ 1 for t in t1}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("i", [1, 5, 7, 9, 14, 18, 21, 23, 29])
def test_hip_mark_walk_visited_equals_the_set_expression(i):
    """Walks of the oracle and random edge-following walks through the hubs (p -> hub -> successor, and p -> successor where the
    hub is jumped over: succs[ss] and the lists of its members longer than 64 and 128), onto an empty and a partly filled array."""
    from gnnome_amd import decode
    g, succs, preds, edges, _ = _graph("cases", i)
    dg = _decode_graph(g)
    gen = torch.Generator().manual_seed(i)
    walks = [w[1] + w[0] for w in _oracle_walks("cases", i)[::7]]
    for h in g["hubs"]:
        for p in sorted(set(preds[h])):
            for step in (h, None):
                walk = [p] if step is None else [p, h]
                for _ in range(int(torch.randint(1, 12, (1,), generator=gen))):
                    nxt = succs[walk[-1]]
                    if not nxt:
                        break
                    walk.append(nxt[int(torch.randint(0, len(nxt), (1,), generator=gen))])
                walks.append(walk)
    wide = sum(1 for w in walks for ss in w[:-1] if len(succs[ss]) > 128 or any(len(succs[t]) > 128 for t in succs[ss]))
    jumped = 0
    for k, walk in enumerate(walks):
        start = torch.zeros(g["num_nodes"], dtype=torch.uint8)
        if k % 2:
            start[torch.randperm(g["num_nodes"], generator=gen)[:g["num_nodes"] // 5]] = 1
        want = start.clone()
        marked = _marked(walk, succs, preds)
        jumped += len(marked) > len(set(walk) | {w ^ 1 for w in walk})
        want[torch.tensor(sorted(marked))] = 1
        got = start.to(dev())
        decode.mark_walk_visited(dg, got, torch.tensor(walk))
        assert torch.equal(got.cpu(), want), (k, walk)
    assert jumped >= 5 and (wide >= 5 or max(len(succs[h]) for h in g["hubs"]) <= 128)


# ------------------------------------------------------------------------------------------------ GPU: sample_edges_device

@pytest.mark.gpu
def test_hip_sample_edges_device_deterministic_properties():
    """Only what does not depend on chance: the same seed gives the same draws, every index is in range, a one-hot distribution
    (weight 1 against the 1e-9 floor of three other edges: a draw lands elsewhere with probability 3e-9) returns its index for every
    draw, also when that index is the first or the last one, and the last index is never exceeded."""
    from gnnome_amd import decode
    g = _graph("cases", 1)[0]
    prob = torch.sigmoid(g["scores"]).to(dev())
    prob[::3] = 0.0
    draws = []
    for _ in range(2):
        torch.manual_seed(11)
        draws.append(decode.sample_edges_device(prob, 100))
    assert torch.equal(draws[0], draws[1])
    assert draws[0].shape == (100,) and int(draws[0].min()) >= 0 and int(draws[0].max()) < prob.numel()
    for hot in (0, 1, 3):
        one = torch.zeros(4, device=dev())
        one[hot] = 1.0
        torch.manual_seed(hot)
        got = decode.sample_edges_device(one, 100)
        assert got.tolist() == [hot] * 100
    torch.manual_seed(2)
    assert decode.sample_edges_device(torch.ones(1, device=dev()), 50).tolist() == [0] * 50
