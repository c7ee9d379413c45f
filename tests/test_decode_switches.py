"""The decoder switches on the device: gnnome_greedy_walks_opts (csrc/decode.hip) and the keywords of gnnome_amd/decode.py and
pipeline.py against the statement (tests/decode_switch_statement.py) and against walks of the reference's own functions
(tests/golden/g19_decode_switches.pt).  Everything compared is an integer or an fp32 sum accumulated in walk order: exact."""
import ctypes
import math
import pickle

import pytest
import torch

import decode_switch_statement as st
from conftest import load_golden
from decode_graphs import CASES, adversarial_graph
from decode_switch_cases import OUTER_CASES, RANDOM_RUNS, WALK_CASES, case, statement_walks
from oracle import decode_oracle as oracle

pytestmark = pytest.mark.gpu
FIELDS = ("walks_f", "walks_b", "len_f", "len_b", "sum_f", "sum_b", "contig_len", "status")


def dev():
    return torch.device("cuda", 0)


def _decode_graph(g):
    from gnnome_amd import decode
    dg = decode.DecodeGraph(g["src"], g["dst"], g["num_nodes"], g["prefix_length"], g["read_length"], device=dev())
    return dg.set_scores(g["scores"])


def _visited_array(g):
    v = torch.zeros(g["num_nodes"], dtype=torch.uint8, device=dev())
    if g["visited"]:
        v[torch.tensor(g["visited"], device=dev())] = 1
    return v


def _launch(g, starts=None, **kw):
    from gnnome_amd import decode
    res = decode.greedy_walks(_decode_graph(g), _visited_array(g), torch.tensor(g["starts"] if starts is None else starts), **kw)
    return {k: getattr(res, k).cpu() for k in FIELDS}


def _assert_same_outputs(a, b):
    for k in ("len_f", "len_b", "sum_f", "sum_b", "contig_len", "status"):
        assert torch.equal(a[k], b[k]), k                    # fp32 sums compared as values of equal bits: no NaN arises here
    assert torch.equal(a["sum_f"].view(torch.int32), b["sum_f"].view(torch.int32))
    assert torch.equal(a["sum_b"].view(torch.int32), b["sum_b"].view(torch.int32))
    for c in range(a["len_f"].numel()):
        assert torch.equal(a["walks_f"][c, :a["len_f"][c]], b["walks_f"][c, :b["len_f"][c]])
        assert torch.equal(a["walks_b"][c, :a["len_b"][c]], b["walks_b"][c, :b["len_b"][c]])


def _assert_equals_statement(g, res, want, edges):
    """walks, lengths, contig lengths, status 0, fp32 sums bitwise."""
    bad = []
    for c, w in enumerate(want):
        walk_f, walk_b, sum_f, sum_b = w[0], w[1], w[4], w[5]
        lf, lb = int(res["len_f"][c]), int(res["len_b"][c])
        got_f, got_b = res["walks_f"][c, :lf].tolist(), (torch.flip(res["walks_b"][c, :lb], [0]) ^ 1).tolist()
        clen = oracle.contig_length(walk_b + walk_f, edges, g["prefix_length"], g["read_length"])
        ok = got_f == walk_f and got_b == walk_b and int(res["contig_len"][c]) == clen and int(res["status"][c]) == 0
        ok = ok and torch.equal(res["sum_f"][c:c + 1].view(torch.int32), sum_f.view(torch.int32))
        ok = ok and torch.equal(res["sum_b"][c:c + 1].view(torch.int32), sum_b.view(torch.int32))
        if not ok:
            bad.append((c, g["starts"][c], got_b, got_f, walk_b, walk_f, int(res["contig_len"][c]), clen))
    assert not bad, (len(bad), bad[0])


def _opts_entry_directly(g, stop_logp, mode, seed):
    """gnnome_greedy_walks_opts called as gnnome_amd.decode.greedy_walks calls it, with the switch values given as they are."""
    from gnnome_amd import _lib, decode
    from gnnome_amd.ops import _on, _ptr, _stream
    lib, d = _lib.load(), dev()
    dg, visited = _decode_graph(g), _visited_array(g)
    eid = torch.tensor(g["starts"], device=d)
    cs, cd, ce = dg.src[eid].contiguous(), dg.dst[eid].contiguous(), dg.pair_eid[eid].contiguous()
    p, cap = int(eid.numel()), dg.num_nodes // 2 + 2
    out = {"walks_f": torch.empty((p, cap), dtype=torch.int32, device=d), "walks_b": torch.empty((p, cap), dtype=torch.int32, device=d)}
    for k, dt in (("len_f", torch.int32), ("len_b", torch.int32), ("sum_f", torch.float32), ("sum_b", torch.float32),
                  ("contig_len", torch.int64), ("status", torch.int32)):
        out[k] = torch.empty(p, dtype=dt, device=d)
    need = ctypes.c_size_t(0)
    _lib.check(lib.gnnome_greedy_walks_workspace_bytes(dg.num_nodes, p, ctypes.byref(need)), "workspace")
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=d)
    with _on(d):
        _lib.check(lib.gnnome_greedy_walks_opts(_ptr(dg.succ_ptr), _ptr(dg.succ_nbr), _ptr(dg.succ_eid), _ptr(dg.logp), _ptr(dg.prefix_length),
                                                _ptr(dg.read_length), _ptr(visited), dg.num_nodes, _ptr(cs), _ptr(cd), _ptr(ce), p,
                                                _ptr(out["walks_f"]), _ptr(out["walks_b"]), cap, *[_ptr(out[k]) for k in FIELDS[2:]], _ptr(ws),
                                                ws.numel(), stop_logp, mode, seed, _stream(d)),
                   "greedy_walks_opts")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ switches off

@pytest.mark.parametrize("i", [1, 2, 7, 16, 21, 25, 29])
def test_hip_new_entry_with_switches_off_equals_the_old_entry_bit_for_bit(i):
    g = adversarial_graph(**CASES[i])
    old = _launch(g)
    _assert_same_outputs(_opts_entry_directly(g, -math.inf, 0, 0), old)
    _assert_same_outputs(_opts_entry_directly(g, -math.inf, 0, 12345), old)       # the seed is not read in rank mode


@pytest.mark.parametrize("name", [n for n, _, ps in WALK_CASES if 1e-30 in ps])
def test_hip_a_threshold_nothing_is_below_gives_the_default_entrys_walks(name):
    """p_threshold = 1e-30 runs the kernel WITH the early-stopping test, which never fires (every log-probability of these graphs
    is above log(1e-30), asserted in the host tests): outputs equal the default entry's bit for bit."""
    g = case(name)[0]
    _assert_same_outputs(_launch(g, early_stopping=True, p_threshold=1e-30), _launch(g))


# ------------------------------------------------------------------------------------------------ early stopping

@pytest.mark.parametrize("name,p", [(n, p) for n, _, ps in WALK_CASES for p in ps])
def test_hip_early_stopping_equals_the_statement_and_the_reference(name, p):
    g, _, _, edges, _ = case(name)
    res = _launch(g, early_stopping=True, p_threshold=p)
    _assert_equals_statement(g, res, statement_walks(name, True, p, False, 0), edges)
    fx = {c["name"]: c for c in load_golden("g19_decode_switches.pt")["walks"]}[name]
    run = next(r for r in fx["runs"] if r["p_threshold"] == p)
    for c, want in enumerate(run["candidates"]):
        lf, lb = int(res["len_f"][c]), int(res["len_b"][c])
        assert res["walks_f"][c, :lf].tolist() == want["walk_f"], (name, p, want["edge"])
        assert (torch.flip(res["walks_b"][c, :lb], [0]) ^ 1).tolist() == want["walk_b"], (name, p, want["edge"])


# ------------------------------------------------------------------------------------------------ random mode

@pytest.mark.parametrize("name,early,p,seed", RANDOM_RUNS)
def test_hip_random_walks_equal_the_statement(name, early, p, seed):
    """Several seeds (both sides of 2^63), lists longer than 64 with more and with fewer than 64 admissible successors, early
    stopping on and off; a second launch from the same seed gives identical outputs."""
    g, _, _, edges, _ = case(name)
    res = _launch(g, early_stopping=early, p_threshold=p, random_walks=True, seed=seed)
    _assert_equals_statement(g, res, statement_walks(name, early, p, True, seed), edges)
    _assert_same_outputs(_launch(g, early_stopping=early, p_threshold=p, random_walks=True, seed=seed), res)


def test_hip_random_candidates_on_one_start_edge_differ_and_other_seeds_differ():
    """100 candidates on the same start edge of a graph with wide hubs: the draw depends on the candidate index, so they do not all
    walk alike; candidate 0 walks as it does alone; another seed gives other walks."""
    g = case("wide_open")[0]
    k = int((g["dst"] == g["hubs"][0]).nonzero()[0])     # an edge into the hub of 104 successors; nothing of this graph is visited
    res = _launch(g, starts=[k] * 100, random_walks=True, seed=21)
    walks = {(tuple(res["walks_f"][c, :res["len_f"][c]].tolist()), tuple(res["walks_b"][c, :res["len_b"][c]].tolist())) for c in range(100)}
    assert len(walks) >= 3
    alone = _launch(g, starts=[k], random_walks=True, seed=21)
    assert torch.equal(alone["walks_f"][0, :alone["len_f"][0]], res["walks_f"][0, :res["len_f"][0]])
    assert torch.equal(alone["walks_b"][0, :alone["len_b"][0]], res["walks_b"][0, :res["len_b"][0]])
    other = _launch(g, starts=[k] * 100, random_walks=True, seed=22)
    assert any(not torch.equal(other["walks_f"][c, :other["len_f"][c]], res["walks_f"][c, :res["len_f"][c]]) for c in range(100))


@pytest.mark.parametrize("name,kw", [("wide_open", dict(random_walks=True, seed=8)), ("parallel", dict(random_walks=True, seed=9, early_stopping=True)),
                                     ("wide_hubs", dict(early_stopping=True, p_threshold=0.95)), ("small_hubs", dict(random_walks=True, seed=10))])
def test_hip_every_walk_is_a_path_that_repeats_nothing_and_enters_nothing_visited(name, kw):
    g, succs, _, _, _ = case(name)
    res = _launch(g, **kw)
    gone = set(g["visited"])
    for c, k in enumerate(g["starts"]):
        s, d = int(g["src"][k]), int(g["dst"][k])
        wf = res["walks_f"][c, :res["len_f"][c]].tolist()
        wb = res["walks_b"][c, :res["len_b"][c]].tolist()           # as walked, on the reverse-complement strand
        assert wf[0] == d and wb[0] == s ^ 1
        for w in (wf, wb):
            assert all(b in succs[a] for a, b in zip(w[:-1], w[1:]))
        nodes = wf + wb
        reads = [x >> 1 for x in nodes]
        assert len(set(reads)) == len(reads) or (s >> 1) == (d >> 1)    # no node and no mate twice (a self-loop's two halves start on one read)
        inner = wf[1:] + wb[1:]
        assert not (set(inner) & gone) and not (set(inner) & {s, s ^ 1, d, d ^ 1})


# ------------------------------------------------------------------------------------------------ the outer loop

def _outer_graph(i):
    return adversarial_graph(**OUTER_CASES[i][1])


@pytest.mark.parametrize("i", range(len(OUTER_CASES)))
def test_hip_outer_loop_with_early_stopping_equals_the_statement_and_the_reference(i):
    from gnnome_amd import decode
    g = _outer_graph(i)
    fx = load_golden("g19_decode_switches.pt")["outer"][i]
    assert fx["name"] == OUTER_CASES[i][0]
    for (seed, threshold, nb_paths, p), run in zip(OUTER_CASES[i][2], fx["runs"]):
        torch.manual_seed(seed)
        trace = []
        want = st.get_contigs_greedy(g["src"], g["dst"], g["num_nodes"], g["scores"], g["prefix_length"], g["read_length"], threshold,
                                     nb_paths=nb_paths, sw=st.Switches(True, p), trace=trace)
        torch.manual_seed(seed)
        stats = []
        got = decode.decode_contigs(_decode_graph(g), threshold, nb_paths=nb_paths, sampler=decode.sample_edges, stats=stats,
                                    early_stopping=True, p_threshold=p)
        assert got == want == run["walks"]
        assert [s["contig_len"] for s in stats] == [t["contig_len"] for t in trace]


class _G:
    def __init__(self, g):
        self.g, self.ndata, self.edata = g, {"read_length": g["read_length"]}, {"prefix_length": g["prefix_length"], "score": g["scores"]}

    def edges(self):
        return self.g["src"], self.g["dst"]

    def num_nodes(self):
        return self.g["num_nodes"]


@pytest.mark.parametrize("i,early", [(0, False), (0, True), (1, False), (1, True)])
def test_hip_outer_loop_with_random_walks_equals_the_statement(i, early):
    """Same torch.manual_seed: the start edges are torch.randint draws from the CPU generator on both sides (the reference's,
    inference.py:60), the kernel seeds launch_seed(seed, iteration); nb_paths = 30 on a small graph draws the same start edge more
    than once, so the reference's dict rule (the last candidate on a pair counts, at the place of the first) is exercised.
    seed=None takes torch.initial_seed(); get_contigs_greedy passes the keywords on."""
    from gnnome_amd import decode
    g = _outer_graph(i)
    repeats = 0
    for seed, threshold, nb_paths in ((31, 0, 30), (2 ** 63 + 32, 25_000, 5)):
        draws = []

        def watching(prob, k):
            idx = st.sample_edges_uniform(prob, k)
            draws.append(idx.tolist())
            return idx

        torch.manual_seed(100 + i)
        trace = []
        want = st.get_contigs_greedy(g["src"], g["dst"], g["num_nodes"], g["scores"], g["prefix_length"], g["read_length"], threshold,
                                     nb_paths=nb_paths, sw=st.Switches(early, 0.5, True, seed), trace=trace, sampler=watching)
        repeats += sum(len(set(d)) < len(d) for d in draws)
        torch.manual_seed(100 + i)
        stats = []
        got = decode.decode_contigs(_decode_graph(g), threshold, nb_paths=nb_paths, stats=stats, early_stopping=early, p_threshold=0.5,
                                    random_walks=True, seed=seed)
        assert got == want and len(want) >= 2
        assert [s["contig_len"] for s in stats] == [t["contig_len"] for t in trace]
    assert repeats >= 1
    torch.manual_seed(7)
    want = st.get_contigs_greedy(g["src"], g["dst"], g["num_nodes"], g["scores"], g["prefix_length"], g["read_length"], 0, nb_paths=4,
                                 sw=st.Switches(early, 0.5, True, 7))
    torch.manual_seed(7)
    assert decode.get_contigs_greedy(_G(g), None, None, None, 0, nb_paths=4, early_stopping=early, p_threshold=0.5, random_walks=True) == want


def _largest(prob, k):
    return torch.argsort(prob.cpu(), descending=True, stable=True)[:k]


class _Interrupt(Exception):
    pass


def test_hip_resumed_random_decode_continues_the_interrupted_one(tmp_path):
    """Interrupted right after the checkpoint of contig 10, resumed with load_checkpoint=True: the walks of the uninterrupted run -
    the kernel seed of an iteration depends on `seed` and the number of contigs found, not on how the run got there."""
    from gnnome_amd import decode
    g = adversarial_graph(seed=1920, hubs=("d64", "mid", "d3", "d4"), reads=200, parallel=0.05)
    dg = _decode_graph(g)
    kw = dict(nb_paths=8, random_walks=True, seed=77, early_stopping=True, p_threshold=0.06)
    whole = decode.decode_contigs(dg, 0, sampler=_largest, **kw)
    assert len(whole) >= 14
    want = st.get_contigs_greedy(g["src"], g["dst"], g["num_nodes"], g["scores"], g["prefix_length"], g["read_length"], 0, nb_paths=8,
                                 sampler=_largest, sw=st.Switches(True, 0.06, True, 77))
    assert whole == want
    ckpt = tmp_path / "checkpoint.pkl"

    def until_10(prob, k):
        if ckpt.is_file():
            with open(ckpt, "rb") as f:
                if len(pickle.load(f)["walks"]) == 10:
                    raise _Interrupt
        return _largest(prob, k)

    with pytest.raises(_Interrupt):
        decode.decode_contigs(dg, 0, sampler=until_10, checkpoint_dir=str(tmp_path), **kw)
    resumed = decode.decode_contigs(dg, 0, sampler=_largest, checkpoint_dir=str(tmp_path), load_checkpoint=True, **kw)
    assert resumed == whole
    other = decode.decode_contigs(dg, 0, sampler=_largest, **{**kw, "seed": 78})
    assert other != whole


# ------------------------------------------------------------------------------------------------ the per-candidate figures

def test_hip_candidates_table_equals_the_reference_rules():
    """gnnome_candidate_table against inference.py:267-296 computed on the host (Python doubles) from the same launch's outputs:
    the gadget graph holds a self-loop start edge (walk length 1, every figure 0) and a two-node walk (mean 0); exact equality."""
    from gnnome_amd import decode
    seen = set()
    for name, kw in (("gadgets", {}), ("gadgets", dict(early_stopping=True)), ("small_hubs", dict(random_walks=True, seed=4)), ("wide_hubs", {})):
        g = case(name)[0]
        res = decode.greedy_walks(_decode_graph(g), _visited_array(g), torch.tensor(g["starts"]), **kw)
        table = decode.candidates_table(res)
        assert tuple(table) == decode.CANDIDATE_FIGURES
        host = {k: getattr(res, k).cpu() for k in ("src", "dst", "len_f", "len_b", "sum_f", "sum_b", "contig_len")}
        for c in range(len(g["starts"])):
            s, d = int(host["src"][c]), int(host["dst"][c])
            want = st.candidate_figures(s, d, int(host["len_f"][c]) + int(host["len_b"][c]), int(host["contig_len"][c]),
                                        host["sum_f"][c].item(), host["sum_b"][c].item())
            got = tuple(table[k][c] for k in decode.CANDIDATE_FIGURES)
            assert got == (s, d) + want, (name, c, got, want)
            assert isinstance(got[2], int) and isinstance(got[3], int) and isinstance(got[6], float)
            seen.add("loop" if s == d else "two" if want[0] == 2 else "long")
            if want[0] > 2 and want[1] > 0:
                assert got[5] == want[2] / (want[0] - 2) and got[6] == got[5] / math.sqrt(want[1])
    assert seen == {"loop", "two", "long"}
    g = _outer_graph(0)
    stats = []
    decode.decode_contigs(_decode_graph(g), 0, nb_paths=6, sampler=_largest, stats=stats, stats_per_candidate=True)
    assert stats and all(len(s["candidates_table"]["len_walk"]) == s["candidates"] for s in stats)
    for s in stats:
        t = s["candidates_table"]
        best = t["len_contig"].index(max(t["len_contig"]))
        assert t["len_contig"][best] == s["contig_len"]
        # a self-loop's row says 1 (inference.py:271-272) whatever its two halves hold
        assert t["len_walk"][best] == (1 if t["src"][best] == t["dst"][best] else s["walk_len"])
    plain = []
    decode.decode_contigs(_decode_graph(g), 0, nb_paths=6, sampler=_largest, stats=plain)
    assert plain and "candidates_table" not in plain[0]


# ------------------------------------------------------------------------------------------------ the pipeline

def test_hip_pipeline_assemble_passes_the_switches_on():
    from gnnome_amd import decode, pipeline
    g = _outer_graph(0)
    for kw in (dict(early_stopping=True), dict(early_stopping=True, p_threshold=0.5), dict(random_walks=True, seed=5)):
        want = decode.decode_contigs(_decode_graph(g), 0, nb_paths=8, sampler=_largest, **kw)
        walks, scores, _ = pipeline.assemble(dict(g), None, 0, nb_paths=8, device=dev(), scores=g["scores"], sampler=_largest, **kw)
        assert walks == want and torch.equal(torch.as_tensor(scores), g["scores"])
    ablation = pipeline.assemble(dict(g), None, 0, nb_paths=8, device=dev(), scores=decode.constant_scores(g), random_walks=True, seed=1)[0]
    assert ablation and all(len(w) >= 1 for w in ablation)
