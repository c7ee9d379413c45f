"""The decoder switches without a device: the statement (tests/decode_switch_statement.py) against walks of the reference's own
functions with early_stopping = True (tests/golden/g19_decode_switches.pt, made by make_golden_decode_switches.py), the precision
torch compares `fp32 tensor < Python double` in, that the cases reach every boundary of the early-stopping rule, the random draw,
and the plumbing: keywords, helpers, and the header / _lib.SIGNATURES agreement of the two new entries."""
import ctypes
import inspect
import math

import numpy as np
import torch

import decode_switch_statement as st
import header_binding
from conftest import load_golden
from decode_switch_cases import AT_006, RANDOM_RUNS, WALK_CASES, case, statement_walks
from gnnome_amd import _lib, decode, pipeline
from oracle import decode_oracle as oracle


def test_torch_compares_an_fp32_tensor_with_a_python_double_in_fp32():
    """inference.py:99 is `neighbor_p < math.log(p_threshold)`: fp32 tensor, Python double.  torch rounds the double to fp32 and
    compares in fp32.  log(0.06) rounds DOWN (away from zero), so the fp32 value x = fp32(log(0.06)) is below the double - a compare
    in double would call it below the threshold - and torch says it is not.  This is what `stop_logp` of the kernel restates."""
    t64 = math.log(0.06)
    x = np.float32(t64)
    assert float(x) < t64                                          # in double, x is below the threshold
    for n in (1, 3, 37):                                           # scalar and vectorised paths of the CPU kernel
        assert not bool((torch.full((n,), float(x), dtype=torch.float32) < t64).any())
    below = np.nextafter(x, np.float32(-np.inf))
    assert bool((torch.tensor([float(below)], dtype=torch.float32) < t64).all())
    assert decode.stop_log_prob(True, 0.06) == float(x) and decode.stop_log_prob(False, 0.06) == -math.inf
    assert float(torch.log(torch.sigmoid(torch.tensor([AT_006])))) == float(x)


def test_statement_equals_the_reference_walks_with_early_stopping():
    fx = load_golden("g19_decode_switches.pt")
    assert [c["name"] for c in fx["walks"]] == [n for n, _, _ in WALK_CASES]
    for c in fx["walks"]:
        g = case(c["name"])[0]
        assert torch.equal(c["src"].long(), g["src"]) and torch.equal(c["scores"], g["scores"]) and c["starts"] == g["starts"]
        assert c["visited"] == g["visited"]
        _, succs, preds, edges, _ = case(c["name"])
        for run in c["runs"]:
            # on the fixture's own log-probabilities: the sums are then the same fp32 additions on every machine
            sw = st.Switches(True, run["p_threshold"])
            got = [st.run_greedy_both_ways(int(g["src"][e]), int(g["dst"][e]), c["logp"], succs, preds, edges, set(g["visited"]), sw)
                   for e in g["starts"]]
            for k, (want, have) in enumerate(zip(run["candidates"], got)):
                assert have[0] == want["walk_f"] and have[1] == want["walk_b"], (c["name"], run["p_threshold"], want["edge"])
                assert sorted(have[2]) == want["visited_f"] and sorted(have[3]) == want["visited_b"]
                assert torch.equal(have[4], run["sum_f"][k:k + 1]) and torch.equal(have[5], run["sum_b"][k:k + 1])


def test_statement_outer_loop_equals_the_reference_function_with_early_stopping():
    fx = load_golden("g19_decode_switches.pt")
    assert len(fx["outer"]) >= 2
    for c in fx["outer"]:
        for run in c["runs"]:
            torch.manual_seed(run["seed"])
            got = st.get_contigs_greedy(c["src"].long(), c["dst"].long(), c["num_nodes"], c["scores"], c["prefix_length"].long(),
                                        c["read_length"].long(), run["len_threshold"], nb_paths=run["nb_paths"],
                                        sw=st.Switches(True, run["p_threshold"]))
            assert got == run["walks"], (c["name"], run["seed"])


def test_switches_off_is_the_oracle_and_a_low_threshold_stops_nothing():
    for name, _, ps in WALK_CASES:
        g, succs, preds, edges, logp = case(name)
        off = statement_walks(name, False, 0.06, False, 0)
        for c, k in enumerate(g["starts"]):
            want = oracle.run_greedy_both_ways(int(g["src"][k]), int(g["dst"][k]), logp, succs, preds, edges, set(g["visited"]))
            assert off[c][:2] == want[:2] and torch.equal(off[c][4], want[4]) and torch.equal(off[c][5], want[5])
        if 1e-30 in ps:
            assert float(logp.min()) > math.log(1e-30)
            low = statement_walks(name, True, 1e-30, False, 0)
            assert [w[:2] for w in low] == [w[:2] for w in off]


CLASSES = ("stop_forward_only", "stop_backward_only", "stop_both", "stop_neither", "successor_exactly_at_threshold",
           "single_improbable_successor_taken", "list_ge2_masked_to_one_improbable_stops", "stop_on_list_gt64", "rank_on_list_gt64",
           "random_among_more_than_64", "random_on_list_gt64_among_fewer", "random_after_early_stopping_test", "stop_in_random_mode")


def test_cases_reach_every_boundary_of_the_switches():
    """Counted on the statement's own trace of the walks the device tests compare: every class at least once."""
    counts = dict.fromkeys(CLASSES, 0)
    for name, _, ps in WALK_CASES:
        for p in ps:
            t32, t64 = float(np.float32(math.log(p))), math.log(p)
            for w in statement_walks(name, True, p, False, 0):
                ev = w[6]
                sf, sb = any(e[0] == "stop" for e in ev["f"]), any(e[0] == "stop" for e in ev["b"])
                if p != 1e-30:
                    counts["stop_forward_only"] += sf and not sb
                    counts["stop_backward_only"] += sb and not sf
                    counts["stop_both"] += sf and sb
                    counts["stop_neither"] += not sf and not sb
                for kind, n_list, n_adm, top in ev["f"] + ev["b"]:
                    counts["successor_exactly_at_threshold"] += kind == "rank" and top == t32 and top < t64
                    counts["single_improbable_successor_taken"] += kind == "single" and top < t32
                    counts["list_ge2_masked_to_one_improbable_stops"] += kind == "stop" and n_list >= 2 and n_adm == 1
                    counts["stop_on_list_gt64"] += kind == "stop" and n_list > 64
                    counts["rank_on_list_gt64"] += kind == "rank" and n_list > 64
    for name, early, p, seed in RANDOM_RUNS:
        for w in statement_walks(name, early, p, True, seed):
            for kind, n_list, n_adm, top in w[6]["f"] + w[6]["b"]:
                counts["random_among_more_than_64"] += kind == "random" and n_adm > 64
                counts["random_on_list_gt64_among_fewer"] += kind == "random" and n_list > 64 and n_adm <= 64
                counts["random_after_early_stopping_test"] += kind == "random" and early
                counts["stop_in_random_mode"] += kind == "stop"
    print("steps per class:", counts)
    assert not {k: v for k, v in counts.items() if v < 1}


def test_the_draw_is_splitmix64_and_multiply_shift():
    """Known outputs of splitmix64 seeded with 0 (the published test vector), then the reduction: in range, the top 32 bits only,
    every value of a small range reached, and a function of each of the four arguments."""
    assert [st.mix64(k * st.GOLDEN_GAMMA) for k in (1, 2, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert st.draw(0, 0, 0, 0, 2 ** 31 - 1) == ((0xE220A8397B1DCDAF >> 32) * (2 ** 31 - 1)) >> 32
    assert st.launch_seed(0, 0) == 0xE220A8397B1DCDAF and decode.launch_seed(0, 0) == 0xE220A8397B1DCDAF
    assert all(decode.launch_seed(s, i) == st.launch_seed(s, i) for s in (0, 1, 2 ** 64 - 1, 977) for i in (0, 1, 50))
    for n in (1, 2, 3, 7, 64, 65, 300):
        seen = {st.draw(11, c, h, s, n) for c in range(6) for h in (0, 1) for s in range(60)}
        assert seen <= set(range(n)) and (n > 7 or seen == set(range(n)))
    base = [st.draw(5, 1, 0, s, 1000) for s in range(32)]
    assert base != [st.draw(6, 1, 0, s, 1000) for s in range(32)] and base != [st.draw(5, 2, 0, s, 1000) for s in range(32)]
    assert base != [st.draw(5, 1, 1, s, 1000) for s in range(32)] and len(set(base)) > 16


def test_keywords_and_helpers():
    want = {"early_stopping": False, "p_threshold": 0.06, "random_walks": False, "seed": None}
    for fn in (decode.greedy_walks, decode.decode_contigs, decode.get_contigs_greedy, pipeline.assemble, pipeline.assemble_to_fasta):
        params = inspect.signature(fn).parameters
        assert {k: params[k].default for k in want} == want, fn.__name__
    assert inspect.signature(decode.decode_contigs).parameters["stats_per_candidate"].default is False
    prob = torch.rand(500)
    torch.manual_seed(3)
    a = decode.sample_edges_uniform(prob, 40)
    torch.manual_seed(3)
    assert torch.equal(a, st.sample_edges_uniform(prob, 40))
    torch.manual_seed(3)
    assert torch.equal(a, torch.randint(0, 500, (40,)))              # inference.py:60, the reference's own call
    s = decode.constant_scores(17)
    assert s.dtype == torch.float32 and s.tolist() == [10.0] * 17 and decode.constant_scores({"src": torch.zeros(5)}).numel() == 5
    for bad in (0.0, -1.0):
        try:
            decode.stop_log_prob(True, bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_header_and_binding_table_agree_on_the_new_entries():
    parsed = header_binding.parse_header(_lib.HEADER_PATH)
    _, argtypes, names = parsed["gnnome_greedy_walks_opts"]
    _, old_types, old_names = parsed["gnnome_greedy_walks"]
    assert names[:len(old_names) - 1] == old_names[:-1] and names[-4:] == ["stop_logp", "choice_mode", "seed", "stream"]
    assert argtypes[-4:] == [ctypes.c_float, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    assert _lib.SIGNATURES["gnnome_greedy_walks_opts"][-4:] == [ctypes.c_float, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    assert len(_lib.SIGNATURES["gnnome_greedy_walks_opts"]) == len(_lib.SIGNATURES["gnnome_greedy_walks"]) + 3
    assert parsed["gnnome_candidate_table"][2] == ["cand_src", "cand_dst", "len_f", "len_b", "sum_f", "sum_b", "contig_len",
                                                   "num_candidates", "table", "stream"]
    header = open(_lib.HEADER_PATH).read()
    block = header[header.index("The same launch with the reference's two decoder switches"):header.index("int gnnome_greedy_walks_opts(")]
    for cite in ("inference.py:26-28", ":98-100", ":142-145", ":102-104", ":147-149", "DELIBERATE DIVERGENCE"):
        assert cite in block, cite


def test_new_entries_validate_their_arguments_without_a_gpu():
    lib = _lib.load()
    none = [None] * 7 + [0] + [None] * 3
    tail = [None, None, 8, None, None, None, None, None, None, None, 0]
    assert lib.gnnome_greedy_walks_opts(*none, 0, *tail, -math.inf, 0, 0, None) == 0                 # no candidates: nothing to do
    assert lib.gnnome_greedy_walks_opts(*none, 0, *tail, -math.inf, 2, 0, None) == -1 and b"choice_mode" in lib.gnnome_last_error()
    assert lib.gnnome_greedy_walks_opts(*none, 0, *tail, math.nan, 0, 0, None) == -1 and b"stop_logp" in lib.gnnome_last_error()
    assert lib.gnnome_greedy_walks_opts(*none, 3, *tail, -2.8, 1, -5, None) == -1 and b"null" in lib.gnnome_last_error()
    assert lib.gnnome_candidate_table(None, None, None, None, None, None, None, 0, None, None) == 0
    assert lib.gnnome_candidate_table(None, None, None, None, None, None, None, 4, None, None) == -1 and b"null" in lib.gnnome_last_error()
