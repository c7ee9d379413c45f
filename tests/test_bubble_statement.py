"""tests/bubble_statement.py against properties that do not come from it (no GPU): on a diploid overlap graph built from read positions
alone one round of the rule must leave one line per strand; on hand-made graphs every clause of the rule is spelled out, one assertion
each."""
import numpy as np
import pytest

import bubble_cases as bc
import bubble_statement as bs
import graph_simplify_statement as gs

ALL_SEEDS = tuple(range(8))
MARKED = {1: 18, 2: 24, 4: 26, 5: 22}


@pytest.fixture(scope="module")
def diploid():
    return {seed: gs.simplify_graph(bc.diploid_graph(seed), fuzz=0) for seed in ALL_SEEDS}


def degrees(g, keep):
    return np.bincount(g["src"][keep], minlength=g["num_nodes"]), np.bincount(g["dst"][keep], minlength=g["num_nodes"])


def marked(g, **kw):
    return np.nonzero(bs.bubble_nodes(g, **kw))[0].tolist()


def both_strands(nodes):
    return sorted(set(nodes) | {v ^ 1 for v in nodes})


# ---- the diploid graph ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", bc.DIPLOID_SEEDS)
def test_one_round_leaves_one_line_per_strand(diploid, seed):
    g = diploid[seed]
    everything = np.ones(len(g["src"]), dtype=bool)
    out_deg, in_deg = degrees(g, everything)
    assert out_deg.max() == 2 and in_deg.max() == 2                                         # forks and joins at the sites
    mark = bs.bubble_nodes(g)
    assert int(mark.sum()) == MARKED[seed] and np.array_equal(mark[0::2], mark[1::2])
    keep = ~mark[g["src"]] & ~mark[g["dst"]]
    out_deg, in_deg = degrees(g, keep)
    assert out_deg.max() == 1 and in_deg.max() == 1
    assert int(((in_deg > 0) & (out_deg == 0)).sum()) == 2                                  # one line per strand
    assert gs.mate_closed(g["src"][keep], g["dst"][keep])
    assert not bs.bubble_nodes(g, keep).any()                                               # a second round marks nothing
    total, rounds, kept = bs.pop_rounds(g)
    assert rounds == 1 and np.array_equal(total, mark) and np.array_equal(kept, keep)


@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_every_loser_lies_in_one_bubble_and_no_end_of_a_bubble_is_marked(diploid, seed):
    g = diploid[seed]
    mark = bs.bubble_nodes(g)
    pairs = bs.losers(g)
    assert pairs and int(mark.sum()) == sum(a["nodes"] for a, _ in pairs)                   # a loser's mate is a loser; the arms are disjoint
    edges = set(zip(g["src"].tolist(), g["dst"].tolist()))
    for arm, win in pairs:
        assert (arm["source"], arm["sink"]) == (win["source"], win["sink"]) and not set(arm["chain"]) & set(win["chain"])
        path = [arm["source"]] + arm["chain"] + [arm["sink"]]
        assert all(e in edges for e in zip(path, path[1:]))
        assert not mark[win["chain"]].any()
        for v in (arm["source"], arm["sink"]):
            assert not mark[v] and not mark[v ^ 1]
    assert np.array_equal(mark[0::2], mark[1::2])
    keep = ~mark[g["src"]] & ~mark[g["dst"]]
    assert gs.mate_closed(g["src"][keep], g["dst"][keep])


# ---- the choice of the winner ---------------------------------------------------------------------------------------------------

def test_the_heavier_arm_stays():
    g, a1, a3 = bc.two_arms(1, 3)
    assert marked(g) == both_strands(a1)
    arms = bs.bubble_arms(g)
    assert arms["first"].tolist() == [8, 9, 10, 15] and arms["nodes"].tolist() == [1, 1, 3, 3]
    assert arms["source"].tolist() == [2, 5, 2, 5] and arms["sink"].tolist() == [4, 3, 4, 3] and arms["last"].tolist() == [8, 9, 14, 11]
    assert arms["weight"].tolist() == [1, 1, 3, 3] and arms["overlap"].tolist() == [1000, 1000, 2000, 2000]


def test_equal_weight_goes_to_the_larger_summed_overlap():
    g, a, b = bc.two_arms(2, 2, ol1=[500, 500, 500], ol2=[500, 501, 500])
    assert marked(g) == both_strands(a)


@pytest.mark.parametrize("flip", (False, True))
def test_equal_weight_and_overlap_go_to_the_smaller_key_on_both_strands(flip):
    g, a, b = bc.two_arms(2, 2, flip=flip)
    assert marked(g) == both_strands(b)                                                     # min(a_1, a_k ^ 1): 8 against 12, 9 against 13


def test_the_key_is_the_same_for_an_arm_and_its_mate():
    g, a, b = bc.two_arms(2, 2)
    arms = bs.arm_list(g)
    key = {a["first"]: min(a["first"], a["last"] ^ 1) for a in arms}
    assert all(key[a["first"]] == key[a["last"] ^ 1] for a in arms) and len(set(key.values())) == 2


def test_the_weight_column_overrides_the_node_count():
    g, a1, a3 = bc.two_arms(1, 3)
    weight = np.ones(g["num_nodes"], dtype=np.int64)
    weight[[a1[0], a1[0] ^ 1]] = 4
    assert marked(g, weight=weight) == both_strands(a3)


# ---- the two bounds -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_diff,pops", ((300, True), (299, False)))
def test_a_difference_of_max_diff_pops_and_one_more_does_not(max_diff, pops):
    """dist = 1000 - 2 * 500 = 0 for the one-read arm and 3000 - 4 * 675 = 300 for the winner."""
    g, a1, a3 = bc.two_arms(1, 3, ol2=675)
    assert sorted(bs.bubble_arms(g)["dist"].tolist()) == [0, 0, 300, 300]
    assert marked(g, max_diff=max_diff) == (both_strands(a1) if pops else [])


@pytest.mark.parametrize("max_dist,pops", ((300, True), (299, False)))
def test_a_winner_at_max_dist_pops_and_one_base_further_does_not(max_dist, pops):
    g, a1, a3 = bc.two_arms(1, 3, ol2=675)                                                  # the winner is the far one
    assert marked(g, max_dist=max_dist) == (both_strands(a1) if pops else [])


@pytest.mark.parametrize("max_dist,pops", ((400, True), (399, False)))
def test_an_arm_at_max_dist_pops_and_one_base_further_does_not(max_dist, pops):
    g, a1, a3 = bc.two_arms(1, 3, ol1=300, ol2=750)                                         # the loser is the far one: 1000 - 600 against 0
    assert sorted(bs.bubble_arms(g)["dist"].tolist()) == [0, 0, 400, 400]
    assert marked(g, max_dist=max_dist) == (both_strands(a1) if pops else [])


def test_a_negative_distance_is_a_distance():
    g, a1, a3 = bc.two_arms(1, 3, ol1=600, ol2=800)
    assert sorted(bs.bubble_arms(g)["dist"].tolist()) == [-200, -200, -200, -200] and marked(g, max_diff=0) == both_strands(a1)


# ---- what is no bubble ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(bc.no_bubble_graphs()))
def test_shapes_that_are_no_bubble(name):
    assert marked(bc.no_bubble_graphs()[name]) == [], name


def test_the_arms_of_the_shapes_that_are_no_bubble():
    arms = {name: bs.bubble_arms(g) for name, g in bc.no_bubble_graphs().items()}
    assert arms["a direct edge beside an arm"]["first"].tolist() == [8, 9]
    assert arms["parallel edges into a_1"]["first"].tolist() == [10, 11]
    assert arms["an arm that forks before it joins"]["first"].tolist() == [8, 9, 12, 13]
    for name in ("t == s", "t == s ^ 1", "a circular chain"):
        assert arms[name]["first"].size == 0, name


def test_a_weight_that_differs_between_the_strands_is_refused():
    g, a1, a3 = bc.two_arms(1, 3)
    weight = np.ones(g["num_nodes"], dtype=np.int64)
    weight[a1[0]] = 2
    with pytest.raises(ValueError, match="weight"):
        bs.bubble_nodes(g, weight=weight)
    with pytest.raises(ValueError, match="weight"):
        bs.bubble_nodes(g, weight=np.ones(g["num_nodes"]))                                  # not an int column
    with pytest.raises(ValueError, match="mates"):
        bs.bubble_nodes(g, keep=np.arange(len(g["src"])) > 0)


# ---- several bubbles, rounds, keep ----------------------------------------------------------------------------------------------

def test_two_bubbles_at_one_source_are_judged_separately():
    g = bc.two_bubbles_at_one_source()
    assert marked(g) == both_strands([8, 12, 14])                                           # overlaps 500 and 510 lose to 520; one read to two
    assert [(a["first"], w["first"]) for a, w in bs.losers(g) if a["source"] == 2] == [(8, 10), (12, 10), (14, 16)]


def test_a_bubble_inside_an_arm_goes_first():
    g = bc.nested_bubble()
    assert marked(g) == [12, 13]                                                            # round 1: the inner bubble only
    total, rounds, keep = bs.pop_rounds(g, rounds=1)
    assert rounds == 1 and np.nonzero(total)[0].tolist() == [12, 13]
    assert marked(g, keep=keep) == [8, 9]                                                   # round 2: the outer one
    total, rounds, keep = bs.pop_rounds(g)
    assert rounds == 2 and np.nonzero(total)[0].tolist() == [8, 9, 12, 13]
    out_deg, in_deg = degrees(g, keep)
    assert out_deg.max() == 1 and in_deg.max() == 1 and gs.mate_closed(g["src"][keep], g["dst"][keep])
    with pytest.raises(ValueError, match="rounds"):
        bs.pop_rounds(g, rounds=0)


def test_a_keep_mask_opens_a_bubble():
    g, a1, a3 = bc.two_arms(1, 3)
    gone = {(a3[0], a3[1]), (a3[1] ^ 1, a3[0] ^ 1)}
    keep = np.array([e not in gone for e in zip(g["src"].tolist(), g["dst"].tolist())])
    assert marked(g, keep=keep) == [] and marked(g) == both_strands(a1)


def test_pop_bubbles_indexes_back_and_counts():
    g = bc.nested_bubble()
    g["overlap_similarity"] = np.arange(len(g["src"]), dtype=np.float32)
    s = bs.pop_bubbles(g)
    assert s["removed"] == {"bubble_nodes": 4, "bubble_rounds": 2, "reads": 2} and s["num_nodes"] == 16
    assert s["kept_reads"].tolist() == [0, 1, 2, 3, 5, 7, 8, 9]
    assert np.array_equal(2 * s["kept_reads"][s["src"] >> 1] + (s["src"] & 1), g["src"][s["edge_origin"]])
    assert np.array_equal(2 * s["kept_reads"][s["dst"] >> 1] + (s["dst"] & 1), g["dst"][s["edge_origin"]])
    assert np.array_equal(s["overlap_similarity"], g["overlap_similarity"][s["edge_origin"]]) and len(s["src"]) == len(g["src"]) - 8
    assert gs.mate_closed(s["src"], s["dst"]) and (s["read_length"][s["src"]] - s["overlap_length"] == s["prefix_length"]).all()
    loose = bs.pop_bubbles(g, rounds=1, compact=False)
    assert loose["removed"] == {"bubble_nodes": 2, "bubble_rounds": 1, "reads": 0} and loose["num_nodes"] == 20
    whole = bs.simplify_graph(g, fuzz=0)
    assert whole["removed"] == {"transitive_edges": 0, "tip_nodes": 0, "bubble_nodes": 4, "bubble_rounds": 2, "reads": 2}
    assert np.array_equal(whole["edge_origin"], s["edge_origin"])
