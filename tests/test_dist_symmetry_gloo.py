"""The reversed pass of SymGatedGCNModel and the symmetry-loss step (train.py:159-170) on destination-range partitions, on CPU ranks over
gloo with the checker backend: `rev` logits against the whole-graph host sequence on views.reversed() and the reference golden G4, one
symmetry step against the oracle's autograd on the unpartitioned graph, a hand graph with the two shapes that only the reversed pass
exercises, the swapped degree columns of a from_slices plan, and what stays refused.  The bars are tests/test_dist_gloo.py's."""
import functools

import pytest
import torch

import cpu_ops
import gnnome_amd
from conftest import load_golden
from dist_symmetry_worker import run_ranks
from gnnome_amd import dist as gdist
from gnnome_amd import engine
from gnnome_amd.synth import random_state_dict
from test_train_host import check_grads

CPU = torch.device("cpu")


_run = functools.partial(run_ranks, timeout=180)   # (world, case, tmp_path) -> what each rank saved


def _prob_diff(a, b):
    return (torch.sigmoid(a) - torch.sigmoid(b)).abs().max().item()


def _g4_case(**kw):
    g = load_golden("g4_reverse_h64.pt")
    case = dict(src=g["src"], dst=g["dst"], num_nodes=g["num_nodes"], x=g["x"], x_rev=g["x_rev"], e=g["e"], y=g["y"], pos_weight=g["pos_weight"],
                alpha=g["alpha"], hidden=64, layers=8, state_dict=random_state_dict(64, seed=g["seed"]))
    case.update(kw)
    return g, case


@pytest.mark.parametrize("world", [2, 3])
def test_reversed_logits_match_the_whole_graph_host_sequence_and_golden_g4(world, tmp_path):
    g, case = _g4_case()
    m = gnnome_amd.models.SymGatedGCNModel(2, 2, 64, 16, 8, 64, "batch").eval()
    m.load_state_dict(case["state_dict"])
    views = cpu_ops.CpuViews(g["src"], g["dst"], g["num_nodes"])
    whole = engine.run_stack(cpu_ops, engine.Prepared(m, CPU), views.reversed(), g["x_rev"], g["e"])
    outs = _run(world, case, tmp_path)
    for o in outs:
        assert o["rev"].shape == whole.shape
        assert _prob_diff(o["rev"], whole) < 1e-4
        assert _prob_diff(o["rev"], g["logits_rev"].squeeze(1)) < 1e-4
        assert _prob_diff(o["org"], g["logits"].squeeze(1)) < 1e-4            # the forward pass of the same plan is what it was
        assert torch.equal(o["runner_rev"], o["rev"])                        # PartitionedRunner.forward(reverse=True): the same call
        assert o["plan_untouched"]
    assert torch.equal(outs[0]["rev"], outs[-1]["rev"])                      # every rank holds the full result
    assert _prob_diff(outs[0]["rev"], outs[0]["org"]) > 1e-3                 # (and it is another function than the forward pass)
    assert sum(o["n_score"] for o in outs) == g["src"].numel()               # each edge scored exactly once, by the same rank as forward
    assert sum(o["e_local"] for o in outs) > 1.05 * g["src"].numel()


@pytest.mark.parametrize("world", [2, 3])
def test_one_symmetry_step_matches_oracle_autograd(world, tmp_path):
    """loss, all 142 parameter gradients (the all-reduced sum of both passes) and the BatchNorm buffers against the oracle's autograd on
    the UNPARTITIONED graph; bn_e's running statistics advance four times per layer and step, bn_h's twice."""
    from oracle.symgated_oracle import OracleModel, symmetry_loss
    g, case = _g4_case(train=True)
    om = OracleModel(2, 2, 64, 16, 8, 64, "batch", dropout=0.0)
    om.load_state_dict(case["state_dict"])
    om.train()
    n = g["num_nodes"]
    org = om((g["src"], g["dst"], n), g["x"], g["e"]).squeeze(-1)
    rev = om((g["dst"], g["src"], n), g["x_rev"], g["e"]).squeeze(-1)        # dgl.reverse(g, True, True): endpoints swapped, ids kept
    want_loss = symmetry_loss(org, rev, g["y"], g["pos_weight"], g["alpha"])
    want_loss.backward()
    want_g = {k: p.grad for k, p in om.named_parameters()}
    assert len(want_g) == 142
    outs = _run(world, case, tmp_path)
    assert sum(o["n_score"] for o in outs) == g["src"].numel()
    for o in outs:
        assert _prob_diff(o["org"], org.detach()) < 1e-4 and _prob_diff(o["rev"], rev.detach()) < 1e-4
        assert abs(o["loss"].item() - want_loss.item()) < 1e-5
        check_grads(o["grads"], want_g, rtol=1e-3)
        for k, b in om.named_buffers():
            assert torch.allclose(o["buffers"][k].float(), b.float(), atol=1e-5, rtol=1e-4), k
        for li in range(8):
            assert o["buffers"][f"gnn.convs.{li}.bn_e.num_batches_tracked"].item() == 4
            assert o["buffers"][f"gnn.convs.{li}.bn_h.num_batches_tracked"].item() == 2
        assert o["plan_untouched"]
    for k in outs[0]["grads"]:   # identical on every rank: optimizers stay in step without a broadcast
        assert torch.equal(outs[0]["grads"][k], outs[-1]["grads"][k]), k


# 12 nodes in three ranges of four.  Rank 1's nodes 4..7 have out-edges ONLY into other ranges (their reversed in-runs hold nothing but
# cut edges); node 9 is a halo node of rank 0 through 0 -> 9 alone: a forward destination, so only ever a SOURCE in the reversed pass.
# Plus a self-loop (1 -> 1) and a duplicate edge (0 -> 1 twice).
HAND_EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (1, 1), (0, 1),
              (0, 4), (2, 5), (3, 6), (1, 7),
              (4, 8), (5, 9), (6, 10), (7, 11), (4, 9), (5, 0), (6, 2),
              (8, 9), (9, 10), (10, 11), (11, 8), (8, 4), (10, 7),
              (0, 9), (11, 3)]
HAND_BOUNDS = [0, 4, 8, 12]


def test_hand_graph_reversed_logits_are_bit_equal_between_one_and_three_ranks(tmp_path):
    """Every list of this graph whose order differs between the whole graph's numbering and a rank's (owned first, halo after) has at most
    two terms, so the checker backend forms every gated sum in the same association at world 1 and world 3.  What is left outside that
    argument is the backend's dense product, torch's `A @ W.t()` on 12 rows at world 1 and on 4 owned + the halo rows per rank: on an x86
    host whose BLAS picks its kernel by the row count the rows can differ in the last bit (seen once on another CPU: the first rank's
    logits unequal in bits, equal in the four digits printed) - the sums this test is about are not involved then."""
    from oracle.symgated_oracle import degree_features
    src = torch.tensor([a for a, _ in HAND_EDGES], dtype=torch.int32)
    dst = torch.tensor([b for _, b in HAND_EDGES], dtype=torch.int32)
    n = 12
    own = lambda t, r: (t >= HAND_BOUNDS[r]) & (t < HAND_BOUNDS[r + 1])  # noqa: E731
    assert not (own(src, 1) & own(dst, 1)).any() and own(src, 1).any() and own(dst, 1).any()       # rank 1: out-edges only to other ranks
    assert not ((src == 9) & own(dst, 0)).any() and ((dst == 9) & own(src, 0)).any()                 # node 9 on rank 0: a destination only
    gen = torch.Generator().manual_seed(12)
    case = dict(src=src, dst=dst, num_nodes=n, x=degree_features(src, dst, n), x_rev=degree_features(src, dst, n, reverse=True),
                e=torch.randn(len(HAND_EDGES), 2, generator=gen), hidden=64, layers=3, state_dict=random_state_dict(64, num_layers=3, seed=4))
    one = _run(1, dict(case, bounds=[0, n]), tmp_path / "one")[0]
    three = _run(3, dict(case, bounds=HAND_BOUNDS), tmp_path / "three")
    assert three[0]["n_local"] > three[0]["n_own"] and 9 in three[0]["node_gid"].tolist()
    assert sum(o["n_score"] for o in three) == len(HAND_EDGES)
    for o in three:
        assert torch.equal(o["rev"], one["rev"])
    assert not torch.equal(one["rev"], one["org"])


def test_local_degree_features_reverse_is_the_column_swap():
    """PartitionedGraph.local_degree_features(reverse=True) on a from_slices plan (world 1: no process group needed): the two columns of
    reverse=False exchanged bit for bit, the default argument unchanged."""
    from gnnome_amd.synth import make_graph
    from oracle.symgated_oracle import degree_features
    n, e = 300, 3000
    gr = make_graph(n, e, seed=8, kind="banded")
    part = gdist.PartitionedGraph.from_slices(gr["src"], gr["dst"], n, 0, 1, CPU, ops=cpu_ops)
    fwd, rev = part.local_degree_features(), part.local_degree_features(reverse=True)
    assert torch.equal(fwd, part.local_degree_features(reverse=False))
    assert torch.equal(rev, fwd[:, [1, 0]]) and rev.is_contiguous() and not torch.equal(rev, fwd)
    assert torch.allclose(rev, degree_features(gr["src"], gr["dst"], n, reverse=True), atol=2e-6, rtol=1e-6)


def test_refusals():
    from gnnome_amd.synth import make_graph
    from oracle.symgated_oracle import degree_features
    n, e = 60, 400
    gr = make_graph(n, e, seed=2, kind="banded")
    x = degree_features(gr["src"], gr["dst"], n)
    new = lambda **kw: gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], n, 0, 1, CPU, ops=cpu_ops, **kw)  # noqa: E731
    sym = gnnome_amd.models.SymGatedGCNModel(2, 2, 64, 16, 2, 64, "batch").eval()
    part = new()
    runner = gdist.PartitionedRunner(sym, part, x, gr["e"], CPU, ops=cpu_ops, x_rev_global=x[:, [1, 0]])
    with pytest.raises(NotImplementedError, match="CapturedPartitionedForward"):
        gdist.CapturedPartitionedForward(runner, reverse=True)
    with pytest.raises(NotImplementedError, match="CapturedPartitionedForward"):
        runner.capture(reverse=True)
    # the new path is selected by reverse=, not by flipping the plan: a flipped plan keeps the existing message
    flipped = new()
    flipped.views = flipped.views.reversed()
    for model in (sym, gnnome_amd.models.SymGatedGCNModel(2, 2, 64, 16, 2, 64, "batch").train()):
        with pytest.raises(NotImplementedError, match="^partitioned training runs on the forward orientation of the graph$"):
            gdist.PartitionedRunner(model, flipped, x, gr["e"], CPU, ops=cpu_ops)
    with pytest.raises(NotImplementedError, match="^partitioned training runs on the forward orientation of the graph$"):
        gdist.PartitionShard(flipped, cpu_ops, reverse=True)
    with pytest.raises(NotImplementedError, match="forward orientation"):
        gdist.run_partitioned(cpu_ops, engine.Prepared(sym, CPU), flipped, x, gr["e"], reverse=True)
    # a runner without x_rev cannot make the reversed pass
    with pytest.raises(ValueError, match="x_rev"):
        gdist.PartitionedRunner(sym, part, x, gr["e"], CPU, ops=cpu_ops).forward(reverse=True)
    # the one-direction model and the two sum / mean baselines stay on the forward orientation
    from gnnome_amd.models import GatedGCNModel, GCNModel
    gated = GatedGCNModel(2, 2, 64, 16, 2, 64, "batch").eval()
    with pytest.raises(NotImplementedError, match="forward orientation"):
        gdist.PartitionedRunner(gated, new(in_edges_only=True), x, gr["e"], CPU, ops=cpu_ops).forward(reverse=True)
    with pytest.raises(NotImplementedError, match="forward orientation"):
        gdist.PartitionedRunner(gated, new(in_edges_only=True), x, gr["e"], CPU, ops=cpu_ops, x_rev_global=x)
    gcn = GCNModel(2, 2, 64, 16, 2, 64, "batch").eval()
    with pytest.raises(NotImplementedError, match="forward orientation"):
        gdist.PartitionedRunner(gcn, part, x, gr["e"], CPU, ops=cpu_ops).forward(reverse=True)
    with pytest.raises(NotImplementedError, match="forward orientation"):
        gdist.PartitionedRunner(gcn, part, x, gr["e"], CPU, ops=cpu_ops).train_forward(reverse=True)
