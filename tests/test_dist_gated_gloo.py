"""GatedGCNModel on destination-range partitions, on the CPU: the in-edge-only partition, its halo plan and exchange over gloo, eval mode
and the in-edge training step, with the checker backend (tests/cpu_ops_gated.py) as compute - against the SINGLE-RANK GatedGCNModel on the
same backend.  World 2 and 3, uneven bounds, the graphs of tests/gated_partition_graphs.py.  The GPU twin is test_hip_gated_partition.py.

Bars (none of them chosen from what this code gives):
  eval logits   the bars of the symmetric model's partition tests: edge probabilities within 1e-5 of the single-rank forward
                (test_hip_partition.py::test_two_ranks_h256_banded_200k_edges_equals_one_rank; test_dist_gloo.py holds 1e-4 against the
                oracle) and EQUAL BITS on every rank (both files).
  training      the tolerances test_dist_gloo.py applies against the oracle's autograd for the same quantities: probabilities 1e-4, loss
                1e-5 absolute, every parameter gradient rtol 2e-3 of its largest entry (+ 2e-6), BatchNorm buffers atol 1e-5 / rtol 1e-4,
                gradients bit-equal on every rank.  Not bit equality with one rank: the batch statistics are merged by the
                parallel-variance formula and halo rows' gradients are added at their owners.
"""
import pytest
import torch
import torch.nn.functional as F

import cpu_ops
import cpu_ops_gated
import gated_graphs as gg
import gated_partition_graphs as gpg
from dist_gated_worker import run_ranks
from gnnome_amd import dist as gdist
from gnnome_amd import engine_gated
from gnnome_amd.models import GatedGCNModel
from test_train_host import check_grads

BACKEND = cpu_ops_gated.BACKEND
CASES = [(name, world) for name in gpg.GRAPHS for world in (2, 3)]
_cache = {}


def _model(directed=True):
    m = GatedGCNModel(2, 2, gpg.HIDDEN, 16, gpg.LAYERS, gpg.SCORE_HIDDEN, "batch", dropout=0.0, directed=directed)
    m.load_state_dict(gg.random_gated_state_dict(m, seed=8))
    return m


def _graph(name):
    if name not in _cache:
        _cache[name] = gpg.GRAPHS[name]()
    return _cache[name]


def _single_rank(name):
    """The single-rank GatedGCNModel on the checker backend: eval logits, and the in-edge step's logits, loss, gradients, buffers."""
    key = (name, "one")
    if key not in _cache:
        gr = _graph(name)
        views = cpu_ops.CpuViews(gr["src"], gr["dst"], gr["num_nodes"])
        m = _model().eval()
        with torch.no_grad():
            logits = engine_gated.run_stack(BACKEND, engine_gated.Prepared(m, torch.device("cpu")), views, gr["x"], gr["e"])
        m.train()
        names, params = zip(*m.named_parameters())
        out = engine_gated._InEdgeStep.apply(m, engine_gated._StepGraph(views, True, ops=BACKEND), gr["x"], gr["e"], list(names), *params)
        loss = F.binary_cross_entropy_with_logits(out.squeeze(-1), gr["y"], pos_weight=gr["pos_weight"])
        loss.backward()
        _cache[key] = dict(logits=logits, train_logits=out.detach().squeeze(1), loss=loss.detach(), views=views,
                           grads={k: p.grad.clone() for k, p in m.named_parameters()}, buffers={k: b.clone() for k, b in m.named_buffers()})
    return _cache[key]


@pytest.fixture
def ranks(request, tmp_path_factory):
    """What every rank of a (graph, world) pair computed - one spawn per pair, shared by the tests below."""
    name, world = request.param
    if (name, world) not in _cache:
        gr = _graph(name)
        case = dict(gr, state_dict=_model().state_dict())
        _cache[(name, world)] = run_ranks(world, case, str(tmp_path_factory.mktemp(f"{name}{world}")), timeout=120)
    return name, world, _cache[(name, world)]


def test_the_graphs_hold_the_cases_they_are_named_for():
    mixed2, mixed3 = gpg.properties(_graph("mixed"), 2), gpg.properties(_graph("mixed"), 3)
    assert mixed3["zero_in_degree"] >= 1 and mixed3["all_sources_remote"] >= 1 and mixed2["all_sources_remote"] >= 1
    assert mixed3["parallel"] >= 2 and mixed3["self_loops"] >= 1 and 64 < mixed3["max_in_degree"] < 4096
    assert mixed3["rank_pairs"] == 9 and mixed2["rank_pairs"] == 4          # edges between every ordered pair of ranks
    for world in (2, 3):
        assert gpg.properties(_graph("island"), world)["halo_rows"][0] == 0 and min(gpg.properties(_graph("island"), world)["halo_rows"][1:]) > 0
        star = gpg.properties(_graph("star"), world)
        assert star["max_in_degree"] > 4096 and min(star["halo_rows"]) > 0   # the two-level list is fed through the halo
    assert 48 <= _graph("island")["num_nodes"] <= 200 and 48 <= _graph("mixed")["num_nodes"] <= 200
    assert all(len(set(b[i + 1] - b[i] for i in range(len(b) - 1))) > 1 for b in _graph("mixed")["bounds"].values())   # uneven ranges


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_the_local_graph_is_the_owned_in_edges_in_global_order_with_the_remote_sources_as_halo(ranks):
    name, world, outs = ranks
    gr, one = _graph(name), _single_rank(name)
    E = int(gr["src"].numel())
    assert sum(o["n_own"] for o in outs) == gr["num_nodes"]
    assert sum(o["e_local"] for o in outs) == E and all(o["n_score"] == o["e_local"] for o in outs)     # no edge is replicated
    # destination runs in range order, ascending edge id inside a run: the ranks' sorted orders laid end to end are the whole graph's
    assert torch.equal(torch.cat([o["srt_geid"] for o in outs]).long(), one["views"].srt_eid.long())
    census = gdist.partition_census(gr["src"], gr["dst"], gr["num_nodes"], world, bounds=gr["bounds"][world])
    want_halo = gpg.properties(gr, world)["halo_rows"]
    for o, r, halo in zip(outs, census["ranks"], want_halo):
        assert o["n_local"] - o["n_own"] == halo == r["in_edge_halo_rows"] == sum(o["recv"])
        assert o["e_local"] == r["in_edge_local_edges"] and sum(o["send"]) == r["in_edge_rows_sent_per_layer"]
        assert r["in_edge_halo_rows"] <= r["halo_rows"] and r["in_edge_local_edges"] <= r["local_edges"]
        assert int(o["in_degree_local"][o["n_own"]:].sum()) == 0                                       # halo nodes have empty in-lists
    assert all(o["sliced_equal"] for o in outs)                                                        # from_slices builds the same plan


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_eval_logits_equal_the_single_rank_model(ranks):
    name, world, outs = ranks
    want = _single_rank(name)["logits"]
    for o in outs:
        assert o["logits"].shape == want.shape
        assert (torch.sigmoid(o["logits"]) - torch.sigmoid(want)).abs().max().item() < 1e-5
        assert torch.equal(o["logits"], outs[0]["logits"])              # every rank holds the full result, the same bits


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_in_edge_training_step_matches_the_single_rank_step(ranks):
    name, world, outs = ranks
    one = _single_rank(name)
    for o in outs:
        assert (torch.sigmoid(o["train_logits"]) - torch.sigmoid(one["train_logits"])).abs().max().item() < 1e-4
        assert abs(o["loss"].item() - one["loss"].item()) < 1e-5
        check_grads(o["grads"], one["grads"], rtol=2e-3)
        assert set(o["buffers"]) == set(one["buffers"])
        for k, want in one["buffers"].items():
            assert torch.allclose(o["buffers"][k].float(), want.float(), atol=1e-5, rtol=1e-4), k
    for k in outs[0]["grads"]:   # identical on every rank: optimizers stay in step without a broadcast
        assert all(torch.equal(outs[0]["grads"][k], o["grads"][k]) for o in outs[1:]), k


def test_the_single_rank_step_is_itself_right():
    """The reference the partitioned runs are held to, against torch autograd over the plain-torch restatement (gated_graphs.gated_model)."""
    gr, one = _graph("mixed"), _single_rank("mixed")
    leaves = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in _model().state_dict().items()}
    want = gg.gated_model(leaves, gr["src"], gr["dst"], gr["num_nodes"], gr["x"], gr["e"], gpg.LAYERS, training=True)
    F.binary_cross_entropy_with_logits(want.squeeze(-1), gr["y"], pos_weight=gr["pos_weight"]).backward()
    assert (torch.sigmoid(one["train_logits"]) - torch.sigmoid(want.detach().squeeze(1))).abs().max().item() < 1e-5
    check_grads(one["grads"], {k: leaves[k].grad for k in one["grads"]}, rtol=1e-3)


def test_refused_cases_raise_up_front():
    gr = _graph("island")
    dev = torch.device("cpu")
    part = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND, in_edges_only=True)
    full = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND)
    assert part.in_edges_only and not full.in_edges_only
    with pytest.raises(NotImplementedError, match="directed=False"):
        gdist.PartitionedRunner(_model(directed=False).eval(), part, gr["x"], gr["e"], dev, ops=BACKEND)
    with pytest.raises(NotImplementedError, match="directed=False"):
        gdist.run_partitioned(BACKEND, engine_gated.Prepared(_model(directed=False).eval(), dev), part, gr["x"], gr["e"])
    m = _model().train()
    assert m.training_step == "symmetric"
    with pytest.raises(NotImplementedError, match="training_step"):
        gdist.PartitionedRunner(m, part, gr["x"], gr["e"], dev, ops=BACKEND).train_forward()
    with pytest.raises(ValueError, match="in_edges_only"):      # the one-direction model on a partition that also holds out-edges
        gdist.PartitionedRunner(_model().eval(), full, gr["x"], gr["e"], dev, ops=BACKEND)
    from gnnome_amd.models import SymGatedGCNModel
    with pytest.raises(ValueError, match="in-edge-only"):        # ... and the symmetric model on one that lacks them
        gdist.PartitionedRunner(SymGatedGCNModel(2, 2, 64, 16, 1, 64, "batch").eval(), part, gr["x"], gr["e"], dev, ops=BACKEND)
    with pytest.raises(NotImplementedError, match="CapturedPartitionedForward"):
        gdist.PartitionedRunner(_model().eval(), part, gr["x"], gr["e"], dev, ops=BACKEND).capture()
    with pytest.raises(ValueError, match="bounds"):
        gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND, bounds=[0, 5])


def test_one_rank_on_an_in_edge_partition_equals_the_plain_model():
    """World 1 takes the single-process route of the step (no collective, the whole-graph entries): the same bits as the plain model."""
    gr, one = _graph("island"), _single_rank("island")
    dev = torch.device("cpu")
    part = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND, in_edges_only=True)
    logits = gdist.PartitionedRunner(_model().eval(), part, gr["x"], gr["e"], dev, ops=BACKEND).forward().squeeze(1)
    assert torch.equal(logits, one["logits"])
    m = _model().train()
    m.training_step = "in_edge"
    out = gdist.PartitionedRunner(m, part, gr["x"], gr["e"], dev, ops=BACKEND).train_forward()
    F.binary_cross_entropy_with_logits(out.squeeze(-1), gr["y"], pos_weight=gr["pos_weight"]).backward()
    assert torch.equal(out.detach().squeeze(1), one["train_logits"])
    assert all(torch.equal(p.grad, one["grads"][k]) for k, p in m.named_parameters())


def test_header_ctypes_table_and_exports_agree_on_the_partition_entries():
    import ctypes
    import re
    import subprocess

    import header_binding
    from gnnome_amd import _lib
    names = ("gnnome_node_aggregate_in_raw_part_f32", "gnnome_node_aggregate_in_bwd_part_f32")
    header = open(_lib.HEADER_PATH).read()
    parsed = header_binding.parse_header(_lib.HEADER_PATH)
    kind = lambda t: "ptr" if t in (ctypes.c_void_p,) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)) else t  # noqa: E731
    lib = header_binding.bind(_lib.LIB_PATH, _lib.HEADER_PATH)
    exported = set(re.findall(r" T (gnnome_\w+)", subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                                                                  check=True).stdout))
    assert exported == set(parsed), sorted(exported ^ set(parsed))      # nm -D exports match the header
    for name in names:
        assert [kind(t) for t in parsed[name][1]] == [kind(t) for t in _lib.SIGNATURES[name]], name
        assert hasattr(lib, name) and name in exported
    assert "gated_gcn_full.py:182-230" in header and lib.gnnome_abi_version() == _lib.ABI_VERSION == 32
    # argument validation runs before anything touches the device
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)
    assert lib.gnnome_node_aggregate_in_raw_part_f32(None, 64, 0, 0, None, None, 256, None, None, None, None, None, None) == 0       # no rows: a no-op
    assert lib.gnnome_node_aggregate_in_raw_part_f32(one, 64, 5, 4, one, one, 256, one, one, two, two, two, None) == -1
    assert b"5 destination rows of 4 local rows" in lib.gnnome_last_error()
    assert lib.gnnome_node_aggregate_in_raw_part_f32(one, 96, 4, 5, one, one, 96, one, one, two, two, two, None) == -1
    assert b"hidden=96" in lib.gnnome_last_error()
    assert lib.gnnome_node_aggregate_in_bwd_part_f32(one, 3, 64, 5, 4, one, one, one, 256, one, one, one, one, one, two, two, None) == -1
    assert b"5 destination rows of 4 local rows" in lib.gnnome_last_error()
    assert lib.gnnome_node_aggregate_in_bwd_part_f32(one, 3, 64, 0, 4, one, one, one, 256, one, one, one, one, one, two, two, None) == -1
    assert b"no destination row" in lib.gnnome_last_error()
    assert lib.gnnome_node_aggregate_in_bwd_part_f32(None, 0, 64, 0, 0, None, None, None, 256, None, None, None, None, None, None, None, None) == 0
