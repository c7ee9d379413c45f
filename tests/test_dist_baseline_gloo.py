"""GCNModel and SAGEModel on destination-range partitions, on the CPU: the scale exchange, the interior / boundary row lists, the out-lists
in the whole graph's order, eval mode and the training step over gloo with the checker backend (tests/cpu_ops_baselines.py) as compute -
against the SINGLE-RANK sequences of engine_baselines on the same backend.  World 2 and 3, uneven bounds, the graphs of
tests/gated_partition_graphs.py.  The GPU twin is test_hip_baseline_partition.py.

Bars (the project's existing ones for partitioned runs, none chosen from what this code gives):
  eval logits   edge probabilities within 1e-5 of the single-rank forward, EQUAL BITS on every rank (test_hip_partition.py's eval bars).
  training      test_hip_partition.py::_check_partitioned_step's: probabilities 1e-4, loss 1e-5, every gradient rtol 3e-2 of its largest
                entry, the whole gradient 3e-3 in relative L2, gradients bit-equal on every rank.
  scales        the halo rows' scales EQUAL the whole graph's (degrees are integers below 2^24: exact as float32, same formulas).
"""
import pytest
import torch
import torch.nn.functional as F

import baseline_partition_graphs as bpg
import cpu_ops_baselines
from dist_baseline_worker import CONFIGS, run_ranks
from gnnome_amd import dist as gdist
from gnnome_amd import engine_baselines as eb
from test_train_host import check_grads

BACKEND = cpu_ops_baselines.BACKEND
CASES = [(name, world) for name in bpg.GRAPHS for world in (2, 3)]
_cache = {}


def _graph(name):
    if name not in _cache:
        _cache[name] = bpg.GRAPHS[name]()
    return _cache[name]


def _single_rank(name, config):
    """engine_baselines' single-rank sequences on the checker backend: eval logits, and the step's logits, loss and gradients."""
    key = (name, config)
    if key not in _cache:
        kind, directed, dropout = config
        gr = _graph(name)
        views = cpu_ops_baselines.Views(gr["src"], gr["dst"], gr["num_nodes"])
        m = bpg.model(kind, directed, dropout).eval()
        with torch.no_grad():
            logits = eb.run_stack(BACKEND, eb.Prepared(m, torch.device("cpu")), views, gr["x"], gr["e"], directed)
        m.train()
        masks = bpg.known_masks(gr, dropout) if dropout > 0 else [None] * bpg.LAYERS
        out, kept = eb._step_forward(BACKEND, m, views, gr["x"], gr["e"], masks)
        leaf = out.clone().requires_grad_(True)
        loss = F.binary_cross_entropy_with_logits(leaf, gr["y"], pos_weight=gr["pos_weight"])
        loss.backward()
        grads = eb._step_backward(BACKEND, m, views, gr["x"], gr["e"], kept, leaf.grad)
        _cache[key] = dict(logits=logits, train_logits=out, loss=loss.detach(), grads={k: grads[k] for k, _ in m.named_parameters()})
    return _cache[key]


@pytest.fixture
def ranks(request, tmp_path_factory):
    """What every rank of a (graph, world) pair computed - one spawn per pair, shared by the tests below."""
    name, world = request.param
    if (name, world) not in _cache:
        _cache[(name, world)] = run_ranks(world, dict(_graph(name)), str(tmp_path_factory.mktemp(f"{name}{world}")), timeout=180)
    return name, world, _cache[(name, world)]


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_halo_scales_equal_the_whole_graphs_scales_exactly(ranks):
    name, world, outs = ranks
    gr = _graph(name)
    for directed in (True, False):
        want = dict(zip(("din_rsqrt", "dout_rsqrt", "din_inv"), bpg.whole_scales(gr, directed)))
        views = cpu_ops_baselines.Views(gr["src"], gr["dst"], gr["num_nodes"])
        single = eb.Scales(views, directed)
        for o in outs:
            assert o["n_local"] > o["n_own"] or name == "island"
            for k, w in want.items():
                got = o["configs"][("gcn", directed, 0.0)]["plan"][k]
                assert got.shape == (o["n_local"],)
                assert torch.equal(got, w[o["node_gid"]]), (k, directed)
                assert torch.equal(got, getattr(single, k)[o["node_gid"]])


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_interior_and_boundary_rows_partition_the_owned_rows(ranks):
    name, world, outs = ranks
    some_boundary = some_interior = False
    for o in outs:
        n_own = o["n_own"]
        for directed in (True, False):
            c = o["configs"][("sage", directed, 0.0)]
            ls = c["lists"]
            for which, walked in (("rows_fwd", [("in_ptr", "srt_src")] + ([] if directed else [("out_ptr", "out_dst")])),
                                  ("rows_bwd", [("out_ptr", "out_dst")] + ([] if directed else [("in_ptr", "srt_src")]))):
                interior, boundary = c[which]
                assert interior.dtype == boundary.dtype == torch.int32
                assert torch.equal(torch.sort(torch.cat([interior, boundary])).values.long(), torch.arange(n_own))   # disjoint, cover [0, n_own)
                for ptr, idx in walked:
                    for i in interior.tolist():
                        assert bool((ls[idx][int(ls[ptr][i]):int(ls[ptr][i + 1])] < n_own).all())
                # a boundary row IS one: some walked list names a halo id
                for i in boundary.tolist():
                    assert any(bool((ls[idx][int(ls[ptr][i]):int(ls[ptr][i + 1])] >= n_own).any()) for ptr, idx in walked)
                some_boundary |= boundary.numel() > 0
                some_interior |= interior.numel() > 0
    assert some_boundary and some_interior


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_the_owned_lists_are_the_whole_graphs_lists_in_its_order(ranks):
    """What bit equality rests on: an owned node's in-list and out-list name the whole graph's neighbours in the whole graph's order."""
    name, world, outs = ranks
    gr = _graph(name)
    whole = cpu_ops_baselines.Views(gr["src"], gr["dst"], gr["num_nodes"])
    for o in outs:
        ls, gid = o["configs"][("gcn", True, 0.0)]["lists"], o["node_gid"]
        for ptr, idx in (("in_ptr", "srt_src"), ("out_ptr", "out_dst")):
            wp, wi = getattr(whole, ptr), getattr(whole, idx)
            a, b = int(wp[o["lo"]]), int(wp[o["hi"]])
            assert torch.equal((wp[o["lo"]:o["hi"] + 1] - a).int(), ls[ptr][:o["n_own"] + 1])
            assert torch.equal(gid[ls[idx][:b - a].long()], wi[a:b].long()), idx


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_eval_logits_equal_the_single_rank_model(ranks):
    name, world, outs = ranks
    for config in CONFIGS:
        if config[2] > 0:
            continue
        want = _single_rank(name, config)["logits"]
        for o in outs:
            c = o["configs"][config]
            assert c["logits"].shape == want.shape
            assert (torch.sigmoid(c["logits"]) - torch.sigmoid(want)).abs().max().item() < 1e-5, config
            assert torch.equal(c["logits"], outs[0]["configs"][config]["logits"])       # every rank holds the full result, the same bits
            assert torch.equal(c["logits_split"], c["logits"])                            # the row-list launches change nothing


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_training_step_matches_the_single_rank_step(ranks):
    name, world, outs = ranks
    for config in CONFIGS:
        one = _single_rank(name, config)
        for o in outs:
            c = o["configs"][config]
            assert (torch.sigmoid(c["train_logits"]) - torch.sigmoid(one["train_logits"])).abs().max().item() < 1e-4, config
            assert abs(c["loss"].item() - one["loss"].item()) < 1e-5, config
            check_grads(c["grads"], one["grads"], rtol=3e-2)
            num = sum(((c["grads"][k] - w).double() ** 2).sum().item() for k, w in one["grads"].items()) ** 0.5
            den = sum((w.double() ** 2).sum().item() for w in one["grads"].values()) ** 0.5
            assert num / den < 3e-3, f"{config}: relative L2 error of the full gradient {num / den:.2e}"
        for k in outs[0]["configs"][config]["grads"]:
            assert all(torch.equal(outs[0]["configs"][config]["grads"][k], o["configs"][config]["grads"][k]) for o in outs[1:]), (config, k)


def test_the_single_rank_step_is_itself_right():
    """The reference the partitioned runs are held to, against torch autograd over the plain-torch restatement (baseline_graphs)."""
    import baseline_graphs as bg
    gr = _graph("mixed")
    for config in CONFIGS:
        kind, directed, dropout = config
        if dropout > 0:
            continue
        one = _single_rank("mixed", config)
        leaves = {k: v.clone().requires_grad_(True) for k, v in bpg.model(kind, directed).state_dict().items()}
        want = bg.baseline_model(kind, leaves, gr["src"], gr["dst"], gr["num_nodes"], gr["x"], gr["e"], bpg.LAYERS, directed)
        F.binary_cross_entropy_with_logits(want.squeeze(-1), gr["y"], pos_weight=gr["pos_weight"]).backward()
        assert (torch.sigmoid(one["train_logits"]) - torch.sigmoid(want.detach().squeeze(1))).abs().max().item() < 1e-5
        check_grads(one["grads"], {k: leaves[k].grad for k in one["grads"]}, rtol=1e-3)


def test_refused_cases_raise_up_front():
    from gnnome_amd.models import GATModel
    gr = _graph("island")
    dev = torch.device("cpu")
    full = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND)
    in_only = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND, in_edges_only=True)
    for kind in bpg.KINDS:
        with pytest.raises(ValueError, match="out-lists"):
            gdist.PartitionedRunner(bpg.model(kind).eval(), in_only, gr["x"], gr["e"], dev, ops=BACKEND)
        with pytest.raises(ValueError, match="in_edges_only"):
            gdist.run_partitioned(BACKEND, eb.Prepared(bpg.model(kind).eval(), dev), in_only, gr["x"], gr["e"])
        with pytest.raises(NotImplementedError, match="CapturedPartitionedForward"):
            gdist.PartitionedRunner(bpg.model(kind).eval(), full, gr["x"], gr["e"], dev, ops=BACKEND).capture()
        with pytest.raises(ValueError, match="out-lists"):
            eb.train_forward_on(bpg.model(kind).train(), gdist.PartitionShard(in_only, BACKEND), gr["x"], gr["e"])
        flipped = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND)
        flipped.views = flipped.views.reversed()
        with pytest.raises(NotImplementedError, match="forward orientation"):
            gdist.PartitionedRunner(bpg.model(kind).eval(), flipped, gr["x"], gr["e"], dev, ops=BACKEND)
        empty = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND)
        empty.n_own = 0
        with pytest.raises(NotImplementedError, match="without owned nodes"):
            gdist.PartitionedRunner(bpg.model(kind).eval(), empty, gr["x"], gr["e"], dev, ops=BACKEND)
    with pytest.raises(NotImplementedError, match="GATModel is not served on partitions"):
        gdist.PartitionedRunner(GATModel(2, 2, 64, 16, 2, 32, "batch").eval(), full, gr["x"], gr["e"], dev, ops=BACKEND)
    with pytest.raises(TypeError, match="GCNModel and SAGEModel"):
        eb.train_forward_on(GATModel(2, 2, 64, 16, 2, 32, "batch"), gdist.PartitionShard(full, BACKEND), gr["x"], gr["e"])


def test_a_degree_that_float32_cannot_hold_is_refused():
    """The bound is on the degrees of g' as they are formed in float32: in + 1 and out + 1, or in + out + 1 - a bound equal to the largest
    of them is accepted, one below it refused, and the doubled graph's sum is refused where neither term alone would be."""
    gr = _graph("island")
    dev = torch.device("cpu")
    din = torch.bincount(gr["dst"].long(), minlength=gr["num_nodes"])
    dout = torch.bincount(gr["src"].long(), minlength=gr["num_nodes"])
    top_directed, top_doubled = int(torch.maximum(din, dout).max()) + 1, int((din + dout).max()) + 1
    assert top_doubled > top_directed
    keep = eb.MAX_EXACT_DEGREE
    try:
        for directed, top in ((True, top_directed), (False, top_doubled)):
            for bound, refused in ((top, False), (top - 1, True)):
                part = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND)
                eb.MAX_EXACT_DEGREE = bound
                if refused:
                    with pytest.raises(ValueError, match="float32"):
                        eb.plan_for(BACKEND, part, directed)
                else:
                    eb.plan_for(BACKEND, part, directed)
        part = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND)
        eb.MAX_EXACT_DEGREE = top_directed          # no single in- or out-degree passes it; the doubled graph's sum does
        eb.plan_for(BACKEND, part, True)
        with pytest.raises(ValueError, match="doubled"):
            eb.plan_for(BACKEND, part, False)
    finally:
        eb.MAX_EXACT_DEGREE = keep
    assert eb.MAX_EXACT_DEGREE == 1 << 24 and float(torch.tensor(1 << 24, dtype=torch.float32)) == float(1 << 24)


def test_one_rank_equals_the_plain_sequences_bit_for_bit():
    """World 1: no collective, no halo, every row interior - the checker backend's sums are then the single-rank ones term for term."""
    gr = _graph("island")
    dev = torch.device("cpu")
    for config in CONFIGS:
        kind, directed, dropout = config
        if dropout > 0:
            continue
        one = _single_rank("island", config)
        part = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, ops=BACKEND)
        logits = gdist.PartitionedRunner(bpg.model(kind, directed).eval(), part, gr["x"], gr["e"], dev, ops=BACKEND).forward().squeeze(1)
        assert torch.equal(logits, one["logits"]), config
        m = bpg.model(kind, directed).train()
        out = gdist.PartitionedRunner(m, part, gr["x"], gr["e"], dev, ops=BACKEND).train_forward()
        F.binary_cross_entropy_with_logits(out.squeeze(-1), gr["y"], pos_weight=gr["pos_weight"]).backward()
        assert torch.equal(out.detach().squeeze(1), one["train_logits"]), config
        check_grads({k: p.grad for k, p in m.named_parameters()}, one["grads"], rtol=1e-5)


def test_header_ctypes_table_and_exports_agree_on_the_partition_entries():
    import ctypes
    import re
    import subprocess

    import header_binding
    from gnnome_amd import _lib
    names = ("gnnome_node_neighbour_sum_part_f32", "gnnome_node_neighbour_sum_bwd_part_f32")
    header = open(_lib.HEADER_PATH).read()
    parsed = header_binding.parse_header(_lib.HEADER_PATH)
    kind = lambda t: "ptr" if t in (ctypes.c_void_p,) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)) else t  # noqa: E731
    lib = header_binding.bind(_lib.LIB_PATH, _lib.HEADER_PATH)
    exported = set(re.findall(r" T (gnnome_\w+)", subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                                                                  check=True).stdout))
    for name in names:
        assert [kind(t) for t in parsed[name][1]] == [kind(t) for t in _lib.SIGNATURES[name]], name
        assert hasattr(lib, name) and name in exported
    for cite in ("models/full_graph.py:56-75", "full_graph.py:100-119", "layers/processor.py:35-46", "processor.py:73-84"):
        assert cite in header[header.index("on one rank's shard of a destination-range partition"):], cite
    # argument validation runs before anything touches the device
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)
    fwd, bwd = lib.gnnome_node_neighbour_sum_part_f32, lib.gnnome_node_neighbour_sum_bwd_part_f32
    assert fwd(one, 64, 64, 5, 4, None, 0, one, one, None, None, None, None, two, 64, None) == -1
    assert b"5 destination rows of 4 local rows" in lib.gnnome_last_error()
    assert fwd(one, 96, 96, 4, 5, None, 0, one, one, None, None, None, None, two, 96, None) == -1
    assert b"hidden=96" in lib.gnnome_last_error()
    assert fwd(None, 64, 64, 4, 5, None, 0, one, one, None, None, None, None, two, 64, None) == -1
    assert b"null pointer" in lib.gnnome_last_error()
    assert fwd(one, 64, 64, 4, 5, one, 0, one, one, None, None, None, None, two, 64, None) == 0          # an empty row list: nothing is launched
    assert fwd(None, 64, 64, 0, 5, None, 0, None, None, None, None, None, None, None, 64, None) == 0      # no owned row: a no-op
    assert bwd(one, 64, 64, 5, 4, None, 0, one, one, None, None, 0, None, None, None, 0, None, 0, None, 0, two, 64, None) == -1
    assert b"5 destination rows of 4 local rows" in lib.gnnome_last_error()
    assert bwd(one, 96, 96, 4, 5, None, 0, one, one, None, None, 0, None, None, None, 0, None, 0, None, 0, two, 96, None) == -1
    assert b"hidden=96" in lib.gnnome_last_error()
    assert bwd(one, 64, 64, 4, 5, None, 0, None, one, None, None, 0, None, None, None, 0, None, 0, None, 0, two, 64, None) == -1
    assert b"null pointer" in lib.gnnome_last_error()
    assert bwd(one, 64, 64, 4, 5, one, 0, one, one, None, None, 0, None, None, None, 0, None, 0, None, 0, two, 64, None) == 0
