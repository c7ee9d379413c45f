"""The doubled plan of GatedGCNModel(directed=False) - PartitionedGraph.from_global / from_slices(..., in_edges_only=True, doubled=True) -
as plan logic alone: CPU tensors, the checker backend of the gloo tests (tests/cpu_ops_gated.py), worlds 1, 2 and 3 on the fixed graph of
tests/gated_doubled_graphs.py.  No model runs here; the eval logits and the training step are test_dist_gated_doubled_gloo.py's."""
import pytest
import torch

import cpu_ops
import cpu_ops_gated
import gated_doubled_graphs as gdg
import gated_graphs as gg
from dist_gated_doubled_worker import plan_record, run_ranks, same_plan
from gnnome_amd import dist as gdist
from gnnome_amd import engine_gated
from gnnome_amd.models import GatedGCNModel, GCNModel, SymGatedGCNModel

BACKEND = cpu_ops_gated.BACKEND
DEV = torch.device("cpu")
_cache = {}


def _graph():
    if "graph" not in _cache:
        _cache["graph"] = gdg.graph()
    return _cache["graph"]


def _one_rank_plan(**kw):
    gr = _graph()
    return gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, DEV, ops=BACKEND, in_edges_only=True, **kw)


def _plans(world, tmp_path_factory):
    if world not in _cache:
        gr = _graph()
        if world == 1:
            part = _one_rank_plan(doubled=True)
            sl = gdist.PartitionedGraph.from_slices(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, DEV, ops=BACKEND, in_edges_only=True, doubled=True)
            rec = plan_record(part)
            rec.update(sliced_equal=bool(same_plan(sl, part) and torch.equal(sl.shuffle_edge_rows(gr["e"]), part.local_edge_rows(gr["e"]))),
                       default_bounds_equal=True, slice_degrees_are_the_original_graphs=True)
            _cache[world] = [rec]
        else:
            _cache[world] = run_ranks(world, dict(gr, plan_only=True), str(tmp_path_factory.mktemp(f"plan{world}")), timeout=120)
    return _cache[world]


def _whole_doubled():
    """Doubled(views) of the whole graph on the checker backend: per sorted position of the doubled views (dst, src, original edge)."""
    if "whole" not in _cache:
        gr = _graph()
        src, dst = gr["src"].long(), gr["dst"].long()
        views = cpu_ops.CpuViews(src, dst, gr["num_nodes"])
        dviews = cpu_ops.CpuViews(*engine_gated.doubled_edge_list(src, dst), gr["num_nodes"])
        enc_gather, score_gather = engine_gated.doubled_row_maps(dviews.srt_eid, views.srt_eid, views.num_edges)
        _cache["whole"] = dict(dst=dviews.srt_dst.long(), src=dviews.srt_src.long(), enc=enc_gather.long())
    return _cache["whole"]


def _keys(dst, src, enc, E):
    return torch.sort((dst.long() * gdg.N + src.long()) * E + enc.long()).values


def test_the_graph_holds_the_cases_it_is_named_for():
    gr = _graph()
    p = gdg.properties(gr)
    assert gr["num_nodes"] == 48 and 150 <= p["edges"] <= 170
    assert p["self_loops"] >= 1 and p["parallel"] >= 1 and p["sources_only"] >= 8
    for world in (2, 3):
        assert gdg.owner(gdg.CROSS[0], world) != gdg.owner(gdg.CROSS[1], world) and p[f"cut{world}"] > 0
        assert min(p[f"in_edges{world}"]) > 0                       # every rank owns in-edges of the doubled list ...
    assert p["scored3"][2] == 0 and min(p["scored3"][:2]) > 0       # ... and at world 3 the last rank's are all reverse copies
    assert min(p["scored2"]) > 0


def test_doubled_is_a_new_argument_valid_with_in_edges_only_alone():
    gr = _graph()
    with pytest.raises(ValueError, match="in_edges_only"):
        gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, DEV, ops=BACKEND, doubled=True)
    with pytest.raises(ValueError, match="in_edges_only"):
        gdist.PartitionedGraph.from_slices(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, DEV, ops=BACKEND, doubled=True)
    plain = _one_rank_plan()
    assert not plain.doubled and plain.enc_rows is None and plain.score_rows is None


@pytest.mark.parametrize("world", [1, 2, 3])
def test_every_doubled_edge_is_owned_once_and_every_original_edge_is_scored_once(world, tmp_path_factory):
    outs, E = _plans(world, tmp_path_factory), int(_graph()["src"].numel())
    assert all(o["doubled"] and o["num_edges_original"] == E and o["num_edges_global"] == 2 * E for o in outs)
    assert sum(o["n_own"] for o in outs) == gdg.N
    owned = torch.cat([o["srt_geid"][:o["n_score"]].long() for o in outs])
    assert torch.equal(torch.sort(owned).values, torch.arange(2 * E))
    assert torch.equal(torch.sort(torch.cat([o["edge_gid"] for o in outs])).values, torch.arange(2 * E))     # no edge is replicated
    scored = torch.cat([o["srt_geid"][o["score_rows"]].long() for o in outs])
    assert torch.equal(torch.sort(scored).values, torch.arange(E))
    for o in outs:
        assert o["n_score"] == o["e_local"] and o["n_score_original"] == o["score_rows"].numel()
        assert torch.equal(o["enc_rows"], o["edge_gid"] % E) and o["enc_rows"].dtype == torch.int64
        assert torch.equal(o["score_rows"], torch.nonzero(o["srt_geid"].long() < E).squeeze(1))             # ascending sorted positions
        assert int(o["in_degree_local"][o["n_own"]:].sum()) == 0                                             # halo nodes have empty in-lists
        assert o["sliced_equal"] and o["default_bounds_equal"] and o["slice_degrees_are_the_original_graphs"]
    if world == 3:
        assert outs[2]["n_score_original"] == 0 and outs[2]["n_score"] > 0
    # edge k lives with the owner of dst[k], its reverse copy with the owner of src[k]
    gr = _graph()
    for r, o in enumerate(outs):
        gid = o["edge_gid"]
        end = torch.where(gid < E, gr["dst"].long()[gid % E], gr["src"].long()[gid % E])
        assert bool(((end >= o["lo"]) & (end < o["hi"])).all()), r


@pytest.mark.parametrize("world", [1, 2, 3])
def test_every_owned_nodes_in_list_is_its_in_list_in_the_doubled_graph(world, tmp_path_factory):
    """As a multiset of (source, original edge) per destination: per rank, the (destination, source, original edge) triples of the local
    sorted order against those of Doubled(views) whose destination the rank owns."""
    outs, whole, E = _plans(world, tmp_path_factory), _whole_doubled(), int(_graph()["src"].numel())
    for o in outs:
        mine = (whole["dst"] >= o["lo"]) & (whole["dst"] < o["hi"])
        assert torch.equal(_keys(o["srt_dst"], o["srt_src"], o["srt_enc"], E), _keys(whole["dst"][mine], whole["src"][mine], whole["enc"][mine], E))
        assert bool(((o["srt_dst"] >= o["lo"]) & (o["srt_dst"] < o["hi"])).all())
    # the self-loop: both copies are in-edges of one node on one rank, one of them scored
    k = int(torch.nonzero((_graph()["src"] == gdg.LOOP[0]) & (_graph()["dst"] == gdg.LOOP[1])).squeeze(1)[0])
    holders = [o for o in outs if bool((o["edge_gid"] == k).any())]
    assert len(holders) == 1 and bool((holders[0]["edge_gid"] == E + k).any())
    ids = holders[0]["srt_geid"][holders[0]["score_rows"]].long()
    assert int((ids == k).sum()) == 1 and int((ids == E + k).sum()) == 0


def _model(cls=GatedGCNModel, **kw):
    m = cls(2, 2, gdg.HIDDEN, 16, gdg.LAYERS, gdg.SCORE_HIDDEN, "batch", dropout=0.0, **kw)
    if cls is GatedGCNModel:
        m.load_state_dict(gg.random_gated_state_dict(m, seed=8))
    return m


def test_refusals_are_raised_up_front():
    gr = _graph()
    dbl, plain = _one_rank_plan(doubled=True), _one_rank_plan()
    args = (gr["x"], gr["e"], DEV)
    # directed=False on a plan that is not doubled: today's refusal, now naming the plan to build
    with pytest.raises(NotImplementedError, match="directed=False.*doubled=True"):
        gdist.PartitionedRunner(_model(directed=False).eval(), plain, *args, ops=BACKEND)
    with pytest.raises(NotImplementedError, match="directed=False.*doubled=True"):
        gdist.run_partitioned(BACKEND, engine_gated.Prepared(_model(directed=False).eval(), DEV), plain, gr["x"], gr["e"])
    m = _model(directed=False).train()
    m.training_step = "in_edge"
    with pytest.raises(NotImplementedError, match="directed=False.*doubled=True"):
        engine_gated.train_forward_in_edge_on(m, gdist.PartitionShard(plain, BACKEND), plain.local_node_rows(gr["x"]), plain.local_edge_rows(gr["e"]))
    # directed=True on a doubled plan
    with pytest.raises(ValueError, match="directed=True"):
        gdist.PartitionedRunner(_model().eval(), dbl, *args, ops=BACKEND)
    with pytest.raises(ValueError, match="directed=True"):
        gdist.run_partitioned(BACKEND, engine_gated.Prepared(_model().eval(), DEV), dbl, gr["x"], gr["e"])
    m = _model().train()
    m.training_step = "in_edge"
    with pytest.raises(ValueError, match="directed=True"):
        engine_gated.train_forward_in_edge_on(m, gdist.PartitionShard(dbl, BACKEND), dbl.local_node_rows(gr["x"]), dbl.local_edge_rows(gr["e"]))
    # any other model class on a doubled plan
    for other in (_model(SymGatedGCNModel), _model(GCNModel)):
        with pytest.raises(ValueError, match="doubled"):
            gdist.PartitionedRunner(other.eval(), dbl, *args, ops=BACKEND)
    from gnnome_amd.models import GATModel
    with pytest.raises(ValueError, match="doubled"):
        gdist.GATPartitionedRunner(GATModel(2, 2, 64, 16, 1, 64, "batch").eval(), dbl, *args, ops=BACKEND)
    # what stays refused for this model on a partition: the captured forward, the symmetric-step adapter, bf16 storage, recompute_gate
    with pytest.raises(NotImplementedError, match="CapturedPartitionedForward"):
        gdist.PartitionedRunner(_model(directed=False).eval(), dbl, *args, ops=BACKEND).capture()
    m = _model(directed=False).train()
    assert m.training_step == "symmetric"
    with pytest.raises(NotImplementedError, match="training_step"):
        gdist.PartitionedRunner(m, dbl, *args, ops=BACKEND).train_forward()
    m.training_step = "in_edge"
    m.activation_storage = "bf16"
    with pytest.raises(ValueError, match="activation_storage"):
        gdist.PartitionedRunner(m, dbl, *args, ops=BACKEND).train_forward()
    m.activation_storage, m.recompute_gate = "fp32", True
    with pytest.raises(ValueError, match="recompute_gate"):
        gdist.PartitionedRunner(m, dbl, *args, ops=BACKEND).train_forward()
