"""engine.score_tail and engine.scored_rows, the one scorer tail of every sequence on a destination-range partition, and
PartitionedGraph.scored, the one description of what a rank scores - without a GPU and without a process group: a stub backend records
the edge_score / gather_rows calls, and the assembly of the logits is a callable the test hands in."""
import types

import pytest
import torch

import cpu_ops_gated
import gated_partition_graphs as gpg
from gnnome_amd import dist as gdist
from gnnome_amd import engine

W_TAIL = tuple(object() for _ in range(5))     # W1_e, W2, b2, W3, b3: the tail hands them on, in this order
VIEWS = types.SimpleNamespace(name="score views")


class RecordingOps:
    """A backend that records every edge_score and gather_rows call and computes nothing."""

    def __init__(self):
        self.scores, self.gathers = [], []

    def edge_score(self, e, Ps, Qd, views, *rest, **kw):
        self.scores.append(dict(e=e, Ps=Ps, Qd=Qd, views=views, tail=rest[:5], out=rest[5], extra=rest[6:], kw=kw))
        return rest[5]

    def gather_rows(self, table, idx):
        self.gathers.append((table, idx))
        return table[idx.long()]


def _inputs(rows):
    return torch.zeros(rows, 4), torch.zeros(6, 2), torch.ones(6, 2)


def _assembler(result):
    seen = []

    def assemble(piece):
        seen.append(piece)
        return result

    return seen, assemble


@pytest.mark.parametrize("keep_z1", [False, True])
def test_a_lone_process_scatters_to_the_edge_ids_itself(keep_z1):
    ops = RecordingOps()
    e, Ps, Qd = _inputs(5)
    z1 = torch.empty(5, 2) if keep_z1 else None
    out = engine.score_tail(ops, e, Ps, Qd, W_TAIL, VIEWS, 5, 7, z1_out=z1)
    assert len(ops.scores) == 1
    call = ops.scores[0]
    assert out is call["out"] and out.shape == (7,) and out.dtype == torch.float32
    assert call["e"] is e and call["Ps"] is Ps and call["Qd"] is Qd and call["views"] is VIEWS
    assert call["tail"] == W_TAIL and call["extra"] == ()
    assert "scatter_to_edge_id" not in call["kw"]                     # left at its default: the kernel scatters
    assert call["kw"].pop("num_edges") == 5
    if keep_z1:
        assert call["kw"].pop("z1_out") is z1
    assert call["kw"] == {}                                           # nothing else is passed, z1_out only when given


def test_one_rank_of_several_scores_its_piece_and_assembles():
    ops = RecordingOps()
    e, Ps, Qd = _inputs(3)
    z1, complete = torch.empty(3, 2), torch.zeros(9)
    seen, assemble = _assembler(complete)
    out = engine.score_tail(ops, e, Ps, Qd, W_TAIL, VIEWS, 3, 9, z1_out=z1, pad=4, assemble=assemble)
    assert out is complete                                            # what assemble returned
    assert len(ops.scores) == 1 and len(seen) == 1
    call = ops.scores[0]
    assert seen[0] is call["out"] and seen[0].shape == (4,) and seen[0].dtype == torch.float32
    assert call["e"] is e and call["Ps"] is Ps and call["Qd"] is Qd and call["views"] is VIEWS and call["tail"] == W_TAIL
    assert call["kw"] == dict(num_edges=3, scatter_to_edge_id=False, z1_out=z1) and call["kw"]["z1_out"] is z1


def test_a_rank_that_scores_nothing_launches_nothing_and_still_assembles():
    ops = RecordingOps()
    e, Ps, Qd = _inputs(0)
    complete = torch.zeros(9)
    seen, assemble = _assembler(complete)
    out = engine.score_tail(ops, e, Ps, Qd, W_TAIL, VIEWS, 0, 9, z1_out=torch.empty(0, 2), pad=1, assemble=assemble)
    assert ops.scores == []
    assert len(seen) == 1 and seen[0].shape == (1,) and out is complete


def test_the_row_selector():
    ops = RecordingOps()
    e = torch.arange(12.0).reshape(6, 2)
    assert engine.scored_rows(ops, e, None, 6) is e and ops.gathers == []          # the sorted prefix as it lies
    none = engine.scored_rows(ops, e, torch.zeros(0, dtype=torch.int32), 0)
    assert none.shape == (0, 2) and ops.gathers == []                              # no rows, no launch
    rows = torch.tensor([4, 1], dtype=torch.int32)
    assert torch.equal(engine.scored_rows(ops, e, rows, 2), e[[4, 1]])
    assert len(ops.gathers) == 1 and ops.gathers[0][0] is e and ops.gathers[0][1] is rows


def _mixed_plan(**kw):
    gr = gpg.mixed()
    assert gr["num_nodes"] == 60
    part = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, torch.device("cpu"), ops=cpu_ops_gated.BACKEND, **kw)
    return gr, part


@pytest.mark.parametrize("in_edges_only", [False, True])
def test_scored_on_a_plain_plan_is_the_sorted_prefix(in_edges_only):
    gr, part = _mixed_plan(in_edges_only=in_edges_only)
    sc = part.scored
    assert sc.count == part.n_score == int(gr["src"].numel()) and sc.total == part.num_edges_global == sc.count
    assert sc.rows is None and sc.views is part.views
    sv = sc.score_views
    assert sv.srt_src is part.views.srt_src and sv.srt_dst is part.views.srt_dst and sv.srt_eid is part.srt_geid


def test_scored_on_a_doubled_plan_is_the_original_edges():
    gr, part = _mixed_plan(in_edges_only=True, doubled=True)
    E = int(gr["src"].numel())
    sc = part.scored
    assert part.n_score == part.num_edges_global == 2 * E
    assert sc.count == part.n_score_original == E and sc.total == part.num_edges_original == E
    assert sc.rows.dtype == torch.int32 and torch.equal(sc.rows.long(), part.score_rows)
    assert sc.views.num_edges == E and torch.equal(sc.views.srt_dst, part.views.srt_dst[part.score_rows])
    assert torch.equal(sc.views.srt_src, part.views.srt_src[part.score_rows])
    assert sc.score_views.srt_src is sc.views.srt_src and sc.score_views.srt_dst is sc.views.srt_dst
    assert torch.equal(sc.score_views.srt_eid, part.srt_geid[part.score_rows])
    assert torch.equal(torch.sort(sc.score_views.srt_eid.long()).values, torch.arange(E))   # every original edge, once
