"""GatedGCNModel(directed=False) on the doubled plan, on the CPU: ranks over gloo with the checker backend (tests/cpu_ops_gated.py) as compute -
eval logits and one in-edge training step at worlds 2 and 3, BatchNorm and LayerNorm - against the same backend's WHOLE-GRAPH directed=False
run (engine_gated.run_stack / _InEdgeStep over the doubled views).  The graph is tests/gated_doubled_graphs.py's; at world 3 its last rank
scores nothing.  The plan itself is test_dist_gated_doubled_host.py's; the GPU twin is test_dist_gated_doubled_gpu.py.

Bars - those of the directed=True partition tests of this model, unchanged (the partitioned run differs from the single-rank one in the same
way: how the batch statistics and the weight-gradient sums are associated across ranks):
  eval logits   tests/test_dist_gated_gloo.py:113-114 - edge probabilities within 1e-5 of the single-rank forward, equal bits on every rank.
  training      tests/test_dist_gated_gloo.py:122-129 - probabilities 1e-4, loss 1e-5 absolute, every parameter gradient rtol 2e-3 of its
                largest entry (check_grads), BatchNorm buffers atol 1e-5 / rtol 1e-4, gradients bit-equal on every rank.
LayerNorm has no cross-rank statistics, but the directed=True tests hold no LayerNorm run - and no logits at all - to bit equality with one
rank, so neither does this file: a rank projects its owned and its halo rows as two products of other shapes than the whole graph's one,
and the backend's GEMM does not promise the same bits for a row whatever the shape around it.  LayerNorm takes the same bars.
"""
import pytest
import torch
import torch.nn.functional as F

import cpu_ops
import cpu_ops_gated
import gated_doubled_graphs as gdg
import gated_graphs as gg
from dist_gated_doubled_worker import run_ranks
from gnnome_amd import engine_gated
from gnnome_amd.models import GatedGCNModel
from test_train_host import check_grads

BACKEND = cpu_ops_gated.BACKEND
CASES = [(norm, world) for norm in ("batch", "layer") for world in (2, 3)]
_cache = {}


def _graph():
    if "graph" not in _cache:
        _cache["graph"] = gdg.graph()
    return _cache["graph"]


def _model(norm):
    m = GatedGCNModel(2, 2, gdg.HIDDEN, 16, gdg.LAYERS, gdg.SCORE_HIDDEN, norm, dropout=0.0, directed=False)
    m.load_state_dict(gg.random_gated_state_dict(m, seed=8))
    return m


class _CpuDoubled:
    """engine_gated.Doubled on the checker backend's views."""

    def __init__(self, views, src, dst):
        self.views = cpu_ops.CpuViews(*engine_gated.doubled_edge_list(src, dst), views.num_nodes)
        self.enc_gather, self.score_gather = engine_gated.doubled_row_maps(self.views.srt_eid, views.srt_eid, views.num_edges)


def _single_rank(norm):
    """The whole-graph directed=False run on the checker backend: eval logits, and the in-edge step's logits, loss, gradients, buffers."""
    if norm not in _cache:
        gr = _graph()
        src, dst = gr["src"].long(), gr["dst"].long()
        views = cpu_ops.CpuViews(src, dst, gr["num_nodes"])
        dbl = _CpuDoubled(views, src, dst)
        views._derived = {"doubled": dbl}      # (what engine_gated.doubled_for keeps with a graph's views)
        m = _model(norm).eval()
        with torch.no_grad():
            logits = engine_gated.run_stack(BACKEND, engine_gated.Prepared(m, torch.device("cpu")), views, gr["x"], gr["e"], directed=False)
        m.train()
        names, params = zip(*m.named_parameters())
        sg = engine_gated._StepGraph(views, False, doubled=lambda v: dbl, ops=BACKEND)
        out = engine_gated._InEdgeStep.apply(m, sg, gr["x"], gr["e"], list(names), *params)
        loss = F.binary_cross_entropy_with_logits(out.squeeze(-1), gr["y"], pos_weight=gr["pos_weight"])
        loss.backward()
        _cache[norm] = dict(logits=logits, train_logits=out.detach().squeeze(1), loss=loss.detach(),
                            grads={k: p.grad.clone() for k, p in m.named_parameters()}, buffers={k: b.clone() for k, b in m.named_buffers()})
    return _cache[norm]


@pytest.fixture
def ranks(request, tmp_path_factory):
    """What every rank of a (norm, world) pair computed - one spawn per pair, shared by the tests below."""
    norm, world = request.param
    if (norm, world) not in _cache:
        case = dict(_graph(), norm=norm, state_dict=_model(norm).state_dict())
        _cache[(norm, world)] = run_ranks(world, case, str(tmp_path_factory.mktemp(f"{norm}{world}")), timeout=120)
    return norm, world, _cache[(norm, world)]


def test_the_single_rank_run_is_itself_right():
    """The reference the partitioned runs are held to, against torch autograd over the plain-torch restatement (gated_graphs.gated_model),
    with the bars tests/test_dist_gated_gloo.py::test_the_single_rank_step_is_itself_right applies."""
    gr = _graph()
    for norm in ("batch", "layer"):
        one = _single_rank(norm)
        leaves = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in _model(norm).state_dict().items()}
        want = gg.gated_model(leaves, gr["src"].long(), gr["dst"].long(), gr["num_nodes"], gr["x"], gr["e"], gdg.LAYERS, directed=False, training=True)
        F.binary_cross_entropy_with_logits(want.squeeze(-1), gr["y"], pos_weight=gr["pos_weight"]).backward()
        assert one["logits"].shape == (gr["src"].numel(),)
        assert (torch.sigmoid(one["train_logits"]) - torch.sigmoid(want.detach().squeeze(1))).abs().max().item() < 1e-5
        check_grads(one["grads"], {k: leaves[k].grad for k in one["grads"]}, rtol=1e-3)


def test_train_partitioned_builds_the_doubled_plan_and_writes_the_same_model_at_worlds_one_and_two(tmp_path):
    """One epoch, one graph, overfit=True, a GatedGCNModel subclass with directed=False and training_step = "in_edge".  "The same model
    file" with the bar of this loop's directed=True test, tests/test_dist_trainer_gloo.py:117-126: relative L2 of the parameters within 10
    times the plain-torch loop's own fp32-to-fp64 difference; the first step's loss within 1e-5 of that loop's (:119)."""
    from dist_gated_doubled_worker import one_epoch_at_worlds_one_and_two, plain_torch_epoch, rel_l2
    from gnnome_amd import trainer
    gr = _graph()
    res = one_epoch_at_worlds_one_and_two(gr, tmp_path)
    (one, file1), (two, file2) = res[1], res[2]
    first = one["trace"][0]
    lr = trainer.hyperparameters_with({})["lr"]
    loss32, end32 = plain_torch_epoch(gr, first["initial_state"], first["pos_weight"], torch.float32, lr)
    _, end64 = plain_torch_epoch(gr, first["initial_state"], first["pos_weight"], torch.float64, lr)
    noise = rel_l2(end32, end64)
    got = rel_l2({k: file2[k] for k in end32}, {k: file1[k] for k in end32})
    to_plain = rel_l2({k: file2[k] for k in end32}, end32)
    print(f"model files of world 2 and world 1: relative L2 {got:.3e}; world 2 to the plain-torch loop {to_plain:.3e}; that loop's fp32 to "
          f"fp64 {noise:.3e}, bar {10 * noise:.3e}")
    for r in (one, two):
        step = r["trace"][1]
        assert step["n_score"] > 0 and torch.isfinite(torch.tensor(r["records"][0]["train/loss"]))
        assert abs(step["loss"] - loss32) < 1e-5
        assert step["logits"].numel() == gr["src"].numel()          # logits over the ORIGINAL edges
    assert set(file1) == set(file2) and got < 10 * noise and to_plain < 10 * noise
    assert [r["world"] for r in two["records"]] == [2]


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_the_ranks_hold_the_doubled_plan(ranks):
    norm, world, outs = ranks
    E = int(_graph()["src"].numel())
    assert sum(o["e_local"] for o in outs) == 2 * E and sum(o["n_score_original"] for o in outs) == E
    assert all(o["sliced_equal"] and o["default_bounds_equal"] for o in outs)
    if world == 3:
        assert outs[2]["n_score_original"] == 0 and outs[2]["n_score"] > 0      # a rank that scores nothing took part in everything below


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_eval_logits_equal_the_whole_graph_directed_false_run(ranks):
    norm, world, outs = ranks
    want = _single_rank(norm)["logits"]
    for o in outs:
        assert o["logits"].shape == want.shape
        diff = (torch.sigmoid(o["logits"]) - torch.sigmoid(want)).abs().max().item()
        print(f"{norm} world {world}: eval max |dp| = {diff:.2e}, equal bits: {torch.equal(o['logits'], want)}")
        assert diff < 1e-5
        assert torch.equal(o["logits"], outs[0]["logits"])              # every rank holds the full result, the same bits


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_in_edge_training_step_matches_the_whole_graph_directed_false_step(ranks):
    norm, world, outs = ranks
    one = _single_rank(norm)
    for o in outs:
        diff = (torch.sigmoid(o["train_logits"]) - torch.sigmoid(one["train_logits"])).abs().max().item()
        print(f"{norm} world {world}: train max |dp| = {diff:.2e}, loss {o['loss'].item():.7f} vs {one['loss'].item():.7f}")
        assert o["train_logits"].shape == one["train_logits"].shape and diff < 1e-4
        assert abs(o["loss"].item() - one["loss"].item()) < 1e-5
        check_grads(o["grads"], one["grads"], rtol=2e-3)
        assert set(o["buffers"]) == set(one["buffers"])
        for k, want in one["buffers"].items():         # running_mean / running_var after ONE momentum update over the 2E rows; the counters
            assert torch.allclose(o["buffers"][k].float(), want.float(), atol=1e-5, rtol=1e-4), k
    if norm == "batch":          # one momentum update of bn_e per layer and step, as on the whole graph
        k = "gnn.convs.0.bn_e.num_batches_tracked"
        assert outs[0]["buffers"][k].item() == one["buffers"][k].item() == _model(norm).state_dict()[k].item() + 1
    for k in outs[0]["grads"]:   # identical on every rank: optimizers stay in step without a broadcast
        assert all(torch.equal(outs[0]["grads"][k], o["grads"][k]) for o in outs[1:]), k
