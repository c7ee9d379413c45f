"""GPU tests of GatedGCNModel(directed=False) on the doubled plan: the HIP kernels as compute, one rank in this process and two and three
ranks as processes sharing the one GPU (gloo with host staging as transport, as test_hip_gated_partition.py) - at most 3 processes with the
device open, every launch under its own time limit - against the whole-graph directed=False eval and in-edge step of the same model on
the same device.  The graph is tests/gated_doubled_graphs.py's (at world 3 its last rank scores nothing); the CPU twins are
test_dist_gated_doubled_host.py and test_dist_gated_doubled_gloo.py.  Never run on two devices.

Bars - those of the directed=True partition tests of this model on the GPU, unchanged:
  aggregation   tests/test_hip_gated_partition.py:96-98 - the owned rows of gnnome_node_aggregate_in_raw_part_f32 on a rank's rows of the
                DOUBLED list EQUAL BIT FOR BIT to gnnome_node_aggregate_in_raw_f32 on the whole doubled graph: same in-lists, same order.
  eval logits   tests/test_hip_gated_partition.py:166-167 - edge probabilities within 1e-5 of the whole-graph forward, equal bits on every rank.
  training      tests/test_hip_gated_partition.py:168-177 - probabilities 1e-4, loss 1e-5, every gradient rtol 3e-2 of its largest entry, the
                whole gradient 3e-3 in relative L2, buffers atol 1e-5 / rtol 1e-4, gradients bit-equal on every rank.
  the loop      tests/test_dist_trainer_gloo.py:117-126 - the model files of world 1 and world 2 within 10 times the plain-torch loop's own
                fp32-to-fp64 difference in relative L2 of the parameters; the first step's losses within 1e-5 (tests/test_hip_trainer_partition.py:53).
LayerNorm has no cross-rank statistics; the directed=True tests hold the aggregation's rows to bit equality and no logits, so this file
does the same: a rank projects its owned and its halo rows as two products of other shapes than the whole graph's one, and the split-operand
GEMM does not promise the same bits for a row whatever the shape around it.  LayerNorm's logits take the bars above; whether the bits were
equal is printed.
"""
import pytest
import torch
import torch.nn.functional as F

import gated_doubled_graphs as gdg
import gated_graphs as gg
import gated_partition_graphs as gpg
from dist_gated_doubled_worker import one_epoch_at_worlds_one_and_two, plain_torch_epoch, rel_l2, run_ranks
from gnnome_amd import dist as gdist
from gnnome_amd import engine_gated, ops, trainer
from gnnome_amd.models import GatedGCNModel
from test_train_host import check_grads

pytestmark = pytest.mark.gpu

_cache = {}
_state = {"failed": False}


def _graph():
    if "graph" not in _cache:
        _cache["graph"] = gdg.graph()
    return _cache["graph"]


def _model(norm):
    m = GatedGCNModel(2, 2, gdg.HIDDEN, 16, gdg.LAYERS, gdg.SCORE_HIDDEN, norm, dropout=0.0, directed=False)
    m.load_state_dict(gg.random_gated_state_dict(m, seed=8))
    return m


def _step(m, forward, gr, dev):
    out = forward()
    loss = F.binary_cross_entropy_with_logits(out.squeeze(-1), gr["y"].to(dev), pos_weight=gr["pos_weight"].to(dev))
    loss.backward()
    return dict(train_logits=out.detach().squeeze(1).cpu(), loss=loss.detach().cpu(), grads={k: p.grad.cpu() for k, p in m.named_parameters()},
                buffers={k: b.detach().cpu().clone() for k, b in m.named_buffers()})


def _single_rank(norm):
    """The merged whole-graph directed=False path: model(graph, x, e) in eval mode and one in-edge step."""
    if norm not in _cache:
        gr, dev = _graph(), torch.device("cuda", 0)
        graph = (gr["src"], gr["dst"], gr["num_nodes"])
        m = _model(norm).to(dev).eval()
        with torch.no_grad():
            logits = m(graph, gr["x"].to(dev), gr["e"].to(dev)).squeeze(1).cpu()
        m.train()
        m.training_step = "in_edge"
        _cache[norm] = dict(_step(m, lambda: m(graph, gr["x"].to(dev), gr["e"].to(dev)), gr, dev), logits=logits)
    return _cache[norm]


def _check(norm, world, outs, one):
    for o in outs:
        assert o["logits"].shape == one["logits"].shape == (_graph()["src"].numel(),)
        dp, dt = ((torch.sigmoid(o[k]) - torch.sigmoid(one[k])).abs().max().item() for k in ("logits", "train_logits"))
        num = sum(((o["grads"][k] - w).double() ** 2).sum().item() for k, w in one["grads"].items()) ** 0.5
        den = sum((w.double() ** 2).sum().item() for w in one["grads"].values()) ** 0.5
        print(f"{norm} world {world}: eval max |dp| = {dp:.2e} (equal bits: {torch.equal(o['logits'], one['logits'])}), train max |dp| = {dt:.2e}, "
              f"loss {o['loss'].item():.7f} vs {one['loss'].item():.7f}, relative L2 error of the full gradient {num / den:.2e}")
        assert dp < 1e-5
        assert torch.equal(o["logits"], outs[0]["logits"])
        assert dt < 1e-4
        assert abs(o["loss"].item() - one["loss"].item()) < 1e-5
        check_grads(o["grads"], one["grads"], rtol=3e-2)
        assert num / den < 3e-3
        assert set(o["buffers"]) == set(one["buffers"])
        for k, want in one["buffers"].items():
            assert torch.allclose(o["buffers"][k].float(), want.float(), atol=1e-5, rtol=1e-4), k
    for k in outs[0]["grads"]:
        assert all(torch.equal(outs[0]["grads"][k], o["grads"][k]) for o in outs[1:]), k


@pytest.mark.parametrize("world", [2, 3])
def test_the_aggregation_on_a_ranks_rows_of_the_doubled_list_equals_the_whole_doubled_graphs_bit_for_bit(world):
    gr, dev, H = _graph(), torch.device("cuda", 0), gdg.HIDDEN
    src, dst = engine_gated.doubled_edge_list(gr["src"].long(), gr["dst"].long())
    n, E2 = gr["num_nodes"], int(src.numel())
    g = torch.Generator().manual_seed(5)
    e, P = 2.0 * torch.randn(E2, H, generator=g), torch.randn(n, 2 * H, generator=g)
    views = ops.GraphViews(src.int().to(dev), dst.int().to(dev), n)
    whole = [t.cpu() for t in ops.node_aggregate_in_raw(e.to(dev)[views.srt_eid.long()], P.to(dev)[:, :H], P.to(dev)[:, H:], views)]
    doubled = dict(src=src, dst=dst, num_nodes=n, bounds=gr["bounds"])
    for rank in range(world):
        sh = gpg.shard_of(doubled, world, rank)
        lv = ops.GraphViews(sh["src"].to(dev), sh["dst"].to(dev), int(sh["node_gid"].numel()))
        assert int(lv.in_ptr[sh["n_own"]]) == lv.num_edges > 0
        local_gid = sh["edge_gid"][lv.srt_eid.long().cpu()]
        Pl = P[sh["node_gid"]].to(dev)
        got = ops.node_aggregate_in_raw_part(e[local_gid].to(dev), Pl[:, :H], Pl[:, H:], lv, sh["n_own"])
        for t, want, what in zip(got, whole, ("v", "fwd", "rden")):
            assert torch.equal(t.cpu(), want[sh["lo"]:sh["hi"]]), f"{what} of rank {rank}"


@pytest.mark.parametrize("norm", ["batch", "layer"])
def test_one_rank_on_a_doubled_plan_matches_the_whole_graph_directed_false_model(norm):
    """World 1 in this process: no collective, the whole-graph entries of the step on the plan's own views."""
    gr, one, dev = _graph(), _single_rank(norm), torch.device("cuda", 0)
    part = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev, in_edges_only=True, doubled=True)
    assert part.doubled and part.n_score == 2 * part.n_score_original == 2 * int(gr["src"].numel())
    x, e = gr["x"].to(dev), gr["e"].to(dev)
    m = _model(norm).to(dev).eval()
    logits = gdist.PartitionedRunner(m, part, x, e, dev).forward().squeeze(1).cpu()
    m.train()
    m.training_step = "in_edge"
    out = dict(_step(m, gdist.PartitionedRunner(m, part, x, e, dev).train_forward, gr, dev), logits=logits)
    _check(norm, 1, [out], one)


@pytest.mark.parametrize("norm,world", [(norm, world) for norm in ("batch", "layer") for world in (2, 3)])
def test_ranks_sharing_the_gpu_match_the_whole_graph_directed_false_model(norm, world, tmp_path):
    """Eval logits and one in-edge training step of every rank.  At most three rank processes under one time limit; after a failed run
    nothing else is started on the device."""
    if _state["failed"]:
        pytest.fail("an earlier partitioned run on the GPU failed: no further rank processes are started")
    gr, one = _graph(), _single_rank(norm)
    _state["failed"] = True
    outs = run_ranks(world, dict(gr, norm=norm, state_dict=_model(norm).state_dict(), device="cuda"), str(tmp_path), timeout=240)
    _state["failed"] = False
    E = int(gr["src"].numel())
    assert sum(o["e_local"] for o in outs) == 2 * E and sum(o["n_score_original"] for o in outs) == E
    assert all(o["sliced_equal"] and o["default_bounds_equal"] for o in outs)
    if world == 3:
        assert outs[2]["n_score_original"] == 0 and outs[2]["n_score"] > 0
    _check(norm, world, outs, one)


def test_train_partitioned_writes_the_same_model_file_at_worlds_one_and_two(tmp_path):
    """One epoch, one graph, overfit=True, a GatedGCNModel subclass with directed=False and training_step = "in_edge": the loop builds the
    doubled plan, finishes with a finite loss, and the two model files agree to the loop's bar (module docstring)."""
    if _state["failed"]:
        pytest.fail("an earlier partitioned run on the GPU failed: no further rank processes are started")
    gr = _graph()
    _state["failed"] = True
    res = one_epoch_at_worlds_one_and_two(gr, tmp_path, device="cuda")
    _state["failed"] = False
    (one, file1), (two, file2) = res[1], res[2]
    first = one["trace"][0]
    lr = trainer.hyperparameters_with({})["lr"]
    _, end32 = plain_torch_epoch(gr, first["initial_state"], first["pos_weight"], torch.float32, lr)
    _, end64 = plain_torch_epoch(gr, first["initial_state"], first["pos_weight"], torch.float64, lr)
    noise = rel_l2(end32, end64)
    got = rel_l2({k: file2[k] for k in end32}, {k: file1[k] for k in end32})
    l1, l2 = one["trace"][1]["loss"], two["trace"][1]["loss"]
    print(f"model files of world 2 and world 1: relative L2 {got:.3e}; the plain-torch loop's fp32 to fp64 {noise:.3e}, bar {10 * noise:.3e}; "
          f"first-step loss {l2:.7f} vs {l1:.7f}")
    for r in (one, two):
        assert torch.isfinite(torch.tensor(r["records"][0]["train/loss"])) and r["trace"][1]["logits"].numel() == gr["src"].numel()
    assert abs(l2 - l1) < 1e-5
    assert set(file1) == set(file2) and got < 10 * noise
    assert [r["world"] for r in two["records"]] == [2]
