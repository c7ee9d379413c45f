"""GPU tests of the REVERSED pass of SymGatedGCNModel and of the symmetry-loss step (train.py:159-170) on destination-range partitions,
with the HIP kernels as compute (the host twin is tests/test_dist_symmetry_gloo.py).  The test box has ONE MI355X: world 1 runs over RCCL
with GNNOME_FORCE_COLLECTIVES=1, world 2 is two processes sharing the device over gloo with host staging, as in tests/test_hip_partition.py,
whose bars these are.  Never run on two devices."""
import functools
import gc

import pytest
import torch

import gnnome_amd
from conftest import load_golden
from dist_symmetry_worker import run_ranks
from gnnome_amd import dist as gdist
from gnnome_amd import ops
from gnnome_amd.synth import random_state_dict
from test_train_host import check_grads

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


_run = functools.partial(run_ranks, timeout=240)   # (world, case, tmp_path) -> what each rank saved


def _prob_diff(a, b):
    return (torch.sigmoid(a) - torch.sigmoid(b)).abs().max().item()


def _case(g, world, **kw):
    case = dict(src=g["src"], dst=g["dst"], num_nodes=g["num_nodes"], x=g["x"], x_rev=g["x_rev"], e=g["e"], y=g["y"], pos_weight=g["pos_weight"],
                alpha=g["alpha"], device="cuda")
    if world == 1:   # one rank that still issues every collective, over RCCL on device memory
        case.update(transport="nccl", force_collectives=True)
    case.update(kw)
    return case


def _model(sd, hidden, layers):
    m = gnnome_amd.models.SymGatedGCNModel(2, 2, hidden, 16, layers, 64, "batch", dropout=0.0)
    m.load_state_dict(sd)
    return m.to(dev())


@pytest.mark.parametrize("hidden,world", [(64, 1), (64, 2), (128, 1), (128, 2)])
def test_reversed_eval_logits_on_the_shard(tmp_path, shipped_weights, hidden, world):
    """run_partitioned(..., reverse=True) against the single-rank model(views.reversed(), x_rev, e) on G4's graph: one rank (equal
    numbering, every collective issued) gives the same bits; two ranks number their halo rows differently, so their sums associate
    differently - test_hip_partition.py's bar for two ranks against the single-process forward, 1e-5 on the probabilities."""
    g = load_golden("g4_reverse_h64.pt")
    layers = 8 if hidden == 64 else 2
    sd = shipped_weights if hidden == 64 else random_state_dict(hidden, num_layers=layers, seed=7)
    m = _model(sd, hidden, layers).eval()
    views = gnnome_amd.graph.views_for((g["src"], g["dst"], g["num_nodes"]), dev())
    with torch.no_grad():
        want = m(views.reversed(), g["x_rev"].to(dev()), g["e"].to(dev())).squeeze(1).cpu()
        fwd = m(views, g["x"].to(dev()), g["e"].to(dev())).squeeze(1).cpu()
    outs = _run(world, _case(g, world, hidden=hidden, layers=layers, state_dict=sd), tmp_path)
    for o in outs:
        diff = _prob_diff(o["rev"], want)
        print(f"H = {hidden}, world {world}: reversed eval probability difference {diff:.3e}")
        if world == 1:
            assert o["backend"] == "nccl"
            assert torch.equal(o["rev"][o["srt_geid"].long()], want[o["srt_geid"].long()]) and torch.equal(o["rev"], want)
            assert torch.equal(o["org"], fwd)
        else:
            assert diff < 1e-5
            assert _prob_diff(o["org"], fwd) < 1e-5
        assert torch.equal(o["runner_rev"], o["rev"]) and o["plan_untouched"]
        assert torch.equal(o["rev"], outs[0]["rev"])
    assert _prob_diff(want, fwd) > 1e-3    # (the reversed pass is another function: a forward pass in its place would not pass)
    assert sum(o["n_score"] for o in outs) == g["src"].numel()
    if world > 1:
        assert all(o["n_local"] > o["n_own"] for o in outs)


@pytest.mark.parametrize("world", [1, 2])
def test_symmetry_step_on_the_shard_matches_the_whole_graph_step(tmp_path, world):
    """loss.symmetry_loss over train_forward() and train_forward(reverse=True), then backward() through both passes, against the same step
    on the whole graph (tests/test_hip_training.py::test_symmetry_loss_harness_matches_golden_and_trains): the loss, the 142 gradients, the
    BatchNorm buffers - with the bars of the partitioned BCE step at H = 64 in tests/test_hip_partition.py."""
    from gnnome_amd.loss import symmetry_loss
    g = load_golden("g4_reverse_h64.pt")
    sd = random_state_dict(64, seed=g["seed"])
    m = _model(sd, 64, 8).train()
    views = gnnome_amd.graph.views_for((g["src"], g["dst"], g["num_nodes"]), dev())
    x, xr, e, y, pw = (g[k].to(dev()) for k in ("x", "x_rev", "e", "y", "pos_weight"))
    org, rev = m(views, x, e).squeeze(-1), m(views.reversed(), xr, e).squeeze(-1)
    want_loss = symmetry_loss(org, rev, y, pw, g["alpha"])
    want_loss.backward()
    want_g = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    want_b = {k: b.detach().cpu() for k, b in m.named_buffers()}
    assert len(want_g) == 142
    outs = _run(world, _case(g, world, hidden=64, layers=8, state_dict=sd, train=True), tmp_path)
    for o in outs:
        num = sum(((o["grads"][k] - w).double() ** 2).sum().item() for k, w in want_g.items()) ** 0.5
        den = sum((w.double() ** 2).sum().item() for w in want_g.values()) ** 0.5
        print(f"world {world}: org / rev probability difference {_prob_diff(o['org'], org.detach().cpu()):.3e} / "
              f"{_prob_diff(o['rev'], rev.detach().cpu()):.3e}, loss difference {abs(o['loss'].item() - want_loss.item()):.3e}, "
              f"gradient relative L2 {num / den:.3e}")
        assert _prob_diff(o["org"], org.detach().cpu()) < 1e-4 and _prob_diff(o["rev"], rev.detach().cpu()) < 1e-4
        assert abs(o["loss"].item() - want_loss.item()) < 1e-5
        check_grads(o["grads"], want_g, rtol=1e-3)
        for k, want in want_b.items():
            assert torch.allclose(o["buffers"][k].float(), want.float(), atol=1e-5, rtol=1e-4), k
        for li in range(8):
            assert o["buffers"][f"gnn.convs.{li}.bn_e.num_batches_tracked"].item() == 4
            assert o["buffers"][f"gnn.convs.{li}.bn_h.num_batches_tracked"].item() == 2
        assert o["plan_untouched"]
    for k in outs[0]["grads"]:
        assert all(torch.equal(outs[0]["grads"][k], o["grads"][k]) for o in outs[1:]), k


def _hub_graph():
    """64 nodes, rank 0 owns [0, 32).  Node 5: 74 out-edges (every node once - its self-loop among them - and nodes 0..9 a second time:
    duplicates) - in the reversed pass a long IN-run; node 7: in-edges but no out-edge - its reversed in-run is empty; 300 random edges
    besides, none leaving node 7."""
    gen = torch.Generator().manual_seed(64)
    src = torch.randint(0, 64, (300,), generator=gen)
    dst = torch.randint(0, 64, (300,), generator=gen)
    src[src == 7] = 8
    hub_dst = torch.cat([torch.arange(64), torch.arange(10)])
    src = torch.cat([src, torch.full((74,), 5), torch.tensor([3, 40])])
    dst = torch.cat([dst, hub_dst, torch.tensor([7, 7])])
    perm = torch.randperm(src.numel(), generator=gen)
    return src[perm].int(), dst[perm].int(), 64


@pytest.mark.parametrize("hidden", [64, 128])
def test_reversed_shard_aggregation_on_hub_and_empty_rows_equals_the_whole_graph_kernel(hidden):
    """The node update of the reversed pass on rank 0's shard of a two-way partition (owned nodes first, halo ascending: the whole graph's
    order of every owned node's lists), as dist.run_partitioned launches it - the plan's own views with the flag flipped, A2 <-> A3 -
    against gnnome_node_aggregate_f32 on the whole graph's views.reversed(): the owned rows bit for bit."""
    src, dst, n = _hub_graph()
    n_own, H = 32, hidden
    assert int((src == 5).sum()) >= 70 and int((src == 7).sum()) == 0 and int((dst == 7).sum()) > 0
    assert bool(((src == 5) & (dst == 5)).any()) and int(((src == 5) & (dst == 3)).sum()) >= 2
    gen = torch.Generator().manual_seed(hidden)
    E = src.numel()
    e_id = torch.randn(E, H, generator=gen)                      # e' rows by edge id
    P, h = torch.randn(n, 3 * H, generator=gen), torch.randn(n, H, generator=gen)
    scale, shift = torch.rand(H, generator=gen) + 0.5, torch.randn(H, generator=gen)
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    rv = views.reversed()
    Pd, hd = P.to(dev()), h.to(dev())
    A1, A2, A3 = (Pd[:, i * H:(i + 1) * H] for i in range(3))
    es = e_id.to(dev())[views.srt_eid.long()].contiguous()
    want = ops.node_aggregate(es, A1, A3, A2, rv, hd, 0, scale.to(dev()), shift.to(dev()))        # roles swapped: engine.layer_step
    # rank 0's shard, as PartitionedGraph._build numbers it
    keep = (src < n_own) | (dst < n_own)
    ls, ld = src[keep].long(), dst[keep].long()
    halo = torch.unique(torch.cat([ls, ld])[torch.cat([ls, ld]) >= n_own])
    gid = torch.cat([torch.arange(n_own), halo])
    to_local = lambda t: torch.where(t < n_own, t, n_own + torch.searchsorted(halo, t))  # noqa: E731
    lv = ops.GraphViews(to_local(ls).int().to(dev()), to_local(ld).int().to(dev()), gid.numel())
    assert gid.numel() > n_own and not lv.transposed
    lr = lv.reversed()
    assert lr.transposed and lr.srt_src.data_ptr() == lv.srt_src.data_ptr() and lr.out_pos.data_ptr() == lv.out_pos.data_ptr()
    el = e_id[keep].to(dev())[lv.srt_eid.long()].contiguous()
    Pl, hl = Pd[gid.to(dev())].contiguous(), hd[gid.to(dev())].contiguous()
    B1, B2, B3 = (Pl[:, i * H:(i + 1) * H] for i in range(3))
    got = ops.node_aggregate(el, B1, B3, B2, lr, hl, 0, scale.to(dev()), shift.to(dev()), num_nodes_out=n_own)
    assert torch.equal(got[:n_own], want[:n_own])
    # node 7's reversed in-run (its out_pos run) is empty: that gated sum is 0 / 1e-6 = 0 whatever table it gathers from - an all-zero
    # one leaves row 7 as it was and changes the hub's row
    Pz = Pd.clone()
    Pz[:, H:2 * H] = 0
    other = ops.node_aggregate(es, Pz[:, :H], Pz[:, 2 * H:], Pz[:, H:2 * H], rv, hd, 0, scale.to(dev()), shift.to(dev()))
    assert torch.equal(want[7], other[7]) and not torch.equal(want[5], other[5])


def test_captured_refusal_of_the_reversed_pass_pins_no_device_memory(shipped_weights):
    g = load_golden("g4_reverse_h64.pt")
    m = _model(shipped_weights, 64, 8).eval()
    part = gdist.PartitionedGraph.from_global(g["src"], g["dst"], g["num_nodes"], 0, 1, dev())
    runner = gdist.PartitionedRunner(m, part, g["x"], g["e"], dev(), x_rev_global=g["x_rev"])
    gc.collect()
    gc.disable()
    try:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev())
        with pytest.raises(NotImplementedError, match="CapturedPartitionedForward") as ex:
            gdist.CapturedPartitionedForward(runner, reverse=True)
        with pytest.raises(NotImplementedError, match="CapturedPartitionedForward") as ex2:
            runner.capture(reverse=True)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated(dev()) == before and ex.value is not ex2.value    # with both errors still in hand
    finally:
        gc.enable()
    flipped = gdist.PartitionedGraph.from_global(g["src"], g["dst"], g["num_nodes"], 0, 1, dev())
    flipped.views = flipped.views.reversed()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev())
    with pytest.raises(NotImplementedError, match="forward orientation"):
        gdist.PartitionedRunner(m, flipped, g["x"], g["e"], dev())
    assert torch.cuda.memory_allocated(dev()) == before
