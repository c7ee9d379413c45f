"""GPU tests of GatedGCNModel on destination-range partitions: the two partition entries of csrc/node_aggregate_in_bwd.hip on one process, and
the ranks of an in-edge-only partition as processes sharing the one GPU (HIP kernels as compute, gloo with host staging as transport, as
test_hip_partition.py) against the single-rank model on the same GPU.  The CPU twin is test_dist_gated_gloo.py; the graphs are those of
tests/gated_partition_graphs.py (H = 64, 2 layers, hidden_edge_scores 32 for the model; the kernels at all three widths).

Bars (none of them chosen from what this code gives):
  raw form      owned rows EQUAL BIT FOR BIT to gnnome_node_aggregate_in_raw_f32 on the whole graph: same in-lists, same order, same kernel.
  backward      against the fp64 evaluation of the header's formulas (cpu_ops_gated on double inputs), element by element, u = 2^-24:
                de:   |err| <= 2u (9 (|Tf A2h| + |Uf|) + |de|) - sigmoid within 3 ulp makes w = s(1-s) good to 8u absolute, the inner fma
                      rounds once (u |t|, w <= 1/4), the outer fma once (u |de|); doubled for the fp64 reference's own s.
                dA2h: |err| <= 2u (k + 8 + world) sum |s Tf| with k the longest fma chain of the node's out-list: its length up to 4096
                      items, 128 + ceil(len / 128) above (fixed 128-item blocks), 8 for s and the lane-group tree, one addition per rank
                      for the partials summed on the host in rank order.
  eval logits   edge probabilities within 1e-5 of the single-rank forward and equal bits on every rank (test_hip_partition.py's bars).
  training      test_hip_partition.py::_check_partitioned_step's tolerances for the same quantities: probabilities 1e-4, loss 1e-5, every
                gradient rtol 3e-2 of its largest entry, the whole gradient 3e-3 in relative L2, buffers atol 1e-5 / rtol 1e-4, gradients
                bit-equal on every rank.
"""
import pytest
import torch
import torch.nn.functional as F

import cpu_ops
import cpu_ops_gated
import gated_graphs as gg
import gated_partition_graphs as gpg
from dist_gated_worker import run_ranks
from gnnome_amd import ops
from gnnome_amd.models import GatedGCNModel
from test_train_host import check_grads

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
_cache = {}
_state = {"failed": False}


def _graph(name):
    if name not in _cache:
        _cache[name] = gpg.GRAPHS[name]()
    return _cache[name]


def _kernel_case(name, hidden):
    """Whole-graph operands of both entries (rows by edge id / by node id) and their whole-graph results, made once per (graph, width)."""
    key = (name, hidden, "kernel")
    if key not in _cache:
        gr = _graph(name)
        n, E = gr["num_nodes"], int(gr["src"].numel())
        g = torch.Generator().manual_seed(hidden + n)
        c = dict(e=2.0 * torch.randn(E, hidden, generator=g), P=torch.randn(n, 4 * hidden, generator=g), Tf=torch.randn(n, hidden, generator=g),
                 Uf=torch.randn(n, hidden, generator=g), de=torch.randn(E, hidden, generator=g))
        dev = torch.device("cuda", 0)
        views = ops.GraphViews(gr["src"].to(dev), gr["dst"].to(dev), n)
        Pd = c["P"].to(dev)
        c["srt_eid"] = views.srt_eid.long().cpu()
        c["raw"] = [t.cpu() for t in ops.node_aggregate_in_raw(c["e"].to(dev)[views.srt_eid.long()], Pd[:, :hidden], Pd[:, hidden:2 * hidden], views)]
        # the fp64 evaluation of the backward's formulas on the whole graph (sorted order)
        cv = cpu_ops.CpuViews(gr["src"], gr["dst"], n)
        assert torch.equal(cv.srt_eid.long(), c["srt_eid"])
        order = c["srt_eid"]
        e64, A2_64, Tf64, Uf64 = c["e"][order].double(), c["P"][:, hidden:2 * hidden].double(), c["Tf"].double(), c["Uf"].double()
        de64 = c["de"][order].double().clone()
        c["dA2_64"] = cpu_ops_gated.node_aggregate_in_bwd(e64, Tf64, Uf64, A2_64, cv, de64)
        c["de_64"] = de64
        s, d = cv.srt_src.long(), cv.srt_dst.long()
        sig = torch.sigmoid(e64)
        c["de_bound"] = 2 * U * (9 * ((Tf64[d] * A2_64[s]).abs() + Uf64[d].abs()) + de64.abs())
        out_len = torch.bincount(s, minlength=n)
        chain = torch.where(out_len > 4096, 128 + (out_len + 127) // 128, out_len).double()
        c["dA2_mag"], c["dA2_chain"] = torch.zeros(n, hidden, dtype=torch.float64).index_add(0, s, (sig * Tf64[d]).abs()), chain
        c["pos_of_id"] = torch.empty(E, dtype=torch.int64)
        c["pos_of_id"][order] = torch.arange(E)
        _cache[key] = c
    return _cache[key]


def _shard_on_device(gr, c, hidden, world, rank):
    dev = torch.device("cuda", 0)
    sh = gpg.shard_of(gr, world, rank)
    views = ops.GraphViews(sh["src"].to(dev), sh["dst"].to(dev), int(sh["node_gid"].numel()))
    local_gid = sh["edge_gid"][views.srt_eid.long().cpu()]          # global edge id of every local sorted position
    assert int(views.in_ptr[sh["n_own"]]) == views.num_edges
    P = c["P"][sh["node_gid"]].to(dev)
    return sh, views, local_gid, P


@pytest.mark.parametrize("hidden", [64, 128, 256])
@pytest.mark.parametrize("name,world", [("mixed", 3), ("island", 2), ("star", 2), ("star", 3)])
def test_raw_partition_form_equals_the_whole_graph_entry_on_the_owned_rows(name, world, hidden):
    gr, c = _graph(name), _kernel_case(name, hidden)
    for rank in range(world):
        sh, views, local_gid, P = _shard_on_device(gr, c, hidden, world, rank)
        got = ops.node_aggregate_in_raw_part(c["e"][local_gid].to(P.device), P[:, :hidden], P[:, hidden:2 * hidden], views, sh["n_own"])
        for t, want, what in zip(got, c["raw"], ("v", "fwd", "rden")):
            assert t.shape == (sh["n_own"], hidden)
            assert torch.equal(t.cpu(), want[sh["lo"]:sh["hi"]]), f"{what} of rank {rank}"


@pytest.mark.parametrize("hidden", [64, 128, 256])
@pytest.mark.parametrize("name,world", [("mixed", 3), ("island", 2), ("star", 2), ("star", 3)])
def test_backward_partition_form_against_the_fp64_formulas(name, world, hidden):
    gr, c = _graph(name), _kernel_case(name, hidden)
    n = gr["num_nodes"]
    total = torch.zeros(n, hidden)
    partials = []
    for rank in range(world):
        sh, views, local_gid, P = _shard_on_device(gr, c, hidden, world, rank)
        dev = P.device
        de = c["de"][local_gid].to(dev)
        dA2 = ops.node_aggregate_in_bwd_part(c["e"][local_gid].to(dev), c["Tf"][sh["lo"]:sh["hi"]].to(dev).contiguous(),
                                             c["Uf"][sh["lo"]:sh["hi"]].to(dev).contiguous(), P[:, hidden:2 * hidden], views, de, sh["n_own"])
        assert dA2.shape == (int(sh["node_gid"].numel()), hidden)
        pos = c["pos_of_id"][local_gid]
        err = (de.cpu().double() - c["de_64"][pos]).abs()
        assert bool((err <= c["de_bound"][pos]).all()), f"de of rank {rank}: worst ratio {(err / c['de_bound'][pos]).max().item():.2f}"
        total[sh["lo"]:sh["hi"]] = dA2[:sh["n_own"]].cpu()                # the owner's own partial first ...
        partials.append((sh["node_gid"][sh["n_own"]:], dA2[sh["n_own"]:].cpu()))
    for halo_gid, rows in partials:                                        # ... then the received ones in ascending rank order (fp32, on the host)
        total[halo_gid] += rows
    bound = 2 * U * (c["dA2_chain"][:, None] + 8 + world) * c["dA2_mag"]
    err = (total.double() - c["dA2_64"]).abs()
    assert bool((err <= bound).all()), f"dA2h: worst ratio {(err / bound.clamp(min=1e-300)).max().item():.2f}"
    assert bool((total[torch.bincount(gr["src"].long(), minlength=n) == 0] == 0).all())   # no out-edge: a zero row


# ---- the model: ranks as processes sharing the device --------------------------------------------------------------------------------

def _model():
    m = GatedGCNModel(2, 2, gpg.HIDDEN, 16, gpg.LAYERS, gpg.SCORE_HIDDEN, "batch", dropout=0.0)
    m.load_state_dict(gg.random_gated_state_dict(m, seed=8))
    return m


def _single_rank(name):
    key = (name, "one")
    if key not in _cache:
        gr, dev = _graph(name), torch.device("cuda", 0)
        graph = (gr["src"], gr["dst"], gr["num_nodes"])
        m = _model().to(dev).eval()
        with torch.no_grad():
            logits = m(graph, gr["x"].to(dev), gr["e"].to(dev)).squeeze(1).cpu()
        m.train()
        m.training_step = "in_edge"
        out = m(graph, gr["x"].to(dev), gr["e"].to(dev))
        loss = F.binary_cross_entropy_with_logits(out.squeeze(-1), gr["y"].to(dev), pos_weight=gr["pos_weight"].to(dev))
        loss.backward()
        _cache[key] = dict(logits=logits, train_logits=out.detach().squeeze(1).cpu(), loss=loss.detach().cpu(),
                           grads={k: p.grad.cpu() for k, p in m.named_parameters()}, buffers={k: b.detach().cpu().clone() for k, b in m.named_buffers()})
    return _cache[key]


@pytest.mark.parametrize("name,world", [("mixed", 3), ("island", 2), ("star", 2), ("star", 3)])
def test_ranks_sharing_the_gpu_match_the_single_rank_model(name, world, tmp_path):
    """Eval logits and one in-edge training step of every rank against the single-rank GatedGCNModel on the same GPU.  At most three rank
    processes, each with its own time limit; after a failed run nothing else is started on the device."""
    if _state["failed"]:
        pytest.fail("an earlier partitioned run on the GPU failed: no further rank processes are started")
    gr, one = _graph(name), _single_rank(name)
    _state["failed"] = True
    outs = run_ranks(world, dict(gr, state_dict=_model().state_dict(), device="cuda"), str(tmp_path), timeout=240)
    _state["failed"] = False
    assert sum(o["e_local"] for o in outs) == int(gr["src"].numel()) and all(o["sliced_equal"] for o in outs)
    for o in outs:
        assert (torch.sigmoid(o["logits"]) - torch.sigmoid(one["logits"])).abs().max().item() < 1e-5
        assert torch.equal(o["logits"], outs[0]["logits"])
        assert (torch.sigmoid(o["train_logits"]) - torch.sigmoid(one["train_logits"])).abs().max().item() < 1e-4
        assert abs(o["loss"].item() - one["loss"].item()) < 1e-5
        check_grads(o["grads"], one["grads"], rtol=3e-2)
        num = sum(((o["grads"][k] - w).double() ** 2).sum().item() for k, w in one["grads"].items()) ** 0.5
        den = sum((w.double() ** 2).sum().item() for w in one["grads"].values()) ** 0.5
        assert num / den < 3e-3, f"relative L2 error of the full gradient {num / den:.2e}"
        for k, want in one["buffers"].items():
            assert torch.allclose(o["buffers"][k].float(), want.float(), atol=1e-5, rtol=1e-4), k
    for k in outs[0]["grads"]:
        assert all(torch.equal(outs[0]["grads"][k], o["grads"][k]) for o in outs[1:]), k

