"""GPU tests of GATModel on destination-range partitions: the four partition entries of csrc/node_attention.hip and
csrc/node_attention_bwd.hip on one process, and the ranks of a default partition as processes sharing the one GPU (HIP kernels as compute,
gloo with host staging as transport, as test_hip_baseline_partition.py) against the single-rank model on the same GPU.  The CPU twin is
test_dist_gat_gloo.py; the graphs are those of tests/gated_partition_graphs.py plus baseline_partition_graphs.hub_on_the_boundary (H = 64,
2 layers, hidden_edge_scores 32 for the model; the kernels at all three widths).

Bars (none of them chosen from what this code gives):
  part entries  the owned rows EQUAL BIT FOR BIT the whole-graph entries' rows [lo, hi): out and stats of the forward; der and the work rows
                of the destination phase; dfeat and del of the source phase once the halo rows of g and work hold the whole graph's rows.
                Same lists, same order, same device code.  The destination phase leaves the work rows >= n_own as they were.
  eval logits   edge probabilities within 1e-5 of the single-rank forward and equal bits on every rank (test_hip_partition.py's bars).
  training      test_hip_partition.py::_check_partitioned_step's tolerances for the same quantities: probabilities 1e-4, loss 1e-5, every
                gradient rtol 3e-2 of its largest entry, the whole gradient 3e-3 in relative L2, gradients bit-equal on every rank.
"""
import pytest
import torch
import torch.nn.functional as F

import baseline_partition_graphs as bpg
import gat_partition_cases as gpc
from dist_gat_worker import run_ranks
from gnnome_amd import _lib, engine_gat, ops
from gnnome_amd import engine_baselines as eb
from test_train_host import check_grads

pytestmark = pytest.mark.gpu

CASES = [("mixed", 3), ("island", 2), ("star", 2), ("star", 3)]
SENTINEL = -12345.678
SLOPE = 0.2
_cache = {}
_state = {"failed": False}


def dev():
    return torch.device("cuda", 0)


def _graph(name):
    if name not in _cache:
        _cache[name] = bpg.hub_on_the_boundary() if name == "hub" else bpg.GRAPHS[name]()
    return _cache[name]


def _p(t):
    return None if t is None else t.data_ptr()


def _whole(name, hidden, both):
    """The whole graph's tables (host) and what the three whole-graph entries make of them (host): out, stats; dfeat, del, der and the
    work table - the backward through the C entry itself, which is the one way to keep `work`.  "mixed" runs with a bias."""
    key = (name, hidden, both, "whole")
    if key not in _cache:
        gr = _graph(name)
        n, W = gr["num_nodes"], 3 * hidden
        gen = torch.Generator().manual_seed(hidden + n)
        c = {k: torch.randn(n, W, generator=gen) for k in ("feat", "g")}
        c["el"], c["er"] = torch.randn(n, 4, generator=gen), torch.randn(n, 4, generator=gen)
        c["bias"] = torch.randn(W, generator=gen) if name == "mixed" else None
        views = ops.GraphViews(gr["src"].to(dev()), gr["dst"].to(dev()), n)
        d = {k: (None if v is None else v.to(dev())) for k, v in c.items()}
        plain = ops.node_attention_sum(d["feat"], views, d["el"], d["er"], bias=d["bias"], negative_slope=SLOPE, both=both)
        out, stats = ops.node_attention_sum_stats(d["feat"], views, d["el"], d["er"], bias=d["bias"], negative_slope=SLOPE, both=both)
        assert torch.equal(plain, out)
        dfeat, del_, der, work = (torch.full((n, cols), SENTINEL, device=dev()) for cols in (W, 4, 4, 16))
        rc = _lib.load().gnnome_node_attention_sum_bwd_f32(
            _p(d["g"]), W, _p(d["feat"]), W, _p(d["el"]), 4, _p(d["er"]), 4, _p(out), W, _p(d["bias"]), _p(stats), 8, hidden, 3, n,
            _p(views.in_ptr), _p(views.srt_src), _p(views.out_ptr), _p(views.out_dst), 1 if both else 0, SLOPE, _p(dfeat), W, _p(del_), 4,
            _p(der), 4, _p(work), None)
        torch.cuda.synchronize()
        assert rc == 0
        c.update(out=out.cpu(), stats=stats.cpu(), dfeat=dfeat.cpu(), del_=del_.cpu(), der=der.cpu(), work=work.cpu())
        _cache[key] = c
    return _cache[key]


def _shard(name, world, rank):
    """The full shard on the device, as dist.PartitionedGraph builds it: local views, the lists in the whole graph's order."""
    key = (name, world, rank, "shard")
    if key not in _cache:
        gr = _graph(name)
        if world == 1:
            gr = dict(gr, bounds={1: [0, gr["num_nodes"]]})
        sh = bpg.full_shard_of(gr, world, rank)
        views = ops.GraphViews(sh["src"].to(dev()), sh["dst"].to(dev()), int(sh["node_gid"].numel()))
        sh["lists"] = eb.ShardLists(views, sh["node_gid"].to(dev()))
        _cache[key] = sh
    return _cache[key]


def _check_shard(c, sh, both):
    """All four part entries on one shard against the whole graph's rows, bit for bit."""
    gid, lo, hi, n_own = sh["node_gid"], sh["lo"], sh["hi"], sh["n_own"]
    n_local = gid.numel()
    up = lambda t: None if t is None else t.to(dev()).contiguous()  # noqa: E731
    feat, el, er, bias = up(c["feat"][gid]), up(c["el"][gid]), up(c["er"][lo:hi]), up(c["bias"])
    kw = dict(bias=bias, negative_slope=SLOPE, both=both)
    # ---- forward, both forms
    out = ops.node_attention_sum_part(feat, sh["lists"], n_own, el, er, **kw)
    out2, stats = ops.node_attention_sum_stats_part(feat, sh["lists"], n_own, el, er, **kw)
    assert out.shape == out2.shape == (n_own, feat.shape[1]) and stats.shape == (n_own, 8)
    assert torch.equal(out.cpu(), c["out"][lo:hi]) and torch.equal(out2.cpu(), c["out"][lo:hi]) and torch.equal(stats.cpu(), c["stats"][lo:hi])
    # ---- destination phase: g's halo rows are not there yet (NaN), work's rows >= n_own hold a sentinel and keep it
    g = up(c["g"][gid])
    g[n_own:] = float("nan")
    work = torch.full((n_local, 16), SENTINEL, device=dev())
    der, _ = ops.node_attention_sum_bwd_dst_part(g, sh["lists"], n_own, feat, el, er, out2, stats, work=work, **kw)
    assert der.shape == (n_own, 4)
    assert torch.equal(der.cpu(), c["der"][lo:hi]) and torch.equal(work[:n_own].cpu(), c["work"][lo:hi])
    assert bool((work[n_own:] == SENTINEL).all())
    # ---- the exchange, by hand: the halo rows of g and work from the whole graph's tables
    g[n_own:], work[n_own:] = up(c["g"][gid[n_own:]]), up(c["work"][gid[n_own:]])
    dfeat, del_ = ops.node_attention_sum_bwd_src_part(g, sh["lists"], n_own, feat[:n_own], el[:n_own], work, negative_slope=SLOPE, both=both)
    assert dfeat.shape == (n_own, feat.shape[1]) and del_.shape == (n_own, 4)
    assert torch.equal(dfeat.cpu(), c["dfeat"][lo:hi]) and torch.equal(del_.cpu(), c["del_"][lo:hi])
    return work


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("hidden", [64, 128, 256])
@pytest.mark.parametrize("name,world", CASES)
def test_part_entries_equal_the_whole_graph_entries_on_the_owned_rows(name, world, hidden, both):
    c = _whole(name, hidden, both)
    for rank in range(world):
        _check_shard(c, _shard(name, world, rank), both)


@pytest.mark.parametrize("both", [False, True])
def test_whole_table_is_the_whole_graph_entries(both):
    """num_nodes_out == num_nodes_local (world 1: the shard IS the graph): the forward is the whole-graph entry, the destination phase
    followed by the source phase gnnome_node_attention_sum_bwd_f32 - work included."""
    c = _whole("mixed", 128, both)
    sh = _shard("mixed", 1, 0)
    assert sh["n_own"] == sh["node_gid"].numel() == _graph("mixed")["num_nodes"]
    work = _check_shard(c, sh, both)
    assert torch.equal(work.cpu(), c["work"])


@pytest.mark.parametrize("both", [False, True])
def test_a_hub_on_the_range_boundary_takes_the_block_path_in_the_part_entries(both):
    gr = _graph("hub")
    hub = gr["bounds"][2][1]
    assert int((gr["dst"] == hub).sum()) > 4096 and int((gr["src"] == hub).sum()) > 4096 and gr["src"].numel() < 10000
    c = _whole("hub", 64, both)
    for rank in range(2):
        _check_shard(c, _shard("hub", 2, rank), both)
    own = _shard("hub", 2, 1)
    ls = own["lists"]
    for ptr, idx in ((ls.in_ptr, ls.srt_src), (ls.out_ptr, ls.out_dst)):   # the hub is rank 1's row 0; both its lists cross the boundary
        entries = idx[int(ptr[0]):int(ptr[1])]
        assert entries.numel() > 4096 and bool((entries >= own["n_own"]).any()) and bool((entries < own["n_own"]).any())


def test_argument_errors_return_einval_and_write_nothing():
    """num_nodes_out > num_nodes_local, heads != 3 and hidden = 96: GNNOME_EINVAL from each of the four entries - surfaced by the binding
    as GnnomeHipError - with every output left as it was."""
    lib = _lib.load()
    n_local, n_own, H = 12, 8, 64
    src = torch.arange(n_local, dtype=torch.int32).roll(1)
    views = ops.GraphViews(src.to(dev()), torch.arange(n_local, dtype=torch.int32, device=dev()), n_local)
    ip, ss, op, od = (_p(t) for t in (views.in_ptr, views.srt_src, views.out_ptr, views.out_dst))
    z = lambda *shape: torch.zeros(*shape, device=dev())  # noqa: E731
    s = lambda *shape: torch.full(shape, SENTINEL, device=dev())  # noqa: E731
    for hidden, heads, n_out, words in ((H, 3, n_local + 1, (b": 13 ", b"rows of 12 local rows")), (H, 2, n_own, (b"heads=2",)),
                                       (96, 3, n_own, (b"hidden=96",))):
        W = 3 * hidden
        feat, g, el, er, A, stats, wk = z(n_local, W), z(n_local, W), z(n_local, 4), z(n_local, 4), z(n_local, W), z(n_local, 8), z(n_local, 16)
        out, st, der, work, dfeat, del_ = s(n_local, W), s(n_local, 8), s(n_local, 4), s(n_local, 16), s(n_local, W), s(n_local, 4)
        calls = {
            "gnnome_node_attention_sum_part_f32": (_p(feat), W, _p(el), 4, _p(er), 4, hidden, heads, n_out, n_local, ip, ss, op, od, SLOPE, None,
                                                   _p(out), W, None),
            "gnnome_node_attention_sum_stats_part_f32": (_p(feat), W, _p(el), 4, _p(er), 4, hidden, heads, n_out, n_local, ip, ss, op, od, SLOPE,
                                                         None, _p(out), W, _p(st), 8, None),
            "gnnome_node_attention_sum_bwd_dst_part_f32": (_p(g), W, _p(feat), W, _p(el), 4, _p(er), 4, _p(A), W, None, _p(stats), 8, hidden, heads,
                                                           n_out, n_local, ip, ss, op, od, 1, SLOPE, _p(der), 4, _p(work), None),
            "gnnome_node_attention_sum_bwd_src_part_f32": (_p(g), W, _p(feat), W, _p(el), 4, _p(wk), hidden, heads, n_out, n_local, op, od, ip, ss,
                                                           1, SLOPE, _p(dfeat), W, _p(del_), 4, None),
        }
        for name, args in calls.items():
            rc = getattr(lib, name)(*args)
            assert rc == -1, (name, hidden, heads, n_out)
            text = lib.gnnome_last_error()
            assert all(w in text for w in words), (name, text)
            with pytest.raises(_lib.GnnomeHipError):
                _lib.check(rc, name)
        torch.cuda.synchronize()
        for t in (out, st, der, work, dfeat, del_):
            assert bool((t == SENTINEL).all())
    # the Python front ends: an unbuilt width is the C entry's refusal, more owned than local rows their own
    with pytest.raises(_lib.GnnomeHipError, match="hidden=96"):
        ops.node_attention_sum_part(z(n_local, 288), views, n_own, z(n_local, 4), z(n_own, 4))
    with pytest.raises(ValueError, match="owned of"):
        ops.node_attention_sum_stats_part(z(n_local, 192), views, n_local + 1, z(n_local, 4), z(n_local + 1, 4))


# ---- the model: ranks as processes sharing the device --------------------------------------------------------------------------------

def _single_rank(name, config):
    key = (name, config, "one")
    if key not in _cache:
        from gnnome_amd import train
        directed, dropout = config
        gr = _graph(name)
        graph = (gr["src"], gr["dst"], gr["num_nodes"])
        x, e = gr["x"].to(dev()), gr["e"].to(dev())
        m = gpc.model(directed, dropout).to(dev()).eval()
        with torch.no_grad():
            logits = m(graph, x, e).squeeze(1).cpu()
        m.train()
        keep = train.dropout_mask
        if dropout > 0:
            train.dropout_mask = gpc.HandedMasks(gpc.known_masks(gr, dropout), 0, gr["num_nodes"])
        try:
            out = engine_gat.train_forward(m, graph, x, e)
            loss = F.binary_cross_entropy_with_logits(out.squeeze(-1), gr["y"].to(dev()), pos_weight=gr["pos_weight"].to(dev()))
            loss.backward()
        finally:
            train.dropout_mask = keep
        _cache[key] = dict(logits=logits, train_logits=out.detach().squeeze(1).cpu(), loss=loss.detach().cpu(),
                           grads={k: p.grad.cpu() for k, p in m.named_parameters()})
    return _cache[key]


@pytest.mark.parametrize("name,world", [("mixed", 3), ("star", 2)])
def test_ranks_sharing_the_gpu_match_the_single_rank_model(name, world, tmp_path):
    """Eval logits and one training step of every rank, for both `directed` values and once with feat_drop masks handed to both runs,
    against the single-rank model on the same GPU.  At most three rank processes under one time limit; after a failed run nothing else
    is started on the device."""
    if _state["failed"]:
        pytest.fail("an earlier partitioned run on the GPU failed: no further rank processes are started")
    gr = _graph(name)
    ones = {config: _single_rank(name, config) for config in gpc.CONFIGS}
    _state["failed"] = True
    outs = run_ranks(world, dict(gr, device="cuda"), str(tmp_path), timeout=240)
    _state["failed"] = False
    for config in gpc.CONFIGS:
        one = ones[config]
        for o in outs:
            c = o["configs"][config]
            if config[1] == 0.0:
                diff = (torch.sigmoid(c["logits"]) - torch.sigmoid(one["logits"])).abs().max().item()
                print(f"{name} world {world} {config}: eval probability difference {diff:.3e}")
                assert diff < 1e-5, config
                assert torch.equal(c["logits"], outs[0]["configs"][config]["logits"])
            diff = (torch.sigmoid(c["train_logits"]) - torch.sigmoid(one["train_logits"])).abs().max().item()
            num = sum(((c["grads"][k] - w).double() ** 2).sum().item() for k, w in one["grads"].items()) ** 0.5
            den = sum((w.double() ** 2).sum().item() for w in one["grads"].values()) ** 0.5
            print(f"{name} world {world} {config}: step probability difference {diff:.3e}, loss difference "
                  f"{abs(c['loss'].item() - one['loss'].item()):.3e}, gradient relative L2 {num / den:.3e}")
            assert diff < 1e-4, config
            assert abs(c["loss"].item() - one["loss"].item()) < 1e-5, config
            check_grads(c["grads"], one["grads"], rtol=3e-2)
            assert num / den < 3e-3, f"{config}: relative L2 error of the full gradient {num / den:.2e}"
        for k in outs[0]["configs"][config]["grads"]:
            assert all(torch.equal(outs[0]["configs"][config]["grads"][k], o["configs"][config]["grads"][k]) for o in outs[1:]), (config, k)


def test_refusals_raise_before_any_device_allocation():
    from gnnome_amd import dist as gdist
    gr = _graph("island")
    new = lambda **kw: gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev(), **kw)  # noqa: E731
    part, in_only, flipped, empty = new(), new(in_edges_only=True), new(), new()
    flipped.views = flipped.views.reversed()
    empty.n_score = 0
    x, e = gr["x"], gr["e"]       # host tensors: a runner that got as far as its inputs would allocate
    gat, gcn = gpc.model().eval(), bpg.model("gcn").eval()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev())
    with pytest.raises(TypeError, match="GATModel"):
        gdist.GATPartitionedRunner(gcn, part, x, e, dev())
    with pytest.raises(ValueError, match="in_edges_only"):
        gdist.GATPartitionedRunner(gat, in_only, x, e, dev())
    with pytest.raises(NotImplementedError, match="forward orientation"):
        gdist.GATPartitionedRunner(gat, flipped, x, e, dev())
    with pytest.raises(NotImplementedError, match="without owned nodes or owned in-edges"):
        gdist.GATPartitionedRunner(gat, empty, x, e, dev())
    with pytest.raises(NotImplementedError, match=r"^GATModel is not served on partitions.*GATPartitionedRunner"):
        gdist.PartitionedRunner(gat, part, x, e, dev())
    assert torch.cuda.memory_allocated(dev()) == before
    with pytest.raises(NotImplementedError, match="CapturedPartitionedForward"):
        gdist.GATPartitionedRunner(gpc.model().eval().to(dev()), part, x, e, dev()).capture()
