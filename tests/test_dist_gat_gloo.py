"""GATModel on destination-range partitions, on the CPU: engine_gat's partition sequences - eval mode and the training step - on CPU ranks
over gloo with the checker backend (tests/cpu_ops_gat.py) as compute, against the SINGLE-RANK sequences of engine_gat on the same backend.
World 2 and 3, uneven bounds, the graphs of tests/gated_partition_graphs.py.  The GPU twin is test_hip_gat_partition.py.

Bars (the project's existing ones for partitioned runs - test_hip_partition.py::_check_partitioned_step - none chosen from what this code
gives):
  eval logits   edge probabilities within 1e-5 of the single-rank forward, EQUAL BITS on every rank.
  training      probabilities 1e-4, loss 1e-5, every gradient rtol 3e-2 of its largest entry, the whole gradient 3e-3 in relative L2,
                gradients bit-equal on every rank.
  exchanges     counted through a wrapper around dist.HaloExchange: the forward starts layers + 1 halo exchanges with feat_drop (layers
                without: layer 0's halo rows come from x), the backward exactly two forward-direction exchanges per layer - 3H wide,
                then 16 wide - and ONE transpose, the scorer's.
The checker fills fresh tables with NaN and its source phase reads g and work at halo rows, so an exchange left out shows as NaN."""
import pytest
import torch
import torch.nn.functional as F

import baseline_partition_graphs as bpg
import cpu_ops_gat
import gat_partition_cases as gpc
from dist_gat_worker import run_ranks
from gnnome_amd import dist as gdist
from gnnome_amd import engine_baselines as eb
from gnnome_amd import engine_gat
from test_train_host import check_grads

BACKEND = cpu_ops_gat.BACKEND
CASES = [(name, world) for name in bpg.GRAPHS for world in (2, 3)]
CPU = torch.device("cpu")
_cache = {}


def _graph(name):
    if name not in _cache:
        _cache[name] = bpg.GRAPHS[name]()
    return _cache[name]


def _single_rank(name, config):
    """engine_gat's single-rank sequences on the checker backend: eval logits, and the step's logits, loss and gradients."""
    key = (name, config)
    if key not in _cache:
        directed, dropout = config
        gr = _graph(name)
        views = cpu_ops_gat.Views(gr["src"], gr["dst"], gr["num_nodes"])
        m = gpc.model(directed, dropout).eval()
        with torch.no_grad():
            logits = engine_gat.run_stack(BACKEND, engine_gat.Prepared(m, CPU), views, gr["x"], gr["e"], directed)
        m.train()
        masks = gpc.known_masks(gr, dropout) if dropout > 0 else [None] * gpc.LAYERS
        out, kept = engine_gat._step_forward(BACKEND, m, views, gr["x"], gr["e"], masks)
        leaf = out.clone().requires_grad_(True)
        loss = F.binary_cross_entropy_with_logits(leaf, gr["y"], pos_weight=gr["pos_weight"])
        loss.backward()
        grads = engine_gat._step_backward(BACKEND, m, views, gr["x"], gr["e"], kept, leaf.grad)
        _cache[key] = dict(logits=logits, train_logits=out, loss=loss.detach(), grads={k: grads[k] for k, _ in m.named_parameters()})
    return _cache[key]


@pytest.fixture
def ranks(request, tmp_path_factory):
    """What every rank of a (graph, world) pair computed - one spawn per pair, shared by the tests below."""
    name, world = request.param
    if (name, world) not in _cache:
        _cache[(name, world)] = run_ranks(world, dict(_graph(name)), str(tmp_path_factory.mktemp(f"gat{name}{world}")), timeout=180)
    return name, world, _cache[(name, world)]


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_eval_logits_equal_the_single_rank_model(ranks):
    name, world, outs = ranks
    for config in gpc.CONFIGS:
        if config[1] > 0:
            continue
        want = _single_rank(name, config)["logits"]
        for o in outs:
            c = o["configs"][config]
            assert c["logits"].shape == want.shape
            assert (torch.sigmoid(c["logits"]) - torch.sigmoid(want)).abs().max().item() < 1e-5, config
            assert torch.equal(c["logits"], outs[0]["configs"][config]["logits"])       # every rank holds the full result, the same bits


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_training_step_matches_the_single_rank_step(ranks):
    name, world, outs = ranks
    for config in gpc.CONFIGS:
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


@pytest.mark.parametrize("ranks", CASES, indirect=True)
def test_the_exchange_pattern(ranks):
    name, world, outs = ranks
    H, L = gpc.HIDDEN, gpc.LAYERS
    for (directed, dropout), o in ((config, o) for config in gpc.CONFIGS for o in outs):
        c = o["configs"][(directed, dropout)]
        if dropout == 0.0:
            assert c["eval_exchanges"] == ([H] * L, 0)                           # layers 1 .. L-1 and the scorer's: layer 0's rows come from x
        assert c["forward_exchanges"] == ([H] * (L + 1 if dropout > 0 else L), 0)
        assert c["backward_exchanges"] == ([3 * H, 16] * L, 1)                   # dA's halo rows, then the work rows; one transpose, the scorer's


def test_the_single_rank_step_is_itself_right():
    """The reference the partitioned runs are held to, against torch autograd over the plain-torch restatement (gat_training_cases)."""
    import gat_training_cases as gtc
    gr = _graph("mixed")
    for config in gpc.CONFIGS:
        directed, dropout = config
        one = _single_rank("mixed", config)
        masks = gpc.known_masks(gr, dropout) if dropout > 0 else None
        leaves = {k: v.clone().requires_grad_(True) for k, v in gpc.model(directed, dropout).state_dict().items()}
        want = gtc.gat_model_train(leaves, gr["src"], gr["dst"], gr["num_nodes"], gr["x"], gr["e"], gpc.LAYERS, directed, masks)
        F.binary_cross_entropy_with_logits(want.squeeze(-1), gr["y"], pos_weight=gr["pos_weight"]).backward()
        assert (torch.sigmoid(one["train_logits"]) - torch.sigmoid(want.detach().squeeze(1))).abs().max().item() < 1e-5
        check_grads(one["grads"], {k: leaves[k].grad for k in one["grads"]}, rtol=1e-3)


def test_refused_cases_raise_up_front():
    gr = _graph("island")
    full = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, CPU, ops=BACKEND)
    in_only = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, CPU, ops=BACKEND, in_edges_only=True)
    run = lambda m, part: gdist.GATPartitionedRunner(m, part, gr["x"], gr["e"], CPU, ops=BACKEND)  # noqa: E731
    with pytest.raises(TypeError, match="GATModel"):
        run(bpg.model("gcn").eval(), full)
    with pytest.raises(ValueError, match="in_edges_only"):
        run(gpc.model().eval(), in_only)
    flipped = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, CPU, ops=BACKEND)
    flipped.views = flipped.views.reversed()
    with pytest.raises(NotImplementedError, match="forward orientation"):
        run(gpc.model().eval(), flipped)
    for field in ("n_own", "n_score"):
        empty = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, CPU, ops=BACKEND)
        setattr(empty, field, 0)
        with pytest.raises(NotImplementedError, match="without owned nodes or owned in-edges"):
            run(gpc.model().eval(), empty)
    with pytest.raises(NotImplementedError, match="CapturedPartitionedForward"):
        run(gpc.model().eval(), full).capture()
    with pytest.raises(NotImplementedError, match=r"^GATModel is not served on partitions.*GATPartitionedRunner"):
        gdist.PartitionedRunner(gpc.model().eval(), full, gr["x"], gr["e"], CPU, ops=BACKEND)
    with pytest.raises(TypeError, match="GATModel"):
        engine_gat.train_forward_on(bpg.model("sage").train(), gdist.PartitionShard(full, BACKEND), gr["x"], gr["e"])
    with pytest.raises(RuntimeError, match="train mode"):
        run(gpc.model().train(), full).forward()


def test_one_rank_equals_the_plain_sequences_bit_for_bit():
    """World 1: no collective, no halo - the checker backend's sums are then the single-rank ones term for term."""
    gr = _graph("island")
    for config in gpc.CONFIGS:
        directed, dropout = config
        if dropout > 0:
            continue
        one = _single_rank("island", config)
        part = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, CPU, ops=BACKEND)
        logits = gdist.GATPartitionedRunner(gpc.model(directed).eval(), part, gr["x"], gr["e"], CPU, ops=BACKEND).forward().squeeze(1)
        assert torch.equal(logits, one["logits"]), config
        m = gpc.model(directed).train()
        out = gdist.GATPartitionedRunner(m, part, gr["x"], gr["e"], CPU, ops=BACKEND).train_forward()
        F.binary_cross_entropy_with_logits(out.squeeze(-1), gr["y"], pos_weight=gr["pos_weight"]).backward()
        assert torch.equal(out.detach().squeeze(1), one["train_logits"]), config
        check_grads({k: p.grad for k, p in m.named_parameters()}, one["grads"], rtol=1e-5)


def test_the_checker_states_the_attention_entries():
    """The checker backend against the fp64 statements of gat_graphs / gat_training_cases (whole graph), and its part forms on a shard
    against its own whole-graph rows - with the halo rows of g and work filled by hand between the two phases."""
    import gat_graphs as gg
    import gat_training_cases as gtc
    gr = _graph("mixed")
    n, H = gr["num_nodes"], 64
    W = 3 * H
    gen = torch.Generator().manual_seed(3)
    feat, G = torch.randn(n, W, generator=gen), torch.randn(n, W, generator=gen)
    el, er = torch.randn(n, 4, generator=gen), torch.randn(n, 4, generator=gen)
    bias = torch.randn(W, generator=gen)
    views = cpu_ops_gat.Views(gr["src"], gr["dst"], n)
    for both in (False, True):
        A, stats = cpu_ops_gat.node_attention_sum_stats(feat, views, el, er, bias=bias, both=both)
        want, _ = gg.attention_sum_f64(feat, el, er, gr["src"].long(), gr["dst"].long(), n, bias=bias, both=both)
        assert (A.double() - want).abs().max().item() < 1e-4
        dfeat, dl, dr = cpu_ops_gat.node_attention_sum_bwd(G, views, feat, el, er, A, stats, bias=bias, both=both)
        (wf, wl, wr), _ = gtc.attention_sum_bwd_f64(G, feat, el, er, gr["src"].long(), gr["dst"].long(), n, both=both, bias=bias)
        for got, w in ((dfeat, wf), (dl[:, :3], wl), (dr[:, :3], wr)):
            assert (got.double() - w).abs().max().item() < 1e-3 * max(1.0, w.abs().max().item())
        _, work_all = cpu_ops_gat.node_attention_sum_bwd_dst_part(G, views, n, feat, el, er, A, stats, bias=bias, both=both)
        for world in (2, 3):
            for rank in range(world):
                sh = bpg.full_shard_of(gr, world, rank)
                gid, lo, hi, n_own = sh["node_gid"], sh["lo"], sh["hi"], sh["n_own"]
                lists = eb.ShardLists(cpu_ops_gat.Views(sh["src"], sh["dst"], gid.numel()), gid)
                a, st = cpu_ops_gat.node_attention_sum_stats_part(feat[gid], lists, n_own, el[gid], er[lo:hi], bias=bias, both=both)
                assert torch.allclose(a, A[lo:hi], rtol=1e-5, atol=1e-6) and torch.allclose(st, stats[lo:hi], rtol=1e-5, atol=1e-6)
                g_local = G[gid].clone()
                g_local[n_own:] = float("nan")
                work = torch.full((gid.numel(), 16), float("nan"))
                der, work = cpu_ops_gat.node_attention_sum_bwd_dst_part(g_local, lists, n_own, feat[gid], el[gid], er[lo:hi], A[lo:hi], stats[lo:hi],
                                                                        bias=bias, both=both, work=work)
                assert torch.allclose(der, dr[lo:hi], rtol=1e-4, atol=1e-5) and bool(torch.isnan(work[n_own:]).all())
                g_local[n_own:], work[n_own:] = G[gid[n_own:]], work_all[gid[n_own:]]
                df, dl_p = cpu_ops_gat.node_attention_sum_bwd_src_part(g_local, lists, n_own, feat[lo:hi], el[lo:hi], work, both=both)
                assert torch.allclose(df, dfeat[lo:hi], rtol=1e-4, atol=1e-5) and torch.allclose(dl_p, dl[lo:hi], rtol=1e-4, atol=1e-5)


def test_header_ctypes_table_and_exports_agree_on_the_part_entries():
    import ctypes
    import re
    import subprocess

    import header_binding
    from gnnome_amd import _lib
    names = ("gnnome_node_attention_sum_part_f32", "gnnome_node_attention_sum_stats_part_f32", "gnnome_node_attention_sum_bwd_dst_part_f32",
             "gnnome_node_attention_sum_bwd_src_part_f32")
    header = open(_lib.HEADER_PATH).read()
    parsed = header_binding.parse_header(_lib.HEADER_PATH)
    kind = lambda t: "ptr" if t in (ctypes.c_void_p,) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)) else t  # noqa: E731
    lib = header_binding.bind(_lib.LIB_PATH, _lib.HEADER_PATH)
    exported = set(re.findall(r" T (gnnome_\w+)", subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                                                                  check=True).stdout))
    for name in names:
        assert [kind(t) for t in parsed[name][1]] == [kind(t) for t in _lib.SIGNATURES[name]], name
        assert hasattr(lib, name) and name in exported
    for cite in ("models/full_graph.py:78-97", "layers/processor.py:49-70"):
        assert cite in header[header.index("the attention sum on one rank's shard of a destination-range partition"):], cite
    # argument validation runs before anything touches the device
    one, two, three = ctypes.c_void_p(16), ctypes.c_void_p(32), ctypes.c_void_p(48)
    fwd, st = lib.gnnome_node_attention_sum_part_f32, lib.gnnome_node_attention_sum_stats_part_f32
    dst, src = lib.gnnome_node_attention_sum_bwd_dst_part_f32, lib.gnnome_node_attention_sum_bwd_src_part_f32
    for hidden, heads, n_out, n_local, words in ((64, 3, 5, 4, b"5 destination rows of 4 local rows"), (64, 2, 4, 5, b"heads=2"),
                                                 (96, 3, 4, 5, b"hidden=96")):
        W = 3 * hidden
        assert fwd(one, W, one, 4, one, 4, hidden, heads, n_out, n_local, one, one, None, None, 0.2, None, two, W, None) == -1
        assert words in lib.gnnome_last_error()
        assert st(one, W, one, 4, one, 4, hidden, heads, n_out, n_local, one, one, None, None, 0.2, None, two, W, three, 8, None) == -1
        assert words in lib.gnnome_last_error()
        assert dst(one, W, one, W, one, 4, one, 4, one, W, None, one, 8, hidden, heads, n_out, n_local, one, one, one, one, 0, 0.2, two, 4, three,
                   None) == -1
        assert words in lib.gnnome_last_error()
        assert src(one, W, one, W, one, 4, one, hidden, heads, n_out, n_local, one, one, one, one, 0, 0.2, two, W, three, 4, None) == -1
        assert words.replace(b"destination", b"source") in lib.gnnome_last_error()
    assert fwd(None, 192, one, 4, one, 4, 64, 3, 4, 5, one, one, None, None, 0.2, None, two, 192, None) == -1
    assert b"null pointer" in lib.gnnome_last_error()
    assert dst(one, 192, one, 192, one, 4, one, 4, one, 192, None, None, 8, 64, 3, 4, 5, one, one, one, one, 0, 0.2, two, 4, three, None) == -1
    assert b"null pointer" in lib.gnnome_last_error()                                                     # (no stats)
    assert src(one, 192, one, 192, one, 4, one, 64, 3, 4, 5, one, one, one, one, 0, 0.2, one, 192, three, 4, None) == -1
    assert b"alias" in lib.gnnome_last_error()                                                            # (dfeat over g)
    assert src(one, 192, one, 192, one, 4, two, 64, 3, 4, 5, one, one, one, one, 0, 0.2, two, 192, three, 4, None) == -1
    assert b"alias" in lib.gnnome_last_error()                                                            # (dfeat over work, which this phase reads)
    for call in (lambda: fwd(None, 192, None, 4, None, 4, 64, 3, 0, 5, None, None, None, None, 0.2, None, None, 192, None),
                 lambda: dst(None, 192, None, 192, None, 4, None, 4, None, 192, None, None, 8, 64, 3, 0, 5, None, None, None, None, 0, 0.2, None, 4,
                             None, None),
                 lambda: src(None, 192, None, 192, None, 4, None, 64, 3, 0, 5, None, None, None, None, 0, 0.2, None, 192, None, 4, None)):
        assert call() == 0                                                                                # no owned row: a no-op
