"""GPU tests of GCNModel / SAGEModel on destination-range partitions: the two partition entries of csrc/node_neighbour.hip and
csrc/node_neighbour_bwd.hip on one process, and the ranks of a default partition as processes sharing the one GPU (HIP kernels as
compute, gloo with host staging as transport, as test_hip_partition.py) against the single-rank model on the same GPU.  The CPU twin is
test_dist_baseline_gloo.py; the graphs are those of tests/gated_partition_graphs.py plus baseline_partition_graphs.hub_on_the_boundary
(H = 64, 2 layers, hidden_edge_scores 32 for the model; the kernels at all three widths).

Bars (none of them chosen from what this code gives):
  part entries  the owned rows EQUAL BIT FOR BIT the whole-graph entry's rows [lo, hi), forward and backward: same lists, same order, same
                device code.  A launch with a row list writes exactly its rows; the union of any split equals the unsplit result bit for bit.
  eval logits   edge probabilities within 1e-5 of the single-rank forward and equal bits on every rank (test_hip_partition.py's bars).
  training      test_hip_partition.py::_check_partitioned_step's tolerances for the same quantities: probabilities 1e-4, loss 1e-5, every
                gradient rtol 3e-2 of its largest entry, the whole gradient 3e-3 in relative L2, gradients bit-equal on every rank.
"""
import pytest
import torch
import torch.nn.functional as F

import baseline_partition_graphs as bpg
from dist_baseline_worker import CONFIGS, run_ranks
from gnnome_amd import engine_baselines as eb
from gnnome_amd import ops
from test_train_host import check_grads

pytestmark = pytest.mark.gpu

CASES = [("mixed", 3), ("island", 2), ("star", 2), ("star", 3)]
SENTINEL = -12345.678
_cache = {}
_state = {"failed": False}


def dev():
    return torch.device("cuda", 0)


def _graph(name):
    if name not in _cache:
        _cache[name] = bpg.hub_on_the_boundary() if name == "hub" else bpg.GRAPHS[name]()
    return _cache[name]


def _whole(name, hidden):
    """The whole graph on the device: views, the node tables of both directions' operands, the scales of both `directed` values."""
    key = (name, hidden, "whole")
    if key not in _cache:
        gr = _graph(name)
        n = gr["num_nodes"]
        g = torch.Generator().manual_seed(hidden + n)
        c = dict(views=ops.GraphViews(gr["src"].to(dev()), gr["dst"].to(dev()), n))
        for k in ("h", "add", "y"):
            c[k] = torch.randn(n, hidden, generator=g)
        c["mult"] = (torch.rand(n, hidden, generator=g) >= 0.25).float() / 0.75
        c["scales"] = {directed: bpg.whole_scales(gr, directed) for directed in (True, False)}
        _cache[key] = c
    return _cache[key]


def _scale_args(c, form, both):
    """(source-side scale, destination-side scale) of the forward: GraphConv's, or SAGEConv's mean."""
    din_rsqrt, dout_rsqrt, din_inv = c["scales"][not both]
    return (dout_rsqrt, din_rsqrt) if form == "gcn" else (None, din_inv)


def _forward_whole(name, hidden, both, form):
    key = (name, hidden, both, form, "fwd")
    if key not in _cache:
        c = _whole(name, hidden)
        s, d = _scale_args(c, form, both)
        _cache[key] = ops.node_neighbour_sum(c["h"].to(dev()), c["views"], sscale=None if s is None else s.to(dev()), dscale=d.to(dev()),
                                             both=both).cpu()
    return _cache[key]


def _backward_args(c, form, both, rows=slice(None)):
    """Keyword tables of the backward in one of its three forms, restricted to `rows` where the entry reads owned rows only."""
    din_rsqrt, dout_rsqrt, din_inv = c["scales"][not both]
    pick = lambda t: t[rows].to(dev()).contiguous()  # noqa: E731
    if form == "sage":
        return dict(rscale=din_inv, add=pick(c["add"]), mult=pick(c["mult"]), y=pick(c["y"]))
    return dict(rscale=din_rsqrt, oscale=pick(dout_rsqrt), **({"y": pick(c["y"])} if form == "gcn" else {}))


def _backward_whole(name, hidden, both, form):
    key = (name, hidden, both, form, "bwd")
    if key not in _cache:
        c = _whole(name, hidden)
        kw = _backward_args(c, form, both)
        kw["rscale"] = kw["rscale"].to(dev())
        _cache[key] = ops.node_neighbour_sum_bwd(c["h"].to(dev()), c["views"], both=both, **kw).cpu()
    return _cache[key]


def _shard(name, world, rank):
    """The full shard on the device, as dist.PartitionedGraph builds it: local views, the lists in the whole graph's order."""
    key = (name, world, rank, "shard")
    if key not in _cache:
        sh = bpg.full_shard_of(_graph(name), world, rank)
        views = ops.GraphViews(sh["src"].to(dev()), sh["dst"].to(dev()), int(sh["node_gid"].numel()))
        sh["lists"] = eb.ShardLists(views, sh["node_gid"].to(dev()))
        halo_in = eb._rows_with_halo(views.in_ptr, views.srt_src, sh["n_own"])
        halo_out = eb._rows_with_halo(views.out_ptr, views.out_dst, sh["n_own"])
        sh["halo"] = dict(fwd={False: halo_in, True: halo_in | halo_out}, bwd={False: halo_out, True: halo_in | halo_out})
        _cache[key] = sh
    return _cache[key]


def _forward_part(c, sh, both, form, rows=None, out=None):
    s, d = _scale_args(c, form, both)
    gid = sh["node_gid"]
    return ops.node_neighbour_sum_part(c["h"][gid].to(dev()), sh["lists"], sh["n_own"], sscale=None if s is None else s[gid].to(dev()),
                                       dscale=d[sh["lo"]:sh["hi"]].to(dev()).contiguous(), both=both, rows=rows, out=out)


def _backward_part(c, sh, both, form, rows=None, out=None):
    gid = sh["node_gid"]
    kw = _backward_args(c, form, both, slice(sh["lo"], sh["hi"]))
    kw["rscale"] = kw["rscale"][gid].to(dev())
    return ops.node_neighbour_sum_bwd_part(c["h"][gid].to(dev()), sh["lists"], sh["n_own"], both=both, rows=rows, out=out, **kw)   # g by hand


@pytest.mark.parametrize("form", ["gcn", "sage"])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("hidden", [64, 128, 256])
@pytest.mark.parametrize("name,world", CASES)
def test_forward_part_entry_equals_the_whole_graph_entry_on_the_owned_rows(name, world, hidden, both, form):
    c, want = _whole(name, hidden), _forward_whole(name, hidden, both, form)
    for rank in range(world):
        sh = _shard(name, world, rank)
        got = _forward_part(c, sh, both, form)
        assert got.shape == (sh["n_own"], hidden)
        assert torch.equal(got.cpu(), want[sh["lo"]:sh["hi"]]), f"rank {rank}"


@pytest.mark.parametrize("form", ["gcn", "sage", "layer0"])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("hidden", [64, 128, 256])
@pytest.mark.parametrize("name,world", CASES)
def test_backward_part_entry_equals_the_whole_graph_entry_on_the_owned_rows(name, world, hidden, both, form):
    c, want = _whole(name, hidden), _backward_whole(name, hidden, both, form)
    for rank in range(world):
        sh = _shard(name, world, rank)
        got = _backward_part(c, sh, both, form)
        assert got.shape == (sh["n_own"], hidden)
        assert torch.equal(got.cpu(), want[sh["lo"]:sh["hi"]]), f"rank {rank}"


def _check_row_lists(launch, sh, halo, hidden):
    """Each launch leaves exactly its rows written; the union of each split is the unsplit result bit for bit."""
    n_own = sh["n_own"]
    unsplit = launch(None, None).cpu()
    every = torch.arange(n_own, device=dev())
    splits = [(every[~halo], every[halo]), (every[1::2], every[0::2]), (every, every[:0])]
    for parts in splits:
        union = torch.full((n_own, hidden), SENTINEL, device=dev())
        for rows in parts:
            alone = torch.full((n_own, hidden), SENTINEL, device=dev())
            rows = rows.int().contiguous()
            launch(rows, alone)
            launch(rows, union)
            written = (alone != SENTINEL).any(1).cpu()
            want = torch.zeros(n_own, dtype=torch.bool)
            want[rows.long().cpu()] = True
            assert torch.equal(written, want)
            assert torch.equal(alone.cpu()[want], unsplit[want])
        assert torch.equal(union.cpu(), unsplit)


@pytest.mark.parametrize("form", ["gcn", "sage"])   # (sage: no source-side scale - the other instantiation of the row-list kernel)
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("hidden", [64, 128, 256])
@pytest.mark.parametrize("name,world", CASES)
def test_forward_row_lists_write_their_rows_and_add_up_to_the_unsplit_launch(name, world, hidden, both, form):
    c = _whole(name, hidden)
    for rank in range(world):
        sh = _shard(name, world, rank)
        _check_row_lists(lambda rows, out: _forward_part(c, sh, both, form, rows, out), sh, sh["halo"]["fwd"][both], hidden)
        assert torch.equal(_forward_part(c, sh, both, form).cpu(), _forward_whole(name, hidden, both, form)[sh["lo"]:sh["hi"]])


@pytest.mark.parametrize("form", ["gcn", "sage", "layer0"])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("hidden", [64, 128, 256])
@pytest.mark.parametrize("name,world", CASES)
def test_backward_row_lists_write_their_rows_and_add_up_to_the_unsplit_launch(name, world, hidden, both, form):
    c = _whole(name, hidden)
    for rank in range(world):
        sh = _shard(name, world, rank)
        _check_row_lists(lambda rows, out: _backward_part(c, sh, both, form, rows, out), sh, sh["halo"]["bwd"][both], hidden)


def test_whole_table_and_no_row_list_is_the_whole_graph_entry():
    """num_nodes_out == num_nodes_local, rows == NULL: the whole-graph entry's bits (world 1: the shard IS the graph)."""
    c = _whole("mixed", 128)
    gr = _graph("mixed")
    one = dict(gr, bounds={1: [0, gr["num_nodes"]]})
    sh = bpg.full_shard_of(one, 1, 0)
    views = ops.GraphViews(sh["src"].to(dev()), sh["dst"].to(dev()), gr["num_nodes"])
    sh["lists"] = eb.ShardLists(views, sh["node_gid"].to(dev()))
    for both in (False, True):
        assert torch.equal(_forward_part(c, sh, both, "gcn").cpu(), _forward_whole("mixed", 128, both, "gcn"))
        assert torch.equal(_backward_part(c, sh, both, "sage").cpu(), _backward_whole("mixed", 128, both, "sage"))


@pytest.mark.parametrize("both", [False, True])
def test_a_hub_on_the_range_boundary_takes_the_block_path_in_the_part_entries(both):
    gr = _graph("hub")
    hub = gr["bounds"][2][1]
    assert int((gr["dst"] == hub).sum()) > 4096 and int((gr["src"] == hub).sum()) > 4096 and gr["src"].numel() < 10000
    c = _whole("hub", 64)
    for rank in range(2):
        sh = _shard("hub", 2, rank)
        for form in ("gcn", "sage"):
            assert torch.equal(_forward_part(c, sh, both, form).cpu(), _forward_whole("hub", 64, both, form)[sh["lo"]:sh["hi"]])
            assert torch.equal(_backward_part(c, sh, both, form).cpu(), _backward_whole("hub", 64, both, form)[sh["lo"]:sh["hi"]])
    own = _shard("hub", 2, 1)
    ls = own["lists"]
    for ptr, idx in ((ls.in_ptr, ls.srt_src), (ls.out_ptr, ls.out_dst)):   # the hub is rank 1's row 0; both its lists cross the boundary
        entries = idx[int(ptr[0]):int(ptr[1])]
        assert entries.numel() > 4096 and bool((entries >= own["n_own"]).any()) and bool((entries < own["n_own"]).any())


# ---- the model: ranks as processes sharing the device --------------------------------------------------------------------------------

def _single_rank(name, config):
    key = (name, config, "one")
    if key not in _cache:
        from gnnome_amd import train
        kind, directed, dropout = config
        gr = _graph(name)
        graph = (gr["src"], gr["dst"], gr["num_nodes"])
        x, e = gr["x"].to(dev()), gr["e"].to(dev())
        m = bpg.model(kind, directed, dropout).to(dev()).eval()
        with torch.no_grad():
            logits = m(graph, x, e).squeeze(1).cpu()
        m.train()
        keep = train.dropout_mask
        if dropout > 0:
            train.dropout_mask = bpg.HandedMasks(bpg.known_masks(gr, dropout), 0, gr["num_nodes"])
        try:
            out = eb.train_forward(m, graph, x, e)
            loss = F.binary_cross_entropy_with_logits(out.squeeze(-1), gr["y"].to(dev()), pos_weight=gr["pos_weight"].to(dev()))
            loss.backward()
        finally:
            train.dropout_mask = keep
        _cache[key] = dict(logits=logits, train_logits=out.detach().squeeze(1).cpu(), loss=loss.detach().cpu(),
                           grads={k: p.grad.cpu() for k, p in m.named_parameters()})
    return _cache[key]


@pytest.mark.parametrize("name,world", [("mixed", 3), ("star", 2)])
def test_ranks_sharing_the_gpu_match_the_single_rank_models(name, world, tmp_path):
    """Eval logits and one training step of every rank, for both models and both `directed` values and once with feat_drop masks handed
    to both runs, against the single-rank model on the same GPU.  At most three rank processes under one time limit; after a failed run
    nothing else is started on the device."""
    if _state["failed"]:
        pytest.fail("an earlier partitioned run on the GPU failed: no further rank processes are started")
    gr = _graph(name)
    ones = {config: _single_rank(name, config) for config in CONFIGS}
    _state["failed"] = True
    outs = run_ranks(world, dict(gr, device="cuda"), str(tmp_path), timeout=240)
    _state["failed"] = False
    for config in CONFIGS:
        one = ones[config]
        for o in outs:
            c = o["configs"][config]
            if config[2] == 0.0:
                diff = (torch.sigmoid(c["logits"]) - torch.sigmoid(one["logits"])).abs().max().item()
                print(f"{name} world {world} {config}: eval probability difference {diff:.3e}")
                assert diff < 1e-5, config
                assert torch.equal(c["logits"], outs[0]["configs"][config]["logits"])
                assert torch.equal(c["logits_split"], c["logits"])
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
    from gnnome_amd.models import GATModel
    gr = _graph("island")
    part = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev())
    in_only = gdist.PartitionedGraph.from_global(gr["src"], gr["dst"], gr["num_nodes"], 0, 1, dev(), in_edges_only=True)
    x, e = gr["x"], gr["e"]       # host tensors: a runner that got as far as its inputs would allocate
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev())
    for kind in bpg.KINDS:
        with pytest.raises(ValueError, match="out-lists"):
            gdist.PartitionedRunner(bpg.model(kind).eval(), in_only, x, e, dev())
    with pytest.raises(NotImplementedError, match="GATModel is not served on partitions"):
        gdist.PartitionedRunner(GATModel(2, 2, 64, 16, 2, 32, "batch").eval(), part, x, e, dev())
    assert torch.cuda.memory_allocated(dev()) == before
    with pytest.raises(NotImplementedError, match="CapturedPartitionedForward"):
        gdist.PartitionedRunner(bpg.model("gcn").eval().to(dev()), part, x, e, dev()).capture()
