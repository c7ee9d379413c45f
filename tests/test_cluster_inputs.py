"""gnnome_cluster_inputs_f32 (csrc/cluster_inputs.hip) through features.cluster_inputs: every cluster's [z(in) | z(out)] in both
orientations and the e / y gathers, against the torch expression of features.partition_degree_features (train.py:125-135) and the
gathers of train.py:148-186, evaluated in float32 on the CPU."""
import types

import numpy as np
import pytest
import torch

from gnnome_amd import _lib, features, ops
from gnnome_amd.partition import cluster_partition, pack_clusters
from gnnome_amd.synth import make_graph

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32).long()


def assert_ulp(got, want, ulps=2):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN positions differ"
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.equal(got[torch.isinf(got)], want[torch.isinf(want)]), "inf differs"
    fin = torch.isfinite(want)
    g, w = got[fin], want[fin]
    same_sign = (torch.sign(g) == torch.sign(w)) | (g == w)
    assert bool(same_sign.all())
    d = (_bits(g.abs()) - _bits(w.abs())).abs()
    assert int(d.max()) <= ulps if d.numel() else True, f"{int(d.max())} ulp"


def torch_reference(subs, in_deg, out_deg, e, y, outer_nid=None, outer_eid=None):
    """features.partition_degree_features + the two gathers, cluster by cluster, on the CPU in float32."""
    in_deg, out_deg, e, y = in_deg.cpu(), out_deg.cpu(), e.cpu(), y.cpu()
    xs, xrs, es, ys = [], [], [], []
    for s in subs:
        nid, eid = s.nid.cpu(), s.eid.cpu()
        if outer_nid is not None:
            nid = outer_nid.cpu()[nid]
        if outer_eid is not None:
            eid = outer_eid.cpu()[eid]
        if nid.numel():
            xs.append(features.partition_degree_features(in_deg, out_deg, nid, reverse=False))
            xrs.append(features.partition_degree_features(in_deg, out_deg, nid, reverse=True))
        es.append(e[eid])
        ys.append(y[eid])
    empty = torch.empty(0, 2)
    return (torch.cat(xs) if xs else empty, torch.cat(xrs) if xrs else empty, torch.cat(es), torch.cat(ys))


def packed(res):
    vals = list(res.values()) if isinstance(res, dict) else res
    return tuple(torch.cat([getattr(v, k) for v in vals]) for k in ("x", "x_rev", "e", "y"))


def check(subs, in_deg, out_deg, e, y, outer_nid=None, outer_eid=None):
    res = features.cluster_inputs(subs, in_deg, out_deg, e, y, outer_nid=outer_nid, outer_eid=outer_eid)
    got = packed(res)
    want = torch_reference(subs.values() if isinstance(subs, dict) else subs, in_deg, out_deg, e, y, outer_nid, outer_eid)
    assert_ulp(got[0], want[0])
    assert_ulp(got[1], want[1])
    assert torch.equal(_bits(got[2].cpu()), _bits(want[2])) and torch.equal(_bits(got[3].cpu()), _bits(want[3]))
    for v, s in zip(res.values() if isinstance(res, dict) else res, subs.values() if isinstance(subs, dict) else subs):
        assert v.x.is_contiguous() and v.x.shape == (s.nid.numel(), 2) and v.e.shape == (s.eid.numel(), 2)
    return got


@pytest.fixture(scope="module")
def graph():
    g = make_graph(20_000, 200_000, seed=4)
    views = ops.GraphViews(g["src"].to(dev()), g["dst"].to(dev()), g["num_nodes"])
    in_deg, out_deg = features.stored_degrees(views)
    return g, views, in_deg, out_deg, g["e"].to(dev()), g["y"].to(dev())


def test_clusters_of_a_masked_graph_with_the_outer_map(graph):
    g, views, in_deg, out_deg, e, y = graph
    torch.manual_seed(3)
    masked = features.mask_graph_strandwise(views, 0.85)
    parts = cluster_partition(masked, masked.num_nodes() // 1000 + 1, extra_cached_hops=1)
    assert len(parts) > 5
    check(parts, in_deg, out_deg, e, y, outer_nid=masked.nid, outer_eid=masked.eid)


def test_clusters_of_the_full_graph_without_an_outer_map(graph):
    g, views, in_deg, out_deg, e, y = graph
    parts = cluster_partition(views, 30, extra_cached_hops=1)
    check(parts, in_deg, out_deg, e, y)


def test_cluster_sizes_across_tile_borders_and_non_finite_statistics():
    """Sizes around the kernel's 256-position tiles, a one-node cluster (std NaN), a cluster whose degrees are all equal (std 0),
    a cluster with no edges and an empty cluster; ids in random order."""
    rng = np.random.default_rng(7)
    n, E = 6000, 9000
    in_deg = torch.from_numpy(rng.integers(0, 20, n).astype(np.float32))
    out_deg = torch.from_numpy(rng.integers(0, 20, n).astype(np.float32))
    in_deg[100:140] = 5.0
    out_deg[100:140] = 5.0
    e = torch.from_numpy(rng.standard_normal((E, 2)).astype(np.float32))
    y = torch.from_numpy((rng.random(E) < 0.4).astype(np.float32))
    sizes = [1, 255, 256, 257, 40, 0, 3, 1000, 511, 2, 1, 600]
    perm = torch.from_numpy(rng.permutation(n))
    subs, off = [], 0
    for i, s in enumerate(sizes):
        nid = torch.arange(100, 140) if s == 40 else perm[off:off + s]
        off += s
        ne = 0 if i in (0, 5, 9) else int(rng.integers(1, 500))
        subs.append(types.SimpleNamespace(nid=nid.long().to(dev()), eid=torch.from_numpy(rng.integers(0, E, ne)).long().to(dev())))
    got = check(subs, in_deg.to(dev()), out_deg.to(dev()), e.to(dev()), y.to(dev()))
    assert bool(torch.isnan(got[0][0]).all())                         # the one-node cluster
    assert bool(torch.isnan(got[0][1 + 255 + 256 + 257:][:40]).all())  # 0 / 0: equal degrees


def test_one_cluster_of_two_million_nodes():
    """k = 1, the full-graph case: one cluster spans thousands of tiles."""
    rng = np.random.default_rng(11)
    n, E = 2_000_000, 3_000_000
    in_deg = torch.from_numpy(rng.integers(0, 40, n).astype(np.float32)).to(dev())
    out_deg = torch.from_numpy(rng.integers(0, 40, n).astype(np.float32)).to(dev())
    e = torch.from_numpy(rng.standard_normal((E, 2)).astype(np.float32)).to(dev())
    y = torch.from_numpy((rng.random(E) < 0.3).astype(np.float32)).to(dev())
    sub = types.SimpleNamespace(nid=torch.arange(n, device=dev()), eid=torch.arange(E, device=dev()))
    res = features.cluster_inputs([sub], in_deg, out_deg, e, y)[0]
    assert torch.equal(_bits(res.e.cpu()), _bits(e.cpu())) and torch.equal(_bits(res.y.cpu()), _bits(y.cpu()))
    # torch's float32 sum of 2M degrees (~4e7) is itself rounded, so its mean is off by a few of its ulp; against the same torch
    # expression with the statistics taken in float64 (then rounded to float32) the kernel is within 2 ulp, and it stays within
    # that rounding of the float32 result
    for col, d in enumerate((in_deg.cpu(), out_deg.cpu())):
        d64 = d.double()
        m, s = d64.mean().float(), d64.std().float()
        assert_ulp(res.x[:, col], (d - m) / s)
        assert_ulp(res.x_rev[:, 1 - col], (d - m) / s)
        want32 = (d - d.mean()) / d.std()
        slack = (abs(d.mean() - m) + abs(d.std() - s) * (d - m).abs().max() / s) / s
        assert (res.x[:, col].cpu() - want32).abs().max() <= slack + 4 * torch.finfo(torch.float32).eps * want32.abs().max()


def test_bit_identical_across_runs(graph):
    g, views, in_deg, out_deg, e, y = graph
    parts = cluster_partition(views, 17, extra_cached_hops=1)
    a = packed(features.cluster_inputs(parts, in_deg, out_deg, e, y))
    b = packed(features.cluster_inputs(parts, in_deg, out_deg, e, y))
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v))


def _raw_call(node_ptr, nid, edge_ptr, eid, in_deg, out_deg, e, y, outer_nid=None, outer_eid=None):
    return ops.cluster_inputs(node_ptr, nid, edge_ptr, eid, in_deg, out_deg, e, y, outer_nid, outer_eid)


@pytest.mark.parametrize("case,cluster", [("node_ptr", 1), ("edge_ptr", 2), ("nid", 2), ("outer_nid", 1), ("eid", 0), ("outer_eid", 2)])
def test_bad_input_raises_naming_the_cluster(case, cluster):
    d = dev()
    n, E = 50, 80
    in_deg, out_deg = torch.ones(n, device=d), torch.arange(n, device=d, dtype=torch.float32)
    e, y = torch.zeros(E, 2, device=d), torch.zeros(E, device=d)
    node_ptr = torch.tensor([0, 4, 9, 15], device=d)
    edge_ptr = torch.tensor([0, 10, 20, 30], device=d)
    nid = torch.arange(15, device=d)
    eid = torch.arange(30, device=d)
    outer_nid = torch.arange(n, device=d)
    outer_eid = torch.arange(E, device=d)
    if case == "node_ptr":
        node_ptr[2] = 3                 # cluster 1 would end before it starts
    elif case == "edge_ptr":
        edge_ptr[3] = 31                # the last cluster runs past eid
    elif case == "nid":
        nid[11] = n
    elif case == "outer_nid":
        outer_nid[6] = -1               # reached through nid[6], cluster 1
    elif case == "eid":
        eid[3] = E
    elif case == "outer_eid":
        outer_eid[25] = E + 5
    with pytest.raises(_lib.GnnomeHipError, match=f"cluster {cluster}:"):
        _raw_call(node_ptr, nid, edge_ptr, eid, in_deg, out_deg, e, y, outer_nid, outer_eid)


def test_nothing_is_written_when_a_check_fails():
    import ctypes
    d = dev()
    n = 40
    in_deg = out_deg = torch.arange(n, device=d, dtype=torch.float32)
    e, y = torch.zeros(10, 2, device=d), torch.zeros(10, device=d)
    node_ptr, nid = torch.tensor([0, 20, 40], device=d), torch.arange(40, device=d)
    edge_ptr, eid = torch.tensor([0, 5, 10], device=d), torch.arange(10, device=d)
    eid[9] = 10
    x = torch.full((40, 2), 7.0, device=d)
    xr, es, ys = torch.full_like(x, 7.0), torch.full((10, 2), 7.0, device=d), torch.full((10,), 7.0, device=d)
    need = ctypes.c_size_t(0)
    lib = _lib.load()
    assert lib.gnnome_cluster_inputs_workspace_bytes(2, 40, ctypes.byref(need)) == 0
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=d)
    p = ops._ptr
    rc = lib.gnnome_cluster_inputs_f32(p(node_ptr), p(nid), 2, 40, p(edge_ptr), p(eid), 10, None, 0, None, 0, p(in_deg), p(out_deg), n,
                                       p(e), p(y), 10, p(x), p(xr), p(es), p(ys), p(ws), ws.numel(), ops._stream(d))
    assert rc != 0 and b"cluster 1" in lib.gnnome_last_error()
    torch.cuda.synchronize()
    assert bool((x == 7).all() and (xr == 7).all() and (es == 7).all() and (ys == 7).all())


def test_pack_clusters_follows_dict_order(graph):
    g, views, *_ = graph
    parts = cluster_partition(views, 9, extra_cached_hops=1)
    node_ptr, nid, edge_ptr, eid = pack_clusters(parts)
    subs = list(parts.values())
    assert node_ptr.tolist() == np.cumsum([0] + [s.nid.numel() for s in subs]).tolist()
    assert torch.equal(nid, torch.cat([s.nid for s in subs])) and torch.equal(eid, torch.cat([s.eid for s in subs]))
    assert edge_ptr.tolist()[-1] == eid.numel()
