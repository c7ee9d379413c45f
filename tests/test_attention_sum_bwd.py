"""gnnome_node_attention_sum_stats_f32 and gnnome_node_attention_sum_bwd_f32 (csrc/node_attention.hip, node_attention_bwd.hip) against
the fp64 statement of tests/gat_training_cases.py with its DERIVED per-element bound (attention_sum_bwd_f64's docstring - nothing in it is
measured), plus the exact properties the kernel's header promises.  The bound is asserted without a bias and with one (the bias has its
own term in it)."""
import gc

import pytest
import torch

import baseline_graphs as bg
import gat_graphs as gg
import gat_training_cases as cases
from gnnome_amd import ops

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256)
CASES = [(h, b) for h in WIDTHS for b in (False, True)]
case = pytest.mark.parametrize("hidden,both", CASES)
SLOPE = 0.2


def dev():
    return torch.device("cuda", 0)


def _lengths_graph(hidden):
    """baseline_graphs.mixed_graph (in- and out-degrees 0, 1, 2, 63, 64, 65, 129, parallel edges, self-loops among others and alone) plus,
    for d in G U - 1, G U, G U + 1 (G = 256 / hidden rows at once, U = 4 in flight), one new node with d in-edges and one with d
    out-edges; a triple edge, a graph-own loop, and isolated nodes that also make N no multiple of 4."""
    src, dst, n = bg.mixed_graph(hidden)
    rng = torch.Generator().manual_seed(hidden)
    gu = (256 // hidden) * 4
    s, d = [src.long()], [dst.long()]
    for k in (gu - 1, gu, gu + 1):
        pool = torch.randint(0, n, (k,), generator=rng)
        s += [pool, torch.full((k,), n + 1)]          # node n: k in-edges; node n + 1: k out-edges
        d += [torch.full((k,), n), pool]
        n += 2
    s += [torch.tensor([n, n, n, n + 1])]             # a triple edge n -> n + 1 and the loop n + 1 -> n + 1
    d += [torch.tensor([n + 1, n + 1, n + 1, n + 1])]
    n += 3                                            # ... and node n + 2 without any edge
    while n % 4 != 3:
        n += 1
    return torch.cat(s).int(), torch.cat(d).int(), n


def _hubs_graph():
    """Hubs of 4096 (one level, the threshold itself) and 4097 + 130 (two levels, a ragged last block) IN-edges, and the transposes of
    both on further copies of the nodes: the same two lengths as OUT-lists."""
    s, d, n = [], [], 0
    for length in (4096, 4097 + 130):
        hs, hd, hn = bg.hub_edges(length, 60)
        s += [hs.long() + n, hd.long() + n + hn]
        d += [hd.long() + n, hs.long() + n + hn]
        n += 2 * hn
    src, dst = torch.cat(s), torch.cat(d)
    din, dout = torch.bincount(dst, minlength=n), torch.bincount(src, minlength=n)
    for length in (4096, 4097 + 130):
        assert (din == length).any() and (dout == length).any()
    return src.int(), dst.int(), n + 1                # (one isolated node; N = 245)


def _inputs(n, hidden, seed, scale=2.0):
    """feat, G [n,3H]; el / er [n,4] with scores of scale `scale`, NaN in the pad column (loaded, never used); bias [3H]."""
    g = torch.Generator().manual_seed(seed)
    feat, G = torch.randn(n, 3 * hidden, generator=g), torch.randn(n, 3 * hidden, generator=g)
    el, er = (scale / 2 ** 0.5) * torch.randn(n, 4, generator=g), (scale / 2 ** 0.5) * torch.randn(n, 4, generator=g)
    el[:, 3] = er[:, 3] = float("nan")
    return feat, el, er, G, 0.1 * torch.randn(3 * hidden, generator=g)


def _forward(views, feat, el, er, both, bias=None):
    return ops.node_attention_sum_stats(feat, views, el, er, bias=bias, negative_slope=SLOPE, both=both)


def _backward(views, G, feat, el, er, A, stats, both, bias=None, dP=None):
    return ops.node_attention_sum_bwd(G, views, feat, el, er, A, stats, bias=bias, negative_slope=SLOPE, both=both, dP=dP)


def _check(src, dst, n, hidden, both, seed, with_bias, what, views=None, graph=None):
    """Forward with statistics, backward, both against fp64.  `graph`: the edge list the views stand for (reversed views: swapped)."""
    feat, el, er, G, bias = _inputs(n, hidden, seed)
    bias = bias if with_bias else None
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n) if views is None else views
    gsrc, gdst = (src, dst) if graph is None else graph
    on = lambda t: None if t is None else t.to(dev())  # noqa: E731
    fd, eld, erd, Gd, bd = on(feat), on(el), on(er), on(G), on(bias)
    A, stats = _forward(views, fd, eld, erd, both, bd)
    # 1. the statistics entry
    assert torch.equal(A, ops.node_attention_sum(fd, views, eld, erd, bias=bd, negative_slope=SLOPE, both=both))
    gs, gd = bg.neighbour_lists(gsrc, gdst, n, both)
    x = el[:, :3][gs] + er[:, :3][gd]                                               # fp32, one rounding
    s32 = torch.where(x > 0, x, SLOPE * x)
    assert torch.equal(stats[:, :3].cpu(), gg._segment_max(s32, gd, n))
    den = torch.zeros(n, 3, dtype=torch.float64).index_add_(0, gd, torch.exp(s32.double() - stats[:, :3].cpu().double()[gd]))
    count = torch.bincount(gd, minlength=n).double()[:, None]
    assert ((stats[:, 4:7].cpu().double() * den - 1.0).abs() <= (count + 3.0) * bg.EPS32).all()
    assert not stats[:, 3].any() and not stats[:, 7].any()
    # 2. the backward against the statement
    got = _backward(views, Gd, fd, eld, erd, A, stats, both, bd)
    want, bound = cases.attention_sum_bwd_f64(G, feat, el, er, gsrc, gdst, n, SLOPE, both, bias)
    worst = 0.0
    for g_, w_, b_, name in zip(got, want, bound, ("dfeat", "del", "der")):
        g64 = g_.cpu().double()
        if name != "dfeat":
            assert g_.shape == (n, 4) and not g_[:, 3].any(), f"{name}: the pad column is written 0"
            g64 = g64[:, :3]
        assert torch.isfinite(g64).all()
        frac = ((g64 - w_).abs() / b_.clamp(min=1e-300)).max().item()
        worst = max(worst, frac)
        print(f"{what} H={hidden} both={both} bias={with_bias} {name}: max err / bound = {frac:.4f}")
        assert frac <= 1.0, f"{what} H={hidden} both={both} {name}: max err / bound = {frac:.4f}"
    return views, (fd, eld, erd, Gd, bd, A, stats), got, worst


@case
def test_list_lengths_multi_edges_loops_and_isolated_nodes(hidden, both):
    src, dst, n = _lengths_graph(hidden)
    assert n % 4
    views, (fd, eld, erd, Gd, _, A, stats), got, _ = _check(src, dst, n, hidden, both, 1, False, "lengths")
    _check(src, dst, n, hidden, both, 2, True, "lengths", views=views)
    # 3. exact: an isolated node's row, two calls, a scaling by two
    isolated = n - 1
    assert not (src == isolated).any() and not (dst == isolated).any()
    assert torch.equal(got[0][isolated], Gd[isolated])
    again = _backward(views, Gd, fd, eld, erd, A, stats, both)
    twice = _backward(views, 2.0 * Gd, fd, eld, erd, A, stats, both)
    for a, b, c in zip(got, again, twice):
        assert torch.equal(a, b)
        assert torch.equal(c, 2.0 * a)


@case
def test_hubs_of_4096_and_4227_items_on_each_side(hidden, both):
    src, dst, n = _hubs_graph()
    views, (fd, eld, erd, Gd, _, A, stats), got, _ = _check(src, dst, n, hidden, both, 3, False, "hubs")
    for a, b in zip(got, _backward(views, Gd, fd, eld, erd, A, stats, both)):
        assert torch.equal(a, b)


@case
def test_reversed_views_are_the_swapped_edge_list(hidden, both):
    src, dst, n = _lengths_graph(hidden)
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n).reversed()
    _check(src, dst, n, hidden, both, 4, False, "reversed", views=views, graph=(dst, src))


@case
def test_column_blocks_of_projection_tables(hidden, both):
    """feat | el | er as blocks of P [N, 3H + 64], the results as blocks of dP laid out alike: the dense call's bits, the other score columns
    exactly zero after the call."""
    src, dst, n = _lengths_graph(hidden)
    feat, el, er, G, bias = (t.to(dev()) for t in _inputs(n, hidden, 5))
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    W = 3 * hidden
    A, stats = _forward(views, feat, el, er, both, bias)
    dense = _backward(views, G, feat, el, er, A, stats, both, bias)
    P = torch.full((n, W + 64), -7.0, device=dev())
    P[:, :W], P[:, W:W + 4], P[:, W + 4:W + 8] = feat, el, er
    A2, stats2 = _forward(views, P[:, :W], P[:, W:W + 4], P[:, W + 4:W + 8], both, bias)
    assert torch.equal(A2, A) and torch.equal(stats2, stats)
    dP = torch.full((n, W + 64), float("nan"), device=dev())
    ret = _backward(views, G, P[:, :W], P[:, W:W + 4], P[:, W + 4:W + 8], A, stats, both, bias, dP=dP)
    assert ret[0].data_ptr() == dP.data_ptr() and ret[1].data_ptr() == dP[:, W:].data_ptr()
    assert torch.equal(dP[:, :W], dense[0]) and torch.equal(dP[:, W:W + 4], dense[1]) and torch.equal(dP[:, W + 4:W + 8], dense[2])
    assert not dP[:, W + 3].any() and not dP[:, W + 7:].any()


def _refused(run, match, device):
    """`run` raises with `match`, and the kept error holds no device memory (tests/test_declines_pin_no_device_memory.py)."""
    gc.collect()
    gc.disable()
    try:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(device)
        with pytest.raises(Exception, match=match) as ex:
            run()
        torch.cuda.synchronize()
        assert ex.value is not None and torch.cuda.memory_allocated(device) == before
    finally:
        gc.enable()


def test_refusals_and_a_graph_without_edges():
    hidden = 64
    src, dst, n = _lengths_graph(hidden)
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    z = lambda *shape: torch.zeros(*shape, device=dev())  # noqa: E731
    W = 3 * hidden
    G, feat, A, el, er, stats = z(n, W), z(n, W), z(n, W), z(n, 4), z(n, 4), z(n, 8)
    wide, odd, dP = z(n, W + 4), [z(n, 3 * 96) for _ in range(3)], z(n, W + 64)
    run = lambda g, f, a, **kw: ops.node_attention_sum_bwd(g, views, f, el, er, a, stats, **kw)  # noqa: E731
    # heads = 2: the front ends are built for three heads, so the refusal is the C entry's own (nothing is launched or allocated)
    from gnnome_amd import _lib
    lib, p = _lib.load(), (lambda t: t.data_ptr())
    dl, dr, work = z(n, 4), z(n, 4), z(n, 16)
    rc = lib.gnnome_node_attention_sum_bwd_f32(p(G), W, p(feat), W, p(el), 4, p(er), 4, p(A), W, None, p(stats), 8, hidden, 2, n, p(views.in_ptr),
                                               p(views.srt_src), p(views.out_ptr), p(views.out_dst), 0, 0.2, p(dP), W + 64, p(dl), 4, p(dr), 4,
                                               p(work), None)
    assert rc != 0 and b"heads=2" in lib.gnnome_last_error()
    _refused(lambda: run(*odd), "64,128,256", dev())
    _refused(lambda: run(wide[:, 1:W + 1], feat, A), "16-byte aligned", dev())          # rows that start 4 bytes into a 16-byte line
    _refused(lambda: run(dP[:, :W], feat, A, dP=dP), "alias", dev())                     # dfeat would be written over g
    with pytest.raises(ValueError, match="rows"):
        ops.node_attention_sum_bwd(z(n + 1, W), views, feat, el, er, A, stats)
    with pytest.raises(Exception, match="stats"):
        ops.node_attention_sum_stats(feat, views, el, er, stats=z(n, 4))
    # no edges: every node sees its loop alone - a = 1, dfeat = G; without a bias A = feat and D is the loop's own dot, so del = der = 0
    # exactly (with one, A - bias is feat up to two roundings: inside the bound, checked by _check); N = 0: no launch
    empty = torch.zeros(0, dtype=torch.int32)
    for both in (False, True):
        _, (_, _, _, Gd, _, _, _), got, _ = _check(empty, empty, 5, hidden, both, 6, True, "edgeless")
        assert torch.equal(got[0], Gd)
        _, (_, _, _, Gd, _, _, _), got, _ = _check(empty, empty, 5, hidden, both, 6, False, "edgeless")
        assert torch.equal(got[0], Gd) and not got[1].any() and not got[2].any()
    v0 = ops.GraphViews(empty.to(dev()), empty.to(dev()), 0)
    A0, st0 = ops.node_attention_sum_stats(z(0, W), v0, z(0, 4), z(0, 4), both=True)
    out = ops.node_attention_sum_bwd(z(0, W), v0, z(0, W), z(0, 4), z(0, 4), A0, st0, both=True)
    assert A0.shape == (0, W) and st0.shape == (0, 8) and out[0].shape == (0, W) and out[1].shape == (0, 4)


def test_torch_operator_equals_the_ctypes_front_end():
    import gnnome_amd.torch_ops  # noqa: F401
    hidden = 128
    src, dst, n = _lengths_graph(hidden)
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    feat, el, er, G, bias = (t.to(dev()) for t in _inputs(n, hidden, 7))
    op = torch.ops.gnnome_hip.node_attention_sum_bwd
    for both in (False, True):
        A, stats = _forward(views, feat, el, er, both, bias)
        want = _backward(views, G, feat, el, er, A, stats, both, bias)
        got = op(G, feat, el, er, A, stats, views.in_ptr, views.srt_src, views.out_ptr, views.out_dst, both, bias, SLOPE)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    meta = op(*(t.to("meta") for t in (G, feat, el, er, A, stats, views.in_ptr, views.srt_src, views.out_ptr, views.out_dst)))
    assert meta[0].shape == G.shape and meta[1].shape == (n, 4) and meta[0].device.type == "meta"
