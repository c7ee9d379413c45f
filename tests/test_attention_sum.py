"""gnnome_node_attention_sum_f32 (csrc/node_attention.hip) against the fp64 statement of tests/gat_graphs.py, with the DERIVED per-element
bound of attention_sum_f64 (its docstring) - nothing in it is measured.  The bound is asserted on calls without a bias; the bias is the
kernel's last operation and a rounding of its own, so it is checked exactly: out(bias) == out(no bias) + bias, bit for bit."""
import pytest
import torch

import baseline_graphs as bg
import gat_graphs as gg
from gnnome_amd import ops

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256)
CASES = [(h, b) for h in WIDTHS for b in (False, True)]
case = pytest.mark.parametrize("hidden,both", CASES)


def dev():
    return torch.device("cuda", 0)


def _inputs(n, hidden, seed, scale=2.0):
    """feat[n,3H], el / er [n,4] with scores el + er of scale `scale`; the pad column holds NaN (the kernel loads it and must not use it),
    bias[3H]."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(n, 3 * hidden, generator=g)
    el, er = (scale / 2 ** 0.5) * torch.randn(n, 4, generator=g), (scale / 2 ** 0.5) * torch.randn(n, 4, generator=g)
    el[:, 3] = er[:, 3] = float("nan")
    return feat, el, er, 0.1 * torch.randn(3 * hidden, generator=g)


def _views(src, dst, n):
    return ops.GraphViews(src.to(dev()), dst.to(dev()), n)


def _run(views, feat, el, er, both, slope=0.2, bias=None):
    return ops.node_attention_sum(feat.to(dev()), views, el.to(dev()), er.to(dev()), bias=None if bias is None else bias.to(dev()),
                                  negative_slope=slope, both=both)


def _check(src, dst, n, both, feat, el, er, slope=0.2, views=None, what=""):
    """One call (no bias) against the fp64 statement; returns (views, device result, want, bound)."""
    views = _views(src, dst, n) if views is None else views
    got = _run(views, feat, el, er, both, slope)
    want, bound = gg.attention_sum_f64(feat, el, er, src, dst, n, slope, None, both)
    err = (got.cpu().double() - want).abs()
    assert got.shape == feat.shape and torch.isfinite(got).all()
    worst = (err / bound.clamp(min=1e-300)).max().item() if n else 0.0
    print(f"{what} H={feat.shape[1] // 3} both={both} slope={slope}: max err / bound = {worst:.3f}")
    assert (err <= bound).all(), f"{what} H={feat.shape[1] // 3} both={both}: max err / bound = {worst:.3f}"
    return views, got, want, bound


@case
def test_list_lengths_parallel_edges_and_self_loops(hidden, both):
    """In- and out-degrees 0, 1, 2, 63, 64, 65, 129 (and the lane-group counts of `hidden`), parallel edges, self-loops - one graph."""
    src, dst, n = bg.mixed_graph(hidden)
    feat, el, er, bias = _inputs(n, hidden, 1)
    views, got, _, _ = _check(src, dst, n, both, feat, el, er, what="mixed")
    assert torch.equal(got, _run(views, feat, el, er, both))                                     # two runs leave equal bits
    assert torch.equal(_run(views, feat, el, er, both, bias=bias), got + bias.to(dev()))         # the bias: one more rounding, exactly


@case
def test_reversed_views_are_the_swapped_edge_list(hidden, both):
    src, dst, n = bg.mixed_graph(hidden)
    feat, el, er, _ = _inputs(n, hidden, 2)
    _check(dst, src, n, both, feat, el, er, views=_views(src, dst, n).reversed(), what="reversed")


def _hub_with_a_star(hidden):
    """hub_edges(5000, 200) plus one new node, the star, whose single edge star -> hub is the LAST item of the hub's in-list."""
    src, dst, n = bg.hub_edges(5000, 200)
    hub, star = n - 1, n
    src, dst = torch.cat([src, torch.tensor([star], dtype=src.dtype)]), torch.cat([dst, torch.tensor([hub], dtype=dst.dtype)])
    views = _views(src, dst, n + 1)
    lo, hi = (int(v) for v in views.in_ptr[hub:hub + 2].cpu())
    where = (views.srt_src[lo:hi].cpu() == star).nonzero().flatten()
    length = hi - lo
    assert length == 5001 and where.numel() == 1 and int(where) >= (length - 1) // 128 * 128, "the star is not in the hub's last 128-item block"
    return src, dst, n + 1, hub, star, views


@case
def test_a_hub_of_5000_in_edges_among_200_nodes(hidden, both):
    src, dst, n = bg.hub_edges(5000, 200)
    feat, el, er, _ = _inputs(n, hidden, 3)
    views, got, _, _ = _check(src, dst, n, both, feat, el, er, what="hub")
    assert torch.equal(got, _run(views, feat, el, er, both))
    if both:   # ... and as a hub of 5000 OUT-edges: the transposed list
        _check(dst, src, n, True, feat, el, er, what="hub, transposed")


@case
def test_a_dominant_score_in_the_last_block_of_a_hub(hidden, both):
    """One neighbour with el = +30 among 5000 with scores about 0, in the LAST 128-item block of the hub's list: the hub's row is that
    neighbour's row.  A maximum taken per block (without a rescale) would weigh every block's own best item like it."""
    src, dst, n, hub, star, views = _hub_with_a_star(hidden)
    feat, el, er, _ = _inputs(n, hidden, 4, scale=0.01)
    el[star, :3] = 30.0
    _, got, want, bound = _check(src, dst, n, both, feat, el, er, views=views, what="hub, dominant last")
    err = (got[hub].cpu().double() - feat[star].double()).abs()
    assert (err <= bound[hub]).all(), f"hub row against the dominant neighbour's row: max err / bound = {(err / bound[hub]).max().item():.3f}"


@pytest.mark.parametrize("hidden", WIDTHS)
def test_graphs_without_edges(hidden):
    empty = torch.zeros(0, dtype=torch.int32)
    for n in (1, 5):   # N = 1 with E = 0; E = 0 with N = 5: every node sees its own loop alone, weight exp(0) / exp(0) = 1
        feat, el, er, bias = _inputs(n, hidden, 5)
        views = _views(empty, empty, n)
        for both in (False, True):
            assert torch.equal(_run(views, feat, el, er, both, bias=bias).cpu(), feat + bias)
            assert torch.equal(_run(views, feat, el, er, both).cpu(), feat)
    views = _views(empty, empty, 0)   # N = 0: no launch
    z = torch.zeros(0, 3 * hidden, device=dev())
    out = ops.node_attention_sum(z, views, torch.zeros(0, 4, device=dev()), torch.zeros(0, 4, device=dev()), both=True)
    assert out.shape == (0, 3 * hidden)


@case
def test_nodes_that_see_only_their_loop_come_out_exact(hidden, both):
    """A bipartite graph 0..5 -> 6..11.  Directed, a source's N' is its loop alone: out = feat + bias bit for bit."""
    src, dst, n = torch.arange(0, 6, dtype=torch.int32), torch.arange(6, 12, dtype=torch.int32), 12
    feat, el, er, bias = _inputs(n, hidden, 6)
    views, _, _, _ = _check(src, dst, n, both, feat, el, er, what="bipartite")
    got = _run(views, feat, el, er, both, bias=bias).cpu()
    alone = slice(0, 6) if not both else slice(0, 0)     # with both lists a source sees its target too
    assert torch.equal(got[alone], (feat + bias)[alone])
    if not both:
        assert not torch.equal(got[6:], (feat + bias)[6:])


@case
def test_equal_scores_are_the_mean_of_the_neighbour_sum_kernel(hidden, both):
    """el = er = 0: every weight is 1 / |N'(i)|, so each head equals gnnome_node_neighbour_sum_f32 with dscale = 1 / din' - within the sum
    of the two kernels' derived bounds."""
    src, dst, n = bg.mixed_graph(hidden)
    feat, _, _, _ = _inputs(n, hidden, 7)
    zeros = torch.zeros(n, 4)
    views, got, _, bound = _check(src, dst, n, both, feat, zeros, zeros, what="equal scores")
    gd = bg.neighbour_lists(src, dst, n, both)[1]
    dinv = (1.0 / torch.bincount(gd, minlength=n).float())
    featd = feat.to(dev())
    for k in range(3):
        cols = slice(k * hidden, (k + 1) * hidden)
        mean = ops.node_neighbour_sum(featd[:, cols], views, dscale=dinv.to(dev()), both=both)
        _, nbound = bg.neighbour_sum_f64(feat[:, cols], src, dst, n, None, dinv, both)
        assert ((got[:, cols] - mean).abs().cpu().double() <= bound[:, cols] + nbound).all()


@case
def test_the_negative_branch_takes_the_slope(hidden, both):
    src, dst, n = bg.mixed_graph(hidden)
    feat, el, er, _ = _inputs(n, hidden, 8)
    el, er = -el.abs() - 0.01, -er.abs() - 0.01     # el + er < 0 for every pair
    views, leaky, _, _ = _check(src, dst, n, both, feat, el, er, slope=0.2, what="negative, slope 0.2")
    _, flat, _, _ = _check(src, dst, n, both, feat, el, er, slope=0.0, views=views, what="negative, slope 0.0")
    assert (leaky - flat).abs().max().item() > 1e-3


@case
def test_scores_spread_over_120(hidden, both):
    """el uniform in +-60 (the degree-65 and degree-129 nodes among them): exp(s - max) spans more than fp32's range; finite and in bound."""
    src, dst, n = bg.mixed_graph(hidden)
    feat, el, er, _ = _inputs(n, hidden, 9)
    el[:, :3] = 120.0 * torch.rand(n, 3, generator=torch.Generator().manual_seed(10)) - 60.0
    _check(src, dst, n, both, feat, el, er, what="spread")


@case
def test_a_nan_reaches_exactly_the_nodes_that_see_it(hidden, both):
    src, dst, n = bg.mixed_graph(hidden)
    feat, el, er, _ = _inputs(n, hidden, 11)
    views = _views(src, dst, n)
    gs, gd = bg.neighbour_lists(src, dst, n, both)
    poisoned = int(src[0])                                   # a row that is some node's neighbour (and its own)
    sees = torch.zeros(n, dtype=torch.bool)
    sees[gd[gs == poisoned]] = True
    assert sees[poisoned] and 1 < int(sees.sum()) < n
    bad_feat = feat.clone()
    bad_feat[poisoned] = float("nan")
    finite = torch.isfinite(_run(views, bad_feat, el, er, both).cpu()).view(n, 3, hidden)
    assert torch.equal(~finite.all(2), sees[:, None].expand(n, 3))          # all three heads of the nodes that see the row, nothing else
    assert not finite[sees].any()
    bad_el = el.clone()
    bad_el[poisoned, 1] = float("nan")                       # one head's score
    finite = torch.isfinite(_run(views, feat, bad_el, er, both).cpu()).view(n, 3, hidden)
    assert finite[:, 0].all() and finite[:, 2].all()
    assert torch.equal(~finite[:, 1].all(1), sees) and not finite[:, 1][sees].any()
    bad_er = er.clone()
    bad_er[poisoned, 2] = float("nan")                       # er is the DESTINATION's: only the node itself
    finite = torch.isfinite(_run(views, feat, el, bad_er, both).cpu()).view(n, 3, hidden)
    only = torch.zeros(n, dtype=torch.bool)
    only[poisoned] = True
    assert finite[:, 0].all() and finite[:, 1].all() and torch.equal(~finite[:, 2].all(1), only)


@case
def test_column_blocks_of_wider_tables(hidden, both):
    """feat, el, er as blocks of one [N, 3H + 64] table (the projection's layout) and out as a block of another: the dense call's bits, the
    other columns untouched; out aliasing feat is refused."""
    src, dst, n = bg.mixed_graph(hidden)
    feat, el, er, bias = (t.to(dev()) for t in _inputs(n, hidden, 12))
    views = _views(src, dst, n)
    dense = ops.node_attention_sum(feat, views, el, er, bias=bias, both=both)
    W = 3 * hidden
    P = torch.full((n, W + 64), -7.0, device=dev())
    P[:, :W], P[:, W:W + 4], P[:, W + 4:W + 8] = feat, el, er
    T = torch.full((n, W + 64), -5.0, device=dev())
    before = P.clone()
    ret = ops.node_attention_sum(P[:, :W], views, P[:, W:W + 4], P[:, W + 4:W + 8], bias=bias, both=both, out=T[:, 64:])
    assert ret.data_ptr() == T[:, 64:].data_ptr()
    assert torch.equal(T[:, 64:], dense) and bool((T[:, :64] == -5.0).all())
    assert torch.equal(P.nan_to_num(nan=3.0), before.nan_to_num(nan=3.0))
    with pytest.raises(Exception, match="alias"):
        ops.node_attention_sum(feat, views, el, er, both=both, out=feat)


def test_refusals():
    src, dst, n = bg.mixed_graph(64)
    views = _views(src, dst, n)
    z = lambda *shape: torch.zeros(*shape, device=dev())  # noqa: E731
    with pytest.raises(Exception, match="64,128,256"):
        ops.node_attention_sum(z(n, 3 * 32), views, z(n, 4), z(n, 4))
    with pytest.raises(ValueError, match=r"\[N, 4\]"):
        ops.node_attention_sum(z(n, 192), views, z(n, 3), z(n, 4))
    with pytest.raises(ValueError, match="rows"):
        ops.node_attention_sum(z(n + 1, 192), views, z(n + 1, 4), z(n + 1, 4))


def test_torch_operator_equals_the_ctypes_front_end():
    import gnnome_amd.torch_ops  # noqa: F401
    hidden = 128
    src, dst, n = bg.mixed_graph(hidden)
    views = _views(src, dst, n)
    feat, el, er, bias = (t.to(dev()) for t in _inputs(n, hidden, 13))
    op = torch.ops.gnnome_hip.node_attention_sum
    assert torch.equal(op(feat, el, er, views.in_ptr, views.srt_src), ops.node_attention_sum(feat, views, el, er))
    assert torch.equal(op(feat, el, er, views.in_ptr, views.srt_src, None, None, bias, 0.1),
                       ops.node_attention_sum(feat, views, el, er, bias=bias, negative_slope=0.1))
    assert torch.equal(op(feat, el, er, views.in_ptr, views.srt_src, views.out_ptr, views.out_dst, bias),
                       ops.node_attention_sum(feat, views, el, er, bias=bias, both=True))
    P = torch.zeros(n, 3 * hidden + 64, device=dev())
    W = 3 * hidden
    P[:, :W], P[:, W:W + 4], P[:, W + 4:W + 8] = feat, el, er
    assert torch.equal(op(P[:, :W], P[:, W:W + 4], P[:, W + 4:W + 8], views.in_ptr, views.srt_src), ops.node_attention_sum(feat, views, el, er))
    meta = op(*(t.to("meta") for t in (feat, el, er, views.in_ptr, views.srt_src, views.out_ptr, views.out_dst, bias)))
    assert meta.shape == feat.shape and meta.device.type == "meta"
