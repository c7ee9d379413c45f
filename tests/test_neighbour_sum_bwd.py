"""gnnome_node_neighbour_sum_bwd_f32 and gnnome_relu_mul_rows_f32 (csrc/node_neighbour_bwd.hip).  Without its epilogue the backward
kernel must leave the BITS of the forward kernel on the reversed graph (one association, csrc/node_neighbour.h); independently of that
kernel it is held to the fp64 statement of tests/baseline_graphs.py on the swapped edge list with the derived bound of
test_neighbour_sum.py; the epilogue must equal the four element-wise fp32 passes it replaces bit for bit."""
import pytest
import torch

import baseline_graphs as bg
from gnnome_amd import ops

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256)
NAN = float("nan")


def dev():
    return torch.device("cuda", 0)


def _inputs(n, hidden, seed):
    """g, rscale, oscale, add, mult (with zeros), y (zeros, negatives, one NaN) on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(n, hidden, generator=gen)
    rs, osc = 0.25 + torch.rand(n, generator=gen), 0.25 + torch.rand(n, generator=gen)
    add = torch.randn(n, hidden, generator=gen)
    mult = (torch.rand(n, hidden, generator=gen) >= 0.25).float() / 0.75
    y = torch.relu(torch.randn(n, hidden, generator=gen))
    if n:
        y[0, 1], y[n - 1, hidden - 1], y[n // 2, 3] = -2.0, -0.5, NAN
        assert (y == 0).any() and (y < 0).any() and (mult == 0).any()
    return g, rs, osc, add, mult, y


def _epilogue(s, osc=None, add=None, mult=None, y=None):
    """The four element-wise fp32 passes with torch, one rounding each."""
    v = s
    if osc is not None:
        v = osc[:, None] * v
    if add is not None:
        v = add + v
    if mult is not None:
        v = v * mult
    if y is not None:
        v = torch.where(y > 0, v, torch.zeros_like(v))
    return v


def _same(a, b):
    return torch.equal(a.nan_to_num(nan=12345.0), b.nan_to_num(nan=12345.0))


def _views(src, dst, n):
    return ops.GraphViews(src.to(dev()), dst.to(dev()), n)


def _check_plain(src, dst, n, hidden, both, scaled, views=None, seed=1):
    """No epilogue: the forward kernel's bits on the reversed graph, the fp64 statement's value on the swapped edge list, equal bits twice."""
    g, rs, osc, *_ = _inputs(n, hidden, seed)
    rs, osc = (rs, osc) if scaled else (None, None)
    views = _views(src, dst, n) if views is None else views
    on = lambda t: None if t is None else t.to(dev())  # noqa: E731
    got = ops.node_neighbour_sum_bwd(g.to(dev()), views, rscale=on(rs), oscale=on(osc), both=both)
    fwd = ops.node_neighbour_sum(g.to(dev()), views.reversed(), sscale=on(rs), dscale=on(osc), both=both)
    assert got.shape == (n, hidden) and torch.equal(got, fwd)
    want, bound = bg.neighbour_sum_f64(g, dst, src, n, rs, osc, both)
    err = (got.cpu().double() - want).abs()
    worst = (err / bound.clamp(min=1e-300)).max().item()
    assert (err <= bound).all(), f"H={hidden} both={both} scaled={scaled}: max err / bound = {worst:.3f}"
    assert torch.equal(got, ops.node_neighbour_sum_bwd(g.to(dev()), views, rscale=on(rs), oscale=on(osc), both=both))
    return views, worst


@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("hidden", WIDTHS)
def test_without_epilogue_the_forward_kernels_bits_on_the_reversed_graph(hidden, both, scaled):
    src, dst, n = bg.mixed_graph(hidden)   # in- and out-degrees 0, 1, 2, 63, 64, 65, 129, parallel edges, self-loops
    views, worst = _check_plain(src, dst, n, hidden, both, scaled)
    print(f"H={hidden} both={both} scaled={scaled}: max err / bound = {worst:.3f}")
    _check_plain(dst, src, n, hidden, both, scaled, views=views.reversed())   # transposed views exchange the two lists


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("hidden", WIDTHS)
def test_a_hub_of_5000_out_edges(hidden, both):
    dst, src, n = bg.hub_edges(5000, 200)   # src and dst swapped: the hub's 5000 in-edges become out-edges, above the two-level threshold
    assert torch.bincount(src.long(), minlength=n).max().item() >= 5000
    _, worst = _check_plain(src, dst, n, hidden, both, scaled=True)
    print(f"hub H={hidden} both={both}: max err / bound = {worst:.3f}")


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("hidden", WIDTHS)
def test_epilogue_equals_the_four_elementwise_passes(hidden, both):
    src, dst, n = bg.mixed_graph(hidden)
    views = _views(src, dst, n)
    g, rs, osc, add, mult, y = (t.to(dev()) for t in _inputs(n, hidden, 2))
    s = ops.node_neighbour_sum_bwd(g, views, rscale=rs, both=both)
    full = dict(osc=osc, add=add, mult=mult, y=y)
    for absent in (None, "osc", "add", "mult", "y"):
        kw = {k: (None if k == absent else v) for k, v in full.items()}
        got = ops.node_neighbour_sum_bwd(g, views, rscale=rs, oscale=kw["osc"], both=both, add=kw["add"], y=kw["y"], mult=kw["mult"])
        want = _epilogue(s, **kw)
        assert _same(got, want), f"H={hidden} both={both} without {absent}"
        if absent != "y":   # a NaN in y closes the gate, as gnnome_relu_bwd_f32 does
            assert got[n // 2, 3].item() == 0.0 and got[0, 1].item() == 0.0
    # the SAGE set (no oscale) and the GCN set (oscale and y only)
    assert _same(ops.node_neighbour_sum_bwd(g, views, rscale=rs, both=both, add=add, mult=mult, y=y), _epilogue(s, None, add, mult, y))
    assert _same(ops.node_neighbour_sum_bwd(g, views, rscale=rs, oscale=osc, both=both, y=y), _epilogue(s, osc, None, None, y))


@pytest.mark.parametrize("hidden", WIDTHS)
def test_row_strided_operands(hidden):
    """g the right half and add the left half of one [N,2H] table, out a column block of a wider table whose other columns stay."""
    src, dst, n = bg.mixed_graph(hidden)
    views = _views(src, dst, n)
    g, rs, osc, add, mult, y = (t.to(dev()) for t in _inputs(n, hidden, 3))
    dense = ops.node_neighbour_sum_bwd(g, views, rscale=rs, oscale=osc, both=True, add=add, mult=mult, y=y)
    dT = torch.cat([add, g], 1)
    wide_y = torch.cat([y, torch.full_like(y, 5.0)], 1)
    table = torch.full((n, 3 * hidden), -7.0, device=dev())
    ret = ops.node_neighbour_sum_bwd(dT[:, hidden:], views, rscale=rs, oscale=osc, both=True, add=dT[:, :hidden], mult=mult,
                                     y=wide_y[:, :hidden], out=table[:, hidden:2 * hidden])
    assert ret.data_ptr() == table[:, hidden:2 * hidden].data_ptr()
    assert _same(table[:, hidden:2 * hidden], dense)
    assert (table[:, :hidden] == -7.0).all() and (table[:, 2 * hidden:] == -7.0).all()


@pytest.mark.parametrize("hidden", WIDTHS)
def test_graphs_without_edges_and_without_nodes(hidden):
    empty = torch.zeros(0, dtype=torch.int32)
    for n in (1, 5):
        views = _views(empty, empty, n)
        g, rs, osc, add, mult, y = (t.to(dev()) for t in _inputs(n, hidden, 4))
        for both in (False, True):
            got = ops.node_neighbour_sum_bwd(g, views, rscale=rs, oscale=osc, both=both)
            assert torch.equal(got, osc[:, None] * (rs[:, None] * g))
            got = ops.node_neighbour_sum_bwd(g, views, rscale=rs, oscale=osc, both=both, add=add, mult=mult, y=y)
            assert _same(got, _epilogue(rs[:, None] * g, osc, add, mult, y))
    views = _views(empty, empty, 0)   # N = 0: no launch
    z = torch.zeros(0, hidden, device=dev())
    assert ops.node_neighbour_sum_bwd(z, views, both=True, add=z, mult=z, y=z).shape == (0, hidden)


def test_refusals():
    src, dst, n = bg.mixed_graph(64)
    views = _views(src, dst, n)
    g = torch.randn(n, 64, device=dev())
    with pytest.raises(Exception, match="64,128,256"):
        ops.node_neighbour_sum_bwd(torch.randn(n, 96, device=dev()), views)
    wide = torch.randn(n, 132, device=dev())
    with pytest.raises(Exception, match="aligned"):
        ops.node_neighbour_sum_bwd(wide[:, 1:65], views)            # rows that start 4 bytes into a 16-byte line
    with pytest.raises(Exception, match="aligned"):
        ops.node_neighbour_sum_bwd(g, views, add=wide[:, 2:66])
    with pytest.raises(Exception, match="alias"):
        ops.node_neighbour_sum_bwd(g, views, out=g)
    with pytest.raises(Exception, match="alias"):
        ops.node_neighbour_sum_bwd(g, views, add=wide[:, :64], out=wide[:, :64])
    with pytest.raises(ValueError, match="rows"):
        ops.node_neighbour_sum_bwd(g[:5], views)
    with pytest.raises(ValueError, match="mult"):
        ops.relu_mul_rows(g, None)


@pytest.mark.parametrize("relu", (True, False))
def test_relu_mul_rows_in_place_keeps_nan_and_the_other_columns(relu):
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(37, 192, generator=gen)
    x[3, 70] = NAN
    mult = torch.cat([torch.zeros(37, 64), (torch.rand(37, 64, generator=gen) >= 0.5).float() * 2.0], 1)   # a block of a wider mask
    mult[3, 64 + 6] = 0.0   # the NaN meets a dropped element: NaN * 0 stays NaN
    t, m = x.to(dev()), mult.to(dev())
    ret = ops.relu_mul_rows(t[:, 64:128], m[:, 64:], relu=relu)
    assert ret.data_ptr() == t[:, 64:128].data_ptr()
    got = t.cpu()
    want = (torch.relu(x[:, 64:128]) if relu else x[:, 64:128]) * mult[:, 64:]
    assert torch.equal(got[:, :64], x[:, :64]) and torch.equal(got[:, 128:], x[:, 128:])
    assert _same(got[:, 64:128], want)
    assert torch.isnan(got[3, 70]) and int(torch.isnan(got).sum()) == 1


def test_torch_operator_equals_the_ctypes_front_end():
    import gnnome_amd.torch_ops  # noqa: F401
    hidden = 128
    src, dst, n = bg.mixed_graph(hidden)
    views = _views(src, dst, n)
    g, rs, osc, add, mult, y = (t.to(dev()) for t in _inputs(n, hidden, 6))
    op = torch.ops.gnnome_hip.node_neighbour_sum_bwd
    assert torch.equal(op(g, views.out_ptr, views.out_dst), ops.node_neighbour_sum_bwd(g, views))
    assert _same(op(g, views.out_ptr, views.out_dst, None, None, rs, osc, None, None, y),
                 ops.node_neighbour_sum_bwd(g, views, rscale=rs, oscale=osc, y=y))
    dT = torch.cat([add, g], 1)
    assert _same(op(dT[:, hidden:], views.out_ptr, views.out_dst, views.in_ptr, views.srt_src, rs, None, dT[:, :hidden], mult, y),
                 ops.node_neighbour_sum_bwd(g, views, rscale=rs, both=True, add=add, mult=mult, y=y))
    meta = op(*(t.to("meta") for t in (g, views.out_ptr, views.out_dst, views.in_ptr, views.srt_src, rs, osc, add, mult, y)))
    assert meta.shape == g.shape and meta.device.type == "meta"
