"""gnnome_node_neighbour_sum_f32 (csrc/node_neighbour.hip) against the fp64 statement of tests/baseline_graphs.py, with the DERIVED
per-row bound |err_i| <= (|N'(i)| + 2) * 2^-23 * sum_j |term_j| - the standard bound of any summation order of fp32 terms, one rounding
per scale multiply; nothing in it is measured."""
import pytest
import torch

import baseline_graphs as bg
from gnnome_amd import ops

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256)


def dev():
    return torch.device("cuda", 0)


def _inputs(n, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, hidden, generator=g)
    return h, 0.25 + torch.rand(n, generator=g), 0.25 + torch.rand(n, generator=g)


def _check(src, dst, n, hidden, both, scaled, seed=1, views=None):
    """One call against the fp64 statement; returns (views, device result, max err / bound)."""
    h, ss, ds = _inputs(n, hidden, seed)
    ss, ds = (ss, ds) if scaled else (None, None)
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n) if views is None else views
    on = lambda t: None if t is None else t.to(dev())  # noqa: E731
    got = ops.node_neighbour_sum(h.to(dev()), views, sscale=on(ss), dscale=on(ds), both=both)
    want, bound = bg.neighbour_sum_f64(h, src, dst, n, ss, ds, both)
    err = (got.cpu().double() - want).abs()
    assert got.shape == (n, hidden) and torch.isfinite(got).all()
    worst = (err / bound.clamp(min=1e-300)).max().item() if n else 0.0
    assert (err <= bound).all(), f"H={hidden} both={both} scaled={scaled}: max err / bound = {worst:.3f}"
    return views, got, worst


@pytest.mark.parametrize("hidden", WIDTHS)
def test_graphs_without_edges(hidden):
    empty = torch.zeros(0, dtype=torch.int32)
    for n in (1, 5):   # N = 1 with E = 0; E = 0 with N = 5: every node sees its own row alone
        for both in (False, True):
            _, got, _ = _check(empty, empty, n, hidden, both, scaled=False)
            h, _, _ = _inputs(n, hidden, 1)
            assert torch.equal(got.cpu(), h)
            _check(empty, empty, n, hidden, both, scaled=True)
    views = ops.GraphViews(empty.to(dev()), empty.to(dev()), 0)   # N = 0: no launch
    out = ops.node_neighbour_sum(torch.zeros(0, hidden, device=dev()), views, both=True)
    assert out.shape == (0, hidden)


@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("hidden", WIDTHS)
def test_list_lengths_parallel_edges_and_self_loops(hidden, both, scaled):
    """In- and out-degrees 0, 1, 2, 63, 64, 65, 129 (and the lane-group counts of `hidden`), parallel edges, self-loops - one graph."""
    src, dst, n = bg.mixed_graph(hidden)
    views, got, worst = _check(src, dst, n, hidden, both, scaled)
    print(f"H={hidden} both={both} scaled={scaled}: max err / bound = {worst:.3f}")
    # two runs leave equal bits
    h, ss, ds = _inputs(n, hidden, 1)
    on = lambda t: t.to(dev()) if scaled else None  # noqa: E731
    assert torch.equal(got, ops.node_neighbour_sum(h.to(dev()), views, sscale=on(ss), dscale=on(ds), both=both))
    # the views of the reversed graph: the two lists exchange their roles
    _check(dst, src, n, hidden, both, scaled, views=views.reversed())


@pytest.mark.parametrize("hidden", WIDTHS)
def test_a_pre_existing_self_loop_counts_once_more(hidden):
    """Node 0 has the edges 0 -> 0, 0 -> 0 and 1 -> 0: N'(0) = {0, 0, 1, 0}; with both lists the two loops come back as out-edges too."""
    src, dst = torch.tensor([0, 0, 1], dtype=torch.int32), torch.tensor([0, 0, 0], dtype=torch.int32)
    h = torch.zeros(2, hidden)
    h[0], h[1] = 1.0, 16.0
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), 2)
    one = ops.node_neighbour_sum(h.to(dev()), views).cpu()
    two = ops.node_neighbour_sum(h.to(dev()), views, both=True).cpu()
    assert torch.equal(one[0], torch.full((hidden,), 19.0)) and torch.equal(one[1], torch.full((hidden,), 16.0))
    assert torch.equal(two[0], torch.full((hidden,), 21.0)) and torch.equal(two[1], torch.full((hidden,), 17.0))


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("hidden", WIDTHS)
def test_a_hub_of_5000_in_edges_among_200_nodes(hidden, both):
    src, dst, n = bg.hub_edges(5000, 200)
    views, got, worst = _check(src, dst, n, hidden, both, scaled=True)
    print(f"hub H={hidden} both={both}: max err / bound = {worst:.3f}")
    h, ss, ds = _inputs(n, hidden, 1)
    assert torch.equal(got, ops.node_neighbour_sum(h.to(dev()), views, sscale=ss.to(dev()), dscale=ds.to(dev()), both=both))
    if both:   # ... and as a hub of 5000 OUT-edges: the transposed list
        _check(dst, src, n, hidden, True, scaled=False)


@pytest.mark.parametrize("hidden", WIDTHS)
def test_column_blocks_of_a_wider_table(hidden):
    """h and out as column blocks of one [N,3H] table: the result equals the dense call's bit for bit, the other columns are untouched."""
    src, dst, n = bg.mixed_graph(hidden)
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    h, ss, ds = (t.to(dev()) for t in _inputs(n, hidden, 2))
    dense = ops.node_neighbour_sum(h, views, sscale=ss, dscale=ds, both=True)
    table = torch.full((n, 3 * hidden), -7.0, device=dev())
    table[:, hidden:2 * hidden] = h
    before = table.clone()
    ret = ops.node_neighbour_sum(table[:, hidden:2 * hidden], views, sscale=ss, dscale=ds, both=True, out=table[:, 2 * hidden:])
    assert ret.data_ptr() == table[:, 2 * hidden:].data_ptr()
    assert torch.equal(table[:, 2 * hidden:], dense)
    assert torch.equal(table[:, :2 * hidden], before[:, :2 * hidden])
    with pytest.raises(Exception, match="alias"):
        ops.node_neighbour_sum(h, views, out=h)


def test_relu_rows_in_place_keeps_nan_and_the_other_columns():
    x = torch.randn(37, 192, generator=torch.Generator().manual_seed(5))
    x[3, 70] = float("nan")
    t = x.to(dev())
    ops.relu_rows(t[:, 64:128])
    got = t.cpu()
    assert torch.equal(got[:, :64], x[:, :64]) and torch.equal(got[:, 128:], x[:, 128:])
    assert torch.equal(got[:, 64:128].nan_to_num(nan=-1.0), torch.relu(x[:, 64:128]).nan_to_num(nan=-1.0))
    assert torch.isnan(got[3, 70]) and int(torch.isnan(got).sum()) == 1


def test_torch_operator_equals_the_ctypes_front_end():
    import gnnome_amd.torch_ops  # noqa: F401
    hidden = 128
    src, dst, n = bg.mixed_graph(hidden)
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    h, ss, ds = (t.to(dev()) for t in _inputs(n, hidden, 3))
    op = torch.ops.gnnome_hip.node_neighbour_sum
    assert torch.equal(op(h, views.in_ptr, views.srt_src), ops.node_neighbour_sum(h, views))
    assert torch.equal(op(h, views.in_ptr, views.srt_src, None, None, ss, ds), ops.node_neighbour_sum(h, views, sscale=ss, dscale=ds))
    assert torch.equal(op(h, views.in_ptr, views.srt_src, views.out_ptr, views.out_dst, ss, ds),
                       ops.node_neighbour_sum(h, views, sscale=ss, dscale=ds, both=True))
    wide = torch.zeros(n, 2 * hidden, device=dev())
    wide[:, hidden:] = h
    assert torch.equal(op(wide[:, hidden:], views.in_ptr, views.srt_src), ops.node_neighbour_sum(h, views))   # a strided h
    meta = op(*(t.to("meta") for t in (h, views.in_ptr, views.srt_src, views.out_ptr, views.out_dst, ss, ds)))
    assert meta.shape == h.shape and meta.device.type == "meta"
