"""gnnome_node_aggregate_in_f32 (csrc/node_aggregate_in.hip), the kernel alone.  Its oracle is already pinned: the symmetric kernel
gnnome_node_aggregate_f32 on the same inputs with an all-zero A3h table (bwd = 0 / (0 + 1e-6) = +0) - equal BIT FOR BIT on every node
that kernel reduces with its single wave.  Graphs: tests/gated_graphs.py."""
import pytest
import torch

import gnnome_amd  # noqa: F401
from gnnome_amd import ops
from gnnome_amd._lib import NORM_AFFINE, NORM_LAYER

import gated_graphs as gg

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256)
NORMS = (NORM_AFFINE, NORM_LAYER)
_CASES = {}


def dev():
    return torch.device("cuda", 0)


def _inputs(views, rows, hidden, ld_blocks, seed):
    """e[E,H] per sorted position, P[rows, ld_blocks * H] = A1h | A2h | zeros | ..., h[rows,H], scale, shift."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    e = (2.0 * rnd(views.num_edges, hidden)).to(dev())
    P = rnd(rows, ld_blocks * hidden)
    P[:, 2 * hidden:3 * hidden] = 0.0          # the A3h block of the symmetric kernel: all zero
    P = P.to(dev())
    h = rnd(rows, hidden).to(dev())
    scale, shift = (0.5 + torch.rand(hidden, generator=g)).to(dev()), (0.3 * rnd(hidden)).to(dev())
    return e, P, h, scale, shift


def _case(hidden, halo=0, ld_blocks=4):
    """The degree graph of one width with its inputs, built once and shared (read-only)."""
    key = (hidden, halo, ld_blocks)
    if key not in _CASES:
        gr = gg.degree_graph(hidden, halo=halo)
        views = ops.GraphViews(gr["src"].to(dev()), gr["dst"].to(dev()), gr["n"])
        _CASES[key] = (gr, views) + _inputs(views, gr["n"], hidden, ld_blocks, seed=hidden + halo)
    return _CASES[key]


def _blocks(P, hidden):
    return P[:, :hidden], P[:, hidden:2 * hidden], P[:, 2 * hidden:3 * hidden]


def _both(views, e, P, h, scale, shift, norm, hidden, n_out=None):
    A1, A2, Z = _blocks(P, hidden)
    new = ops.node_aggregate_in(e, A1, A2, views, h, norm, scale, shift, num_nodes_out=n_out)
    old = ops.node_aggregate(e, A1, A2, Z, views, h, norm, scale, shift, num_nodes_out=n_out)
    torch.cuda.synchronize()
    rows = h.shape[0] if n_out is None else n_out
    return new[:rows], old[:rows]


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("ld_blocks", (4, 5))
@pytest.mark.parametrize("hidden", WIDTHS)
def test_equals_the_symmetric_kernel_with_a_zero_a3h_table_bit_for_bit(hidden, ld_blocks, norm):
    """In-degrees 0, 1, 2, G-1, G, G+1, 63, 64, 65, 129, parallel edges and self-loops; ld_node = 4H and 5H."""
    gr, views, e, P, h, scale, shift = _case(hidden, ld_blocks=ld_blocks)
    assert set(gg.in_degrees(hidden)) <= set(gr["in_degree"].tolist())
    new, old = _both(views, e, P, h, scale, shift, norm, hidden)
    assert torch.isfinite(new).all()
    assert torch.equal(new, old)
    # in-degree 0: fwd = 0, h' = relu(norm(A1h)) + h - checked against a torch statement on the node without in-edges
    node = int((gr["in_degree"] == 0).nonzero()[0])
    v = P[node, :hidden].double()
    if norm == NORM_LAYER:
        v = (v - v.mean()) / torch.sqrt(v.var(unbiased=False) + 1e-5)
    want = torch.relu(v * scale.double() + shift.double()) + h[node].double()
    assert (new[node].double() - want).abs().max().item() < 1e-5


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("hidden", WIDTHS)
def test_halo_rows_beyond_num_nodes_out_are_read_and_not_written(hidden, norm):
    gr, views, e, P, h, scale, shift = _case(hidden, halo=5)
    n_out = gr["n_out"]
    assert n_out < gr["n"] and int(views.srt_src.max()) >= n_out          # halo rows are referenced
    new, old = _both(views, e, P, h, scale, shift, norm, hidden, n_out=n_out)
    assert torch.equal(new, old)
    A1, A2, _ = _blocks(P, hidden)
    out = torch.full((gr["n"], hidden), 7.0, device=dev())
    ops.node_aggregate_in(e, A1, A2, views, h, norm, scale, shift, num_nodes_out=n_out, node_range=(0, n_out), out=out)
    assert torch.equal(out[:n_out], new) and bool((out[n_out:] == 7.0).all())


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("hidden", WIDTHS)
def test_three_ascending_ranges_equal_the_single_launch_and_two_runs_agree(hidden, norm):
    gr, views, e, P, h, scale, shift = _case(hidden)
    A1, A2, _ = _blocks(P, hidden)
    n = gr["n"]
    whole = ops.node_aggregate_in(e, A1, A2, views, h, norm, scale, shift)
    again = ops.node_aggregate_in(e, A1, A2, views, h, norm, scale, shift)
    cut = torch.full((n, hidden), float("nan"), device=dev())
    bounds = (0, 5, n // 2 + 1, n)          # (no multiples of the four nodes of a workgroup)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ops.node_aggregate_in(e, A1, A2, views, h, norm, scale, shift, node_range=(lo, hi), out=cut)
    torch.cuda.synchronize()
    assert torch.equal(whole, again)
    assert torch.equal(whole, cut)


@pytest.mark.parametrize("hidden", WIDTHS)
def test_64_bit_table_addresses_give_the_same_bits(hidden):
    """gnnome_set_tuning(11, 1): every table row through the 64-bit address form (what rows beyond 2^32 bytes take)."""
    gr, views, e, P, h, scale, shift = _case(hidden)
    A1, A2, _ = _blocks(P, hidden)
    want = ops.node_aggregate_in(e, A1, A2, views, h, NORM_AFFINE, scale, shift)
    ops.set_tuning(11, 1)
    try:
        got = ops.node_aggregate_in(e, A1, A2, views, h, NORM_AFFINE, scale, shift)
    finally:
        ops.set_tuning(11, 0)
    assert torch.equal(got, want)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("hidden", WIDTHS)
def test_one_node_and_no_edges(hidden, norm):
    for src, dst, n in (([0, 0, 0], [0, 0, 0], 1), ([], [], 1), ([], [], 5)):          # N = 1 (self-loops only); N = 1, E = 0; E = 0
        views = ops.GraphViews(torch.tensor(src, dtype=torch.int32, device=dev()), torch.tensor(dst, dtype=torch.int32, device=dev()), n)
        e, P, h, scale, shift = _inputs(views, n, hidden, 4, seed=n + len(src))
        new, old = _both(views, e, P, h, scale, shift, norm, hidden)
        assert torch.isfinite(new).all() and torch.equal(new, old)


def test_a_node_with_5000_in_edges():
    """The hub: 5 000 in-edges among 200 ordinary nodes, H = 128.  Both kernels (the new one: its single wave, two-level sums; the symmetric
    one with A3h = 0: chunk partials) against an fp64 statement of the formula; only the association differs, so the new kernel's error may be
    at most twice the symmetric kernel's.  Measured on an MI355X: 5.870e-07 for both over all rows, 1.692e-07 for both on the hub's row
    (DESIGN.md section 7b)."""
    hidden = 128
    gr = gg.hub_graph()
    views = ops.GraphViews(gr["src"].to(dev()), gr["dst"].to(dev()), gr["n"])
    assert int(views.in_ptr[gr["hub"] + 1] - views.in_ptr[gr["hub"]]) == 5000
    e, P, h, scale, shift = _inputs(views, gr["n"], hidden, 4, seed=9)
    new, old = _both(views, e, P, h, scale, shift, NORM_AFFINE, hidden)
    s, d = views.srt_src.long(), views.srt_dst.long()
    sig = torch.sigmoid(e.double())
    zeros = torch.zeros((gr["n"], hidden), dtype=torch.float64, device=dev())
    fwd = zeros.index_add(0, d, sig * P[:, hidden:2 * hidden].double()[s]) / (zeros.index_add(0, d, sig) + 1e-6)
    want = torch.relu((P[:, :hidden].double() + fwd) * scale.double() + shift.double()) + h.double()
    err_new, err_old = (new.double() - want).abs().max().item(), (old.double() - want).abs().max().item()
    hub_new, hub_old = ((t[gr["hub"]].double() - want[gr["hub"]]).abs().max().item() for t in (new, old))
    print(f"hub of 5000 in-edges, H=128: max-abs error new {err_new:.3e} (hub row {hub_new:.3e}), symmetric kernel with A3h=0 {err_old:.3e} "
          f"(hub row {hub_old:.3e})")
    assert torch.equal(new[:gr["hub"]], old[:gr["hub"]])          # the ordinary nodes are inside the bit-equality claim
    assert err_new <= 2.0 * err_old
    again, _ = _both(views, e, P, h, scale, shift, NORM_AFFINE, hidden)
    assert torch.equal(new, again)
