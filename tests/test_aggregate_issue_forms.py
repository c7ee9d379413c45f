"""The aggregation's default item loop (csrc/node_aggregate.hip accumulate_items_lean: scalar loop control, packed products and adds around the
two transcendentals, row addresses from 32-bit byte offsets) against the loop it replaced, kept as tuning variant 16 (accumulate_items_split):
the same items in the same lane groups in the same order through the same operations, so the results are equal BIT FOR BIT - NaN patterns
included - at every width, on both addressing paths (gnnome_set_tuning(11, 1) forces the 64-bit one), with the record form on and off, on plain
and reversed views, with the hub split on and off.  (The record form kept the previous loop in the end - it measured slower with the new one - so its
cases hold trivially today; they stay for the day it changes.)

The graph is built around the list lengths at which the loop changes its path.  G * U items make a step (16 at H = 64, 8 at H = 128, 2 at
H = 256) and 64 a batch; a node's list is its in-edges followed by its out-edges."""
import pytest
import torch

from gnnome_amd import ops

pytestmark = pytest.mark.gpu

N = 2000
HUB = (3000, 1200)   # in + out above the hub threshold of 4096 items


def dev():
    return torch.device("cuda", 0)


def _specs():
    """(in-degree, out-degree) of the probe nodes 0, 1, 2, ..."""
    s = []
    for k in (1, 2, 3, 7, 8, 9, 15, 16, 17):       # 1, G U - 1, G U, G U + 1 of every width: in-only, out-only, both
        s += [(k, 0), (0, k), (k, k)]
    s += [(3, 5), (5, 3), (12, 9), (1, 20), (20, 1)]                               # a step that holds the last in-edges and the first out-edges
    s += [(63, 0), (64, 0), (65, 0), (0, 63), (0, 64), (0, 65), (30, 33), (32, 32), (40, 25)]   # the batch boundary
    s += [(70, 70), (64, 64), (130, 3), (3, 130)]                                  # several batches, the in/out boundary inside a later one
    s += [HUB]
    return s


def _graph():
    g = torch.Generator().manual_seed(11)
    src, dst = [], []
    for node, (din, dout) in enumerate(_specs()):   # neighbours come from the pool 100 .. 1899 (with repeats: duplicate edges)
        nb = torch.randint(100, 1900, (din,), generator=g).tolist()
        src += nb
        dst += [node] * din
        nb = torch.randint(100, 1900, (dout,), generator=g).tolist()
        src += [node] * dout
        dst += nb
    src += [90, 90, 91, 92, 92, 92, 93]
    dst += [90, 90, 92, 91, 91, 91, 93]    # self-loops (one twice), duplicates, a pair of opposite edges
    # nodes 95 .. 99 and 1900 .. 1999 stay isolated (0 and 0)
    return torch.tensor(src, dtype=torch.int32), torch.tensor(dst, dtype=torch.int32)


_CACHE = {}


def _case(hidden, kind):
    key = (hidden, kind)
    if key not in _CACHE:
        src, dst = _graph()
        e = src.numel()
        gen = torch.Generator().manual_seed(hidden + len(kind))
        ee = 2 * torch.randn(e, hidden, generator=gen)
        if kind == "nonfinite":
            r = torch.rand(e, hidden, generator=gen)
            ee[r < 0.01] = float("inf")
            ee[(r >= 0.01) & (r < 0.02)] = float("-inf")
            ee[(r >= 0.02) & (r < 0.03)] = float("nan")
        elif kind == "edge_of_exp":     # |x| around 88: exp(-x) overflows to inf or falls into the denormals
            ee = (86 + 4 * torch.rand(e, hidden, generator=gen)) * torch.where(torch.rand(e, hidden, generator=gen) < 0.5, -1.0, 1.0)
        P = torch.randn(N, 5 * hidden, generator=gen)
        h = torch.randn(N, hidden, generator=gen)
        sc, sh = 0.5 + torch.rand(hidden, generator=gen), torch.randn(hidden, generator=gen)
        views = ops.GraphViews(src.to(dev()), dst.to(dev()), N)
        _CACHE[key] = (views, views.reversed(), ee.to(dev()), P.to(dev()), h.to(dev()), sc.to(dev()), sh.to(dev()))
    return _CACHE[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _outputs(hidden, views, ee, P, h, sc, sh, every_mode):
    A1, A2, A3 = (P[:, i * hidden:(i + 1) * hidden] for i in range(3))
    out = [ops.node_aggregate(ee, A1, A2, A3, views, h, ops.NORM_AFFINE, sc, sh)]
    if every_mode:
        out.append(ops.node_aggregate(ee, A1, A2, A3, views, h, ops.NORM_LAYER, sc, sh))
        out += list(ops.node_aggregate_raw(ee, A1, A2, A3, views, 1, N))
        out += list(ops.node_aggregate_raw(ee, A1, A2, A3, views, 2, N))
        part = torch.zeros_like(out[0])
        ops.node_aggregate(ee, A1, A2, A3, views, h, ops.NORM_AFFINE, sc, sh, node_range=(0, 37), out=part)
        ops.node_aggregate(ee, A1, A2, A3, views, h, ops.NORM_AFFINE, sc, sh, node_range=(37, N), out=part)
        out.append(part)
    return [_bits(t).clone() for t in out]


def _both_loops(hidden, views, tensors, every_mode):
    try:
        ops.set_tuning(7, 16)
        want = _outputs(hidden, views, *tensors, every_mode)
    finally:
        ops.set_tuning(7, 0)
    got = _outputs(hidden, views, *tensors, every_mode)
    return got, want


@pytest.mark.parametrize("kind", ["normal", "nonfinite", "edge_of_exp"])
@pytest.mark.parametrize("hidden", [64, 128, 256])
def test_default_loop_equals_the_loop_it_replaced(hidden, kind):
    plain, rev, *tensors = _case(hidden, kind)
    old = ops.NODE_RECORDS_MAX_HIDDEN
    try:
        ops.NODE_RECORDS_MAX_HIDDEN = 256
        for views in (plain, rev):
            for addr64 in (0, 1):
                for hubs_off in ((0, 1) if kind == "normal" else (0,)):
                    for rec in ((False, True) if hidden == 64 else (False,)):
                        ops.set_tuning(11, addr64)
                        ops.set_tuning(6, hubs_off)
                        where = (hidden, kind, views.transposed, addr64, hubs_off, rec)
                        if rec:
                            with ops.node_records_for(views, hidden) as ctx:
                                assert ctx.on
                                got, want = _both_loops(hidden, views, tensors, False)
                        else:
                            got, want = _both_loops(hidden, views, tensors, kind == "normal")
                        for i, (a, b) in enumerate(zip(got, want)):
                            assert torch.equal(a, b), (where, i, int((a != b).any(1).sum()))
                        if kind == "normal":   # (the oracle is not vacuous: finite rows, and the probes' rows are not all alike)
                            y = got[0].view(torch.float32)
                            assert torch.isfinite(y).all() and y[:60].std() > 0.1
    finally:
        ops.NODE_RECORDS_MAX_HIDDEN = old
        ops.set_tuning(11, 0)
        ops.set_tuning(6, 0)
        ops.set_tuning(7, 0)


def test_the_graph_holds_the_list_lengths_it_claims():
    plain = _case(128, "normal")[0]
    din = (plain.in_ptr[1:] - plain.in_ptr[:-1]).tolist()
    dout = (plain.out_ptr[1:] - plain.out_ptr[:-1]).tolist()
    for node, (a, b) in enumerate(_specs()):
        assert (din[node], dout[node]) == (a, b), node
    assert (din[1999], dout[1999]) == (0, 0) and (din[97], dout[97]) == (0, 0)
    assert din[len(_specs()) - 1] + dout[len(_specs()) - 1] > 4096
    assert (din[90], dout[90]) == (2, 2) and (din[91], dout[91]) == (3, 1)
