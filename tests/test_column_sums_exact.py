"""The deterministic column sums (gnnome_amd/csrc/train_elementwise.hip: column_walk / column_reduce / column_fold / k_col_finish) on the
borders of their row walk, bit for bit.

The skeleton: a workgroup of 256 threads covers rpb = 1024 / H rows per pass.  col_grid picks ceil(passes / 4) workgroups, at most 1024, cut
to a multiple of 8 from 16 on.  When the grid is a multiple of 8, every XCD (workgroup b runs on XCD b % 8) walks its OWN eighth of the rows,
rounded up to whole passes (per_xcd), its workgroups interleaved inside it; otherwise the workgroups stride over all rows.  col_grid and
column_walk are restated below for ONE purpose: the CPU tests show that each row count of CASES sits where its name says (and that the
restated walk visits every row exactly once there).  The kernels are never compared with the restatement.

The device tests use integer inputs - for agg_edge_bwd_stats the HALVES recipe of tests/aggregate_graphs.py (gates of 0 give a sigmoid of
exactly 0.5, every term a multiple of 1/4) - whose sums of |terms| stay below 2^24 units (the CPU test asserts the worst case per entry and
row count, the device tests the inputs they draw), so the int64 column sums are the one fp32 result in any order.  One row carries a large
value (MARK), the last row and the first row of the last XCD range in turn: a lost or doubled row shows by its size in the message."""
import types

import pytest
import torch

import aggregate_graphs as ag
from gnnome_amd import ops

THREADS, XCDS, MAX_BLOCKS, EW_CAP = 256, 8, 1024, 256 * 8        # kEwThreads, kXcds, kColMaxBlocks, ew_grid's cap (8 workgroups per CU)
WIDTHS = (16, 32, 64, 128, 256)
EDGE_WIDTHS = (64, 128, 256)
MARK = 1000.0
NODES = 37

# name -> (row count from rpb, the grid the restated col_grid must give it); what else each name claims is asserted in the CPU test below
CASES = {
    "one row": (lambda rpb: 1, 1),
    "rpb - 1": (lambda rpb: rpb - 1, 1),
    "rpb": (lambda rpb: rpb, 1),
    "rpb + 1": (lambda rpb: rpb + 1, 1),
    "29 rpb + 1: a grid of 8, one workgroup per XCD": (lambda rpb: 29 * rpb + 1, 8),
    "60 rpb: the last strided grid, 15": (lambda rpb: 60 * rpb, 15),
    "60 rpb + 1: 16 workgroups": (lambda rpb: 60 * rpb + 1, 16),
    "64 rpb + 1: the last XCD's range is partial": (lambda rpb: 64 * rpb + 1, 16),
    "92 rpb: 23 cut to 16": (lambda rpb: 92 * rpb, 16),
    "4096 rpb + 1: capped at 1024": (lambda rpb: 4096 * rpb + 1, 1024),
    "8193 rpb + 1: capped twice": (lambda rpb: 8192 * rpb + rpb + 1, 1024),
}


def col_grid(rows, H):
    rpb = THREADS // (H // 4)
    passes = -(-rows // rpb)
    g = min(max(-(-(passes * THREADS // 4) // THREADS), 1), EW_CAP)
    uncut = min(g, MAX_BLOCKS)
    return (uncut // XCDS * XCDS if uncut >= 2 * XCDS else uncut), g


def column_walk(rows, H, grid, b, per_xcd=None):
    """Workgroup b's passes: (first row of the first pass, end of its rows, stride between passes) - a pass is rpb consecutive rows."""
    rpb = THREADS // (H // 4)
    if grid % XCDS == 0:
        per_xcd = per_xcd_rows(rows, H) if per_xcd is None else per_xcd
        r0 = (b % XCDS) * per_xcd
        return r0 + (b // XCDS) * rpb, min(rows, r0 + per_xcd), (grid // XCDS) * rpb
    return b * rpb, rows, grid * rpb


def per_xcd_rows(rows, H):
    rpb = THREADS // (H // 4)
    return -(-(-(-rows // XCDS)) // rpb) * rpb


def mark_rows(rows, H):
    """The last row, and the first row of the last XCD range that has rows (a strided grid: of the last workgroup that has rows)."""
    grid, _ = col_grid(rows, H)
    rpb = THREADS // (H // 4)
    if grid % XCDS == 0:
        per = per_xcd_rows(rows, H)
        return [rows - 1, max(x * per for x in range(XCDS) if x * per < rows)]
    return [rows - 1, max(b * rpb for b in range(grid) if b * rpb < rows)]


def worst_case_units(rows):
    """Per entry, the largest possible sum of |terms| of one column sum over `rows` rows of the inputs below, in the units that make the
    terms integers (1, or 1/4 for the edge pass) - one MARK row, everything else at its largest magnitude, products counted factor by factor."""
    m, b = int(MARK), ag.BACKWARD_MAX
    return {
        "colsum2(x)": max(b * (rows - 1) + m, b * b * (rows - 1) + m * m),
        "colsum2(x, y)": b * b * (rows - 1) + m * (b + 1),
        "colsum2(x, center)": (b + 1) ** 2 * (rows - 1) + (m + 1) ** 2,                         # |x - c| <= |x| + 1
        "bn_bwd_stats": 2 * b * b * (rows - 1) + 2 * b * m,                                    # |dy| (|x| + |mean|)
        # de' in quarters: 4 |de0| + (|Tf A2| + |Uf| + |Tb A3| + |Ub|) <= 4 b + 2 b^2 + 2 b, times |xe| + |mean| <= 2 b in s2
        "agg_edge_bwd_stats": 2 * b * ((4 * b + 2 * b * b + 2 * b) * (rows - 1) + 4 * m + 2 * b * b + 2 * b),
    }


def _visits(walks, rows, rpb):
    """How often each row is visited by the given walks (a pass covers rpb consecutive rows, cut at the walk's end)."""
    seen = torch.zeros(rows + 1, dtype=torch.int64)
    for first, end, step in walks:
        starts = torch.arange(first, max(end, first), step)
        starts = starts[starts < end]
        seen.index_add_(0, starts, torch.ones_like(starts))
        seen.index_add_(0, torch.clamp(starts + rpb, max=end), -torch.ones_like(starts))
    return seen.cumsum(0)[:rows]


@pytest.mark.parametrize("H", WIDTHS)
def test_every_row_count_sits_on_the_border_it_is_named_for(H):
    rpb = 1024 // H
    for name, (rows_of, want_grid) in CASES.items():
        rows = rows_of(rpb)
        assert rows >= 1
        grid, uncapped = col_grid(rows, H)
        assert grid == want_grid, (name, grid)
        walks = [column_walk(rows, H, grid, b) for b in range(grid)]
        per = per_xcd_rows(rows, H)
        last_xcd = min(rows, 8 * per) - 7 * per
        if name.startswith("29"):
            assert grid % XCDS == 0 and 0 < last_xcd < per
        if name.startswith("60 rpb:"):
            assert grid % XCDS != 0 and col_grid(rows + 1, H)[0] == 16                          # the per-XCD walk starts one row later
        if name.startswith("60 rpb +"):
            assert col_grid(rows - 1, H)[0] == 15 and per % rpb == 0 and per * XCDS > rows      # per_xcd is ROUNDED UP to whole passes here ...
            assert -(-rows // XCDS) % rpb != 0                                                  # ... the plain eighth is no multiple of rpb
        if name.startswith("64"):
            assert 0 < last_xcd < per and last_xcd % rpb != 0
        if name.startswith("92"):
            assert uncapped == 23 and all(w[2] == 2 * rpb for w in walks) and 0 < last_xcd < per
        if name.startswith("4096"):
            assert uncapped == 1025 and col_grid(rows - 1, H)[1] == 1024
            assert max(-(-(w[1] - w[0]) // w[2]) for w in walks) >= 4                           # several passes per workgroup
        if name.startswith("8193"):
            assert uncapped == EW_CAP and max(-(-(w[1] - w[0]) // w[2]) for w in walks) >= 8
        # the restated walk visits every row exactly once
        assert bool((_visits(walks, rows, rpb) == 1).all()), name
        if grid % XCDS == 0:
            # What the rounding of per_xcd is NOT for: an eighth that is no multiple of rpb still gives every row to one thread (the passes of
            # an XCD's workgroups tile its range from its first row on, wherever that is) - the rounding aligns the passes, it carries no row.
            # An eighth rounded DOWN before it is rounded up to passes loses the last rows, at the "+ 1" counts: that the device tests catch.
            eighth = -(-rows // XCDS)
            assert bool((_visits([column_walk(rows, H, grid, b, eighth) for b in range(grid)], rows, rpb) == 1).all()), name
            floor = -(-(rows // XCDS) // rpb) * rpb
            lost = _visits([column_walk(rows, H, grid, b, floor) for b in range(grid)], rows, rpb)
            assert bool((lost == 1).all()) == (XCDS * floor >= rows) and (name[:2] not in ("64", "40") or int(lost[rows - 1]) == 0), name
        marks = mark_rows(rows, H)
        assert marks[0] == rows - 1 and 0 <= marks[1] < rows and (grid % XCDS != 0 or marks[1] % per == 0)
        # the condition of the exact recipes, worst case
        units = {k: v for k, v in worst_case_units(rows).items() if k != "agg_edge_bwd_stats" or H in EDGE_WIDTHS}
        assert max(units.values()) < ag.EXACT_LIMIT, (name, units)


# ---------------------------------------------------------------------------------------------- on the device

def dev():
    return torch.device("cuda", 0)


def _ints(g, *shape):
    return torch.randint(-ag.BACKWARD_MAX, ag.BACKWARD_MAX + 1, shape, generator=g, device=dev()).float()


def _explain(got, want, rows, mark):
    bad = torch.nonzero(got != want).flatten()
    c = int(bad[0])
    return (f"{bad.numel()} columns differ, first {c}: got {got[c].item()!r} want {want[c].item()!r}, difference "
            f"{got[c].item() - want[c].item()!r} ({rows} rows, the row of {MARK} is {mark})")


def _assert_sums(got, want64, bound, rows, mark, what):
    assert int(bound) < ag.EXACT_LIMIT, (what, int(bound))
    for k, (g, w) in enumerate(zip(got, want64)):
        assert torch.equal(g, w.float()), (what, f"s{k + 1}", _explain(g, w.float(), rows, mark))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("H", WIDTHS)
def test_colsum2_and_bn_bwd_stats_are_the_int64_column_sums(H, case):
    rows = CASES[case][0](1024 // H)
    g = torch.Generator(device=dev()).manual_seed(rows + H)
    x, y, dy = _ints(g, rows, H), _ints(g, rows, H), _ints(g, rows, H)
    c = torch.randint(-1, 2, (H,), generator=g, device=dev()).float()
    mean = _ints(g, H)
    scale = torch.randint(1, 3, (H,), generator=g, device=dev()).float()
    shift = torch.randint(-3, 3, (H,), generator=g, device=dev()).float() + 0.5
    for mark in dict.fromkeys(mark_rows(rows, H)):
        keep = x[mark].clone(), y[mark].clone(), dy[mark].clone()
        x[mark], y[mark], dy[mark] = MARK, ag.BACKWARD_MAX + 1.0, MARK
        xl, yl, cl = x.long(), y.long(), c.long()
        _assert_sums(ops.colsum2(x), (xl.sum(0), (xl * xl).sum(0)), max(xl.abs().sum(0).max(), (xl * xl).sum(0).max()), rows, mark, "colsum2(x)")
        _assert_sums(ops.colsum2(x, y), (xl.sum(0), (xl * yl).sum(0)), max(xl.abs().sum(0).max(), (xl * yl).abs().sum(0).max()), rows, mark, "colsum2(x, y)")
        xc = xl - cl
        _assert_sums(ops.colsum2(x, center=c), (xc.sum(0), (xc * xc).sum(0)), ((xl.abs() + cl.abs()) ** 2).sum(0).max(), rows, mark, "colsum2(x, center)")
        # bn_bwd_stats: x plays xe (its MARK row passes the relu mask: 1000 scale + shift > 0), dy carries the mark
        m = (2 * xl * scale.long() + (2 * shift).long() > 0).long()
        gm = dy.long() * m
        _assert_sums(ops.bn_bwd_stats(dy, x, scale, shift, mean), (gm.sum(0), (gm * (xl - mean.long())).sum(0)),
                     max(gm.abs().sum(0).max(), (gm.abs() * (xl.abs() + mean.long().abs())).sum(0).max()), rows, mark, "bn_bwd_stats")
        assert bool(m[mark].all())
        x[mark], y[mark], dy[mark] = keep


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("H", EDGE_WIDTHS)
def test_edge_pass_statistics_are_the_int64_column_sums(H, case):
    """agg_edge_bwd_stats walks the edges as the column sums walk rows.  The halves recipe - premise, asserted first: the device sigmoid of
    GATE_HALF = 0 is exactly 0.5 - over random edges on NODES nodes: de' per row, s1 and s2 bit for bit."""
    one = ops.GraphViews(torch.zeros(1, dtype=torch.int32, device=dev()), torch.ones(1, dtype=torch.int32, device=dev()), 2)
    ones = torch.ones(2, H, device=dev())
    half = ops.node_aggregate_raw(torch.full((1, H), ag.GATE_HALF, device=dev()), None, ones, ones, one, 2, 2)[0][1].cpu()
    assert torch.equal(half, torch.full((H,), 0.5)), ("sigmoid(GATE_HALF) is not exactly 0.5", half)
    E = CASES[case][0](1024 // H)
    t = {k: v.to(dev()) for k, v in ag.exact_backward_inputs(E, NODES, H, seed=E + H).items()}
    g = torch.Generator().manual_seed(E)
    s, d = (torch.randint(0, NODES, (E,), generator=g).to(dev()) for _ in range(2))
    views = types.SimpleNamespace(srt_src=s.int(), srt_dst=d.int())            # (the edge pass reads the two endpoint arrays, in any order)
    for mark in dict.fromkeys(mark_rows(E, H)):
        keep = t["de0"][mark].clone(), t["xe"][mark].clone()
        t["de0"][mark], t["xe"][mark] = MARK, float(ag.BACKWARD_MAX)                # (xe = 2: 2 scale + shift > 0, the row is in the statistics)
        bound = ag.exact_backward_bound(s, d, t, NODES)
        assert max(bound["de"], bound["s1"], bound["s2"]) < ag.EXACT_LIMIT, bound
        want = ag.exact_backward(s, d, t, NODES)
        for x16 in (False, True):
            xe = t["xe"].to(torch.bfloat16) if x16 else t["xe"]
            de, s1, s2 = ops.agg_edge_bwd_stats(t["gates"], t["Tf"], t["Uf"], t["Tb"], t["Ub"], t["A2"], t["A3"], views, t["de0"].clone(), xe,
                                                t["scale"], t["shift"], t["mean"])
            bad = torch.nonzero((de != want["de"].float()).any(1)).flatten()
            assert bad.numel() == 0, (f"bf16 xe: {x16}", f"{bad.numel()} de' rows differ, first row {int(bad[0])} of {E}")
            for k, got, w in (("s1", s1, want["s1"]), ("s2", s2, want["s2"])):
                assert torch.equal(got, w.float()), (f"bf16 xe: {x16}", k, _explain(got, w.float(), E, mark))
        t["de0"][mark], t["xe"][mark] = keep
