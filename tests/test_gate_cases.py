"""The gate cases of tests/gate_cases.py on the CPU: their fp64 statement is an fp32 value inside the bounds the exactness argument needs,
and every mutant of the statement differs from it on the case the table names."""
import pytest
import torch

import gate_cases as gc

SMALL_COUNTS = {T: gc.edge_counts(T, 8) for T in (32, 64, 128)}     # 8 tiles per round: the same edges, cheap on the CPU


def _is_fp32(t):
    return torch.equal(t.float().double(), t)


@pytest.mark.parametrize("H,T", [(64, 64), (128, 32), (256, 32), (128, 128)])
@pytest.mark.parametrize("kind", gc.GRAPHS)
def test_wide_cases_are_exact_and_bounded(H, T, kind):
    for E in SMALL_COUNTS[T]:
        c = gc.Case(H, E, kind, T, 8)
        assert c.e.abs().max() <= 8 and _is_fp32(c.e.double()) and set(c.W3.unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert (c.W3 != 0).sum(1).max() <= 3 and not torch.equal(c.W3, c.W3.t()) and (c.W3.abs().sum(0) != 1).any()
        assert (c.e.abs().max() * (c.W3 != 0).sum(1).max()) < 2 ** 11               # every partial sum of the product
        x = c.x64(E)
        assert torch.equal(x, x.round()) and x.abs().max() < 2 ** 22, c.name
        z = x * c.scale.double() + c.shift.double()
        assert torch.equal(2 * z, (2 * z).round()) and z.abs().max() < 2 ** 23 and torch.equal(c.shift, c.shift.round())
        y = gc.statement(c)
        assert _is_fp32(y) and _is_fp32(z) and y.abs().max() < 2 ** 23 and (y != gc.SENTINEL).all(), c.name
        if E >= T and kind != "n1":     # both sides of the relu, and its zero
            assert 0.25 < (z > 0).double().mean() < 0.75 and (z == 0).any(), c.name
        e0 = gc.encoded64(c)
        assert torch.equal(e0, e0.round()) and e0.abs().max() <= 64 and _is_fp32(gc.encode_statement(c)), c.name


def test_the_straddling_runs_sit_on_the_boundaries():
    T, R = 32, 8
    c = gc.Case(128, 4 * R * T + 1, "straddle", T, R)
    d = c.views.srt_dst
    for edge in (T, R * T):
        assert d[edge - 1] == d[edge] and d[edge - 3] == d[edge + 4]
    assert not torch.equal(c.views.srt_eid, torch.arange(c.E, dtype=torch.int32))    # the sort is a real permutation
    dup = gc.Case(64, 65, "dups", 64, 8)
    raw = gc.raw_features(65)[dup.views.srt_eid.long()]
    same = (dup.views.srt_src[1:] == dup.views.srt_src[:-1]) & (dup.views.srt_dst[1:] == dup.views.srt_dst[:-1])
    assert same.any() and (raw[1:][same] != raw[:-1][same]).any(1).all()              # copies of one edge carry different raw features


@pytest.mark.parametrize("H", [64, 128, 256])
def test_small_recipe_rounds_in_bf16_with_ties(H):
    c = gc.Case(H, 4 * 32 + 1, "uniform", 32, 8, "small")
    x = c.x64(c.E)
    assert x.abs().min() >= 257 and x.abs().max() <= 1023 and (x % 2 == 1).double().mean() > 0.25
    r = gc.to_bf16_nearest_even(x).double()
    assert (r != x).double().mean() > 0.25
    ties = ((x < 512) & (x % 2 == 1)) | ((x >= 512) & (x % 4 == 2))
    assert ties.any() and (r[ties] > x[ties]).any() and (r[ties] < x[ties]).any()     # ties go both ways: to even, not up or down
    c.shift = c.shift * 0 - 600
    y = gc.statement(c, x=r)      # e' from the rounded rows
    assert _is_fp32(y)


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("recipe,E", [("flat", 1), ("flat", 31), ("flat", 129), ("flat", 8193), ("flat", 16385), ("outlier", 4000)])
def test_statistics_recipes_keep_every_sum_below_2_24(H, recipe, E):
    c = gc.Case(H, E, "uniform", 32, 256, recipe)
    for x in (c.x64(E), gc.to_bf16_nearest_even(c.x64(E)).double()):
        d = x - x[0]
        assert torch.equal(d, d.round()) and d.abs().sum(0).max() < 2 ** 24 and (d * d).sum(0).max() < 2 ** 24
    if recipe == "outlier":
        assert (c.views.srt_src == 0).nonzero().flatten().tolist() == [0]
        assert d[1:].min() >= 52 and (d * d).sum(0).max() > 2 ** 23     # large, but still exact


def test_route_table_covers_the_dispatch():
    seen = {gc.gate_kernel(H, k, oop) for _, H, k, _, oop in gc.GATE_ROUTES}
    assert seen == {"bf", "pl", "ws", "tile", "f16", "stream"}
    assert gc.gate_kernel(128, 0, True, aligned=False) == "tile" and gc.gate_kernel(256, 0, True, aligned=False) == "stream"
    assert gc.gate_kernel(128, 0, True, affine=False) == "tile" and gc.gate_kernel(256, 0, False) == "tile"
    assert gc.persistent_grid(256) == 256 and gc.persistent_grid(304) == 256 and gc.persistent_grid(36) == 32
    assert gc.tiles_per_round("f16", 256) == 128 and gc.tiles_per_round("f16", 40) == 16
    assert gc.ref_geometry(256, 1, 256) == ("refm", 32, 1024) and gc.ref_geometry(128, 0, 256)[1] == 64 and gc.ref_geometry(64, 1, 256)[0] == "scalar"


@pytest.mark.parametrize("name", list(gc.MUTANTS))
def test_every_mutant_is_caught_by_its_case(name):
    states, mutant, (H, E, kind, T, R, recipe) = gc.MUTANTS[name]
    c = gc.Case(H, E, kind, T, R, recipe)
    want, got = states(c), mutant(c)
    assert _is_fp32(want) or states is gc.stats_statement
    assert want.shape == got.shape and not torch.equal(want, got), f"{name}: not seen on {c.name}"
    # the case is one the device tests run: its graph, its recipe and, for the route it names, its edge count
    assert kind in gc.GRAPHS and E in gc.edge_counts(T, R) + [4000]
