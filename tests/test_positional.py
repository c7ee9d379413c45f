"""gnnome_amd.positional (csrc/positional.hip) against tests/positional_statement.py, the dense fp64 restatement of
utils/data_utils.py:59-90 that tests/test_positional_statement.py pins on hand-computed cases.

Tolerance.  Every entry of either encoding is a sum of non-negative terms: no cancellation.  Compared in fp64, the relative error
of either side is bounded by (operations on the longest dependency chain) x 2^-53, and a step puts at most (largest in-degree)
additions and two multiplications on a chain.  rtol = 1e-12 covers 9000 such operations; every case asserts that the device's chain
and the statement's together stay below that (check()), exact zeros must be exact zeros, and the float32 output must be the one
cast of the float64 table, bit for bit."""
import functools

import pytest
import torch

import positional_statement as st
from gnnome_amd import ops, positional

gpu = pytest.mark.gpu
RTOL = 1e-12


def dev():
    return torch.device("cuda", 0)


def on_device(graph):
    src, dst, n = graph
    return (torch.tensor(src, dtype=torch.int32, device=dev()), torch.tensor(dst, dtype=torch.int32, device=dev()), n)


@functools.lru_cache(maxsize=None)
def case(name, *args):
    """(graph, statement RW / PR callables with their results cached) - the references are computed once and shared."""
    return getattr(st, name)(*args)


@functools.lru_cache(maxsize=None)
def want(kind, pe_dim, name, *args):
    src, dst, n = case(name, *args)
    return (st.rw if kind == "RW" else st.pr)(src, dst, n, pe_dim)


def check(kind, pe_dim, name, *args, capacity=None):
    graph = case(name, *args)
    ref = want(kind, pe_dim, name, *args)
    chain = st.longest_chain(*graph, pe_dim)
    print(f"{kind} {name}{args} pe_dim={pe_dim}: chain {chain} operations, bound {2 * chain * 2.0 ** -53:.3e}")
    assert 2 * chain * 2.0 ** -53 <= RTOL                     # the device's chain and the statement's
    g = on_device(graph)
    got64 = positional.positional_encoding(g, pe_dim, kind, dtype=torch.float64, capacity=capacity)
    assert got64.shape == (graph[2], pe_dim) and got64.dtype == torch.float64 and got64.is_cuda
    got = got64.cpu()
    err = ((got - ref).abs() / ref.abs().clamp(min=1e-300)).max().item() if ref.numel() else 0.0
    print(f"    largest relative error {err:.3e}")
    assert torch.equal(got == 0, ref == 0)                    # exact zeros are exact zeros
    torch.testing.assert_close(got, ref, rtol=RTOL, atol=0)
    got32 = positional.positional_encoding(g, pe_dim, kind, capacity=capacity)
    assert got32.dtype == torch.float32 and torch.equal(got32, got64.float())
    again = positional.positional_encoding(g, pe_dim, kind, dtype=torch.float64, capacity=capacity)
    assert torch.equal(again, got64)                          # two launches, the same bits
    return got64


# ---- PageRank ------------------------------------------------------------------------------------------------------------------------

PR_CASES = [("single_node",), ("one_edge",), ("source_and_sink",), ("parallel_two_cycle",), ("self_loop_in_degree_two",), ("mixed_small",),
            ("four_nodes",), ("wide_in_lists",), ("random_graph", 257, 1500, 3), ("banded",)]


@gpu
@pytest.mark.parametrize("pe_dim", [1, 20])
@pytest.mark.parametrize("which", range(len(PR_CASES)))
def test_pagerank_equals_the_statement(which, pe_dim):
    check("PR", pe_dim, *PR_CASES[which])


@gpu
def test_pagerank_wide_lists_cross_the_wavefront_once_and_twice():
    src, dst, n = case("wide_in_lists")
    in_deg, _ = st.degrees(src, dst, n)
    assert in_deg[0].item() == 65 and in_deg[1].item() == 130
    check("PR", 3, "wide_in_lists")


@gpu
def test_pagerank_on_reversed_views_is_the_reversed_graph():
    src, dst, n = case("mixed_small")
    s, d, _ = on_device((src, dst, n))
    got = positional.positional_encoding(ops.GraphViews(s, d, n).reversed(), 6, "PR", dtype=torch.float64).cpu()
    ref = st.pr(dst, src, n, 6)
    assert torch.equal(got == 0, ref == 0)
    torch.testing.assert_close(got, ref, rtol=RTOL, atol=0)


# ---- random-walk return ----------------------------------------------------------------------------------------------------------------

RW_CASES = [("triangle",), ("two_cycle",), ("self_loop_in_degree_two",), ("one_edge",), ("dag",), ("parallel_two_cycle",), ("four_nodes",),
            ("mixed_small",), ("hub_three_cycle",), ("random_graph", 40, 70, 9), ("single_node",)]


@gpu
@pytest.mark.parametrize("pe_dim", [1, 20])
@pytest.mark.parametrize("which", range(len(RW_CASES)))
def test_rw_return_equals_the_statement(which, pe_dim):
    check("RW", pe_dim, *RW_CASES[which])


@gpu
def test_rw_hand_cases_are_exact():
    pe = lambda name, k: positional.positional_encoding(on_device(case(name)), k, "RW", dtype=torch.float64).tolist()  # noqa: E731
    assert pe("triangle", 3) == [[0.0, 0.0, 1.0]] * 3
    assert pe("two_cycle", 4) == [[0.0, 1.0, 0.0, 1.0]] * 2
    assert pe("self_loop_in_degree_two", 1) == [[0.5], [0.0]]
    assert pe("parallel_two_cycle", 4) == [[0.0, 1.0, 0.0, 1.0]] * 2
    assert pe("dag", 6) == [[0.0] * 6] * 5
    assert pe("one_edge", 2) == [[0.0, 0.0]] * 2                 # in-degree 0: 1 / max(0, 1)


@gpu
def test_rw_hub_merges_a_run_of_seventy():
    src, dst, n = case("hub_three_cycle")
    assert st.degrees(src, dst, n)[0][0].item() == 70
    got = check("RW", 6, "hub_three_cycle").cpu()
    assert got[0, 2].item() > 0 and got[0, 0].item() == 0 and got[0, 1].item() == 0


@gpu
def test_rw_banded_graph_at_the_default_capacity():
    src, dst, n = case("banded")
    sizes = st.rw_expansion_sizes(src, dst, n, 8)
    assert max(max(r) for r in sizes) <= ops.RW_DEFAULT_CAPACITY
    check("RW", 8, "banded")
    s, d, _ = on_device((src, dst, n))
    _, info = ops.rw_return(ops.GraphViews(s, d, n), 8, torch.float64, return_info=True)
    assert info[:, 0].tolist() == [max(r) for r in sizes]


def _first_overflow(sizes, capacity):
    for node, row in enumerate(sizes):
        for t in row:
            if t > capacity:
                return node, t
    return None


@gpu
@pytest.mark.parametrize("name,args,pe_dim", [("hub_three_cycle", (), 6), ("random_graph", (40, 70, 9), 7), ("banded", (), 6)])
def test_rw_capacity_exactly_reached_passes_and_one_less_raises(name, args, pe_dim):
    src, dst, n = case(name, *args)
    sizes = st.rw_expansion_sizes(src, dst, n, pe_dim)
    need = max(max(r) for r in sizes)
    check("RW", pe_dim, name, *args, capacity=need)                      # a row reaches exactly the capacity
    capacity = need - 1                                                  # the same row now needs capacity + 1
    node, needed = _first_overflow(sizes, capacity)
    assert needed == capacity + 1
    s, d, _ = on_device((src, dst, n))
    views = ops.GraphViews(s, d, n)
    for dtype in (torch.float64, torch.float32):
        out = torch.full((n, pe_dim), -7.0, dtype=dtype, device=dev())
        with pytest.raises(RuntimeError, match=rf"node {node} needs at least {needed} .*capacity={capacity}.*capacity=") as exc:
            ops.rw_return(views, pe_dim, dtype, capacity=capacity, out=out)
        assert "capacity=" in str(exc.value)
        assert (out == -7.0).all()                                       # the output buffer is untouched
    with pytest.raises(RuntimeError, match="capacity="):
        positional.positional_encoding((s, d, n), pe_dim, "RW", capacity=capacity)
    torch.cuda.synchronize()
    check("RW", pe_dim, name, *args)                                     # and the default capacity still works afterwards


@gpu
def test_rw_capacity_beyond_the_lds_budget_is_refused():
    s, d, n = on_device(case("triangle"))
    assert ops.rw_return_lds_bytes(ops.RW_DEFAULT_CAPACITY) == 32 * 1024 + 4
    with pytest.raises(RuntimeError, match="LDS"):
        ops.rw_return(ops.GraphViews(s, d, n), 2, capacity=4097)


@gpu
def test_rw_wide_capacity_runs_four_wavefronts_with_the_same_bits():
    # above 1024 a node is owned by a workgroup of four wavefronts: the same order of every sum, the same bits
    g = on_device(case("banded"))
    a = positional.positional_encoding(g, 8, "RW", dtype=torch.float64)
    b = positional.positional_encoding(g, 8, "RW", dtype=torch.float64, capacity=2048)
    c = positional.positional_encoding(g, 8, "RW", dtype=torch.float64, capacity=4096)
    assert torch.equal(a, b) and torch.equal(a, c)


@gpu
def test_rw_on_reversed_views_is_the_reversed_graph():
    src, dst, n = case("mixed_small")
    s, d, _ = on_device((src, dst, n))
    got = positional.positional_encoding(ops.GraphViews(s, d, n).reversed(), 6, "RW", dtype=torch.float64).cpu()
    ref = st.rw(dst, src, n, 6)
    assert torch.equal(got == 0, ref == 0)
    torch.testing.assert_close(got, ref, rtol=RTOL, atol=0)


# ---- the reference's call --------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("kind", ["RW", "PR"])
def test_add_positional_encoding_on_a_graph_dict(kind):
    src, dst, n = case("banded")
    s, d, _ = on_device((src, dst, n))
    g = {"src": s, "dst": d, "num_nodes": n, "y": torch.zeros(len(src))}
    out = positional.add_positional_encoding(g, 5, kind)
    assert out is g and set(g) == {"src", "dst", "num_nodes", "y", "in_deg", "out_deg", "pe"}
    ind, outd = st.degrees(src, dst, n)
    assert g["in_deg"].dtype == g["out_deg"].dtype == torch.float32 and g["in_deg"].shape == g["out_deg"].shape == (n,)
    assert torch.equal(g["in_deg"].cpu(), ind.float()) and torch.equal(g["out_deg"].cpu(), outd.float())
    assert g["pe"].shape == (n, 5) and g["pe"].dtype == torch.float32 and g["pe"].is_cuda
    torch.testing.assert_close(g["pe"].cpu().double(), want(kind, 5, "banded"), rtol=2.0 ** -23, atol=0)
    host = {"src": torch.tensor(src), "dst": torch.tensor(dst), "num_nodes": n}
    assert set(positional.add_positional_encoding(host, device=dev())) == {"src", "dst", "num_nodes", "in_deg", "out_deg"}
    assert set(positional.add_positional_encoding(dict(host), 3, "none", device=dev())) == {"src", "dst", "num_nodes", "in_deg", "out_deg"}
