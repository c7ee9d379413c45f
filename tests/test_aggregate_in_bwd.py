"""gnnome_node_aggregate_in_raw_f32 and gnnome_node_aggregate_in_bwd_f32 (csrc/node_aggregate_in_bwd.hip), the kernels alone.

The statement, in float64, with s_p = sigmoid(e[p]) over the destination-sorted edges p = (src_p -> dst_p):
    den[i]  = sum_{p: dst_p = i} s_p + 1e-6          fwd[i] = sum_{p: dst_p = i} s_p A2h[src_p] / den[i]
    raw:  aux0 = fwd,  aux1 = 1 / den,  v = A1h + fwd
    bwd:  de[p] += s_p (1 - s_p) (Tf[dst_p] A2h[src_p] - Uf[dst_p]),     dA2h[j] = sum_{p: src_p = j} s_p Tf[dst_p]
THE BAR IS MEASURED, not fixed: the entries the symmetric step uses for the same quantities run on the same inputs -
gnnome_node_aggregate_raw_f32 mode 1 with a zero A3h table (v, aux0, aux1), mode 2 with A3h := Tf (dA2h = its aux2) and
gnnome_agg_edge_bwd_f32 with zero Tb / Ub / A3h (de) - and the new kernel's largest error against the statement may be at most TWICE
theirs (only association and contraction differ: the margin of test_aggregate_in.py's hub test).  Graphs: tests/gated_graphs.py.

Measured on an MI355X (max-abs error against the statement, new / existing entry; `=` where the two outputs agree bit for bit):
see DESIGN.md section 7b."""
import pytest
import torch

import gnnome_amd  # noqa: F401
from gnnome_amd import ops

import gated_graphs as gg

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256)
_CASES = {}


def dev():
    return torch.device("cuda", 0)


def _views(src, dst, n):
    return ops.GraphViews(torch.as_tensor(src, dtype=torch.int32).to(dev()), torch.as_tensor(dst, dtype=torch.int32).to(dev()), n)


def _inputs(views, hidden, ld_blocks, seed):
    """e[E,H] per sorted position, P[N, ld_blocks * H] = A1h | A2h | zeros | ..., Tf, Uf [N,H], a random starting de."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    n = views.num_nodes
    e = (2.0 * rnd(views.num_edges, hidden)).to(dev())
    P = rnd(n, ld_blocks * hidden)
    P[:, 2 * hidden:3 * hidden] = 0.0          # the A3h block of the symmetric entries: all zero
    Tf, Uf, de0 = rnd(n, hidden).to(dev()), rnd(n, hidden).to(dev()), rnd(views.num_edges, hidden).to(dev())
    return dict(e=e, P=P.to(dev()), Tf=Tf, Uf=Uf, de0=de0, H=hidden, views=views)


def _graphs(hidden):
    """name -> (src, dst, n): the degree graph (in-lists of 0, 1, 2, G-1, G, G+1, 63, 64, 65, 129 items, parallel edges, self-loops), the
    same graph with src and dst swapped (the OUT-lists take those lengths), and a single node with three self-loops."""
    gr = gg.degree_graph(hidden)
    return {"degree": (gr["src"], gr["dst"], gr["n"]), "swapped": (gr["dst"], gr["src"], gr["n"]), "one_node": ([0, 0, 0], [0, 0, 0], 1)}


def _case(hidden, name, ld_blocks=5):
    """One graph of one width with its inputs, the statement and the existing entries' outputs: built once, shared, read-only."""
    key = (hidden, name, ld_blocks)
    if key not in _CASES:
        if name == "hub" or name == "hub_swapped":
            gr = gg.hub_graph()
            src, dst, n = (gr["src"], gr["dst"], gr["n"]) if name == "hub" else (gr["dst"], gr["src"], gr["n"])
        else:
            src, dst, n = _graphs(hidden)[name]
        c = _inputs(_views(src, dst, n), hidden, ld_blocks, seed=hidden + len(name) + ld_blocks)
        c["want"] = _statement(c)
        c["old"] = _existing(c) if ld_blocks == 5 else None
        _CASES[key] = c
    return _CASES[key]


def _blocks(c):
    H = c["H"]
    return c["P"][:, :H], c["P"][:, H:2 * H], c["P"][:, 2 * H:3 * H]


def _statement(c):
    """float64, on the device: dict(v, aux0, aux1, dA2h, inc) - inc = the de increment."""
    views, H = c["views"], c["H"]
    s, d = views.srt_src.long(), views.srt_dst.long()
    A1, A2, _ = (t.double() for t in _blocks(c))
    sig = torch.sigmoid(c["e"].double())
    zeros = torch.zeros((views.num_nodes, H), dtype=torch.float64, device=dev())
    den = zeros.index_add(0, d, sig) + 1e-6
    fwd = zeros.index_add(0, d, sig * A2[s]) / den
    Tf, Uf = c["Tf"].double(), c["Uf"].double()
    return dict(v=A1 + fwd, aux0=fwd, aux1=1.0 / den, dA2h=zeros.index_add(0, s, sig * Tf[d]),
                inc=sig * (1.0 - sig) * (Tf[d] * A2[s] - Uf[d]))


def _existing(c):
    """The symmetric step's entries on the same inputs (ld_node = 5H: their projection's)."""
    views, n = c["views"], c["views"].num_nodes
    A1, A2, Z = _blocks(c)
    v, a0, a1, _, _ = ops.node_aggregate_raw(c["e"], A1, A2, Z, views, 1, n)
    zero = torch.zeros_like(c["Tf"])
    _, dA2h = ops.node_aggregate_raw(c["e"], None, zero, c["Tf"], views, 2, n)          # aux2 = sum_out s * A3h[dst] with A3h := Tf
    inc = ops.agg_edge_bwd(c["e"], c["Tf"], c["Uf"], zero, zero, A2, Z, views, torch.zeros_like(c["e"]))
    de = ops.agg_edge_bwd(c["e"], c["Tf"], c["Uf"], zero, zero, A2, Z, views, c["de0"].clone())
    return dict(v=v, aux0=a0, aux1=a1, dA2h=dA2h, inc=inc, de=de)


def _new(c):
    A1, A2, _ = _blocks(c)
    v, a0, a1 = ops.node_aggregate_in_raw(c["e"], A1, A2, c["views"])
    inc = torch.zeros_like(c["e"])
    dA2h = ops.node_aggregate_in_bwd(c["e"], c["Tf"], c["Uf"], A2, c["views"], inc)
    de = c["de0"].clone()
    ops.node_aggregate_in_bwd(c["e"], c["Tf"], c["Uf"], A2, c["views"], de)
    torch.cuda.synchronize()
    return dict(v=v, aux0=a0, aux1=a1, dA2h=dA2h, inc=inc, de=de)


def _err(got, want):
    return (got.double() - want).abs().max().item() if want.numel() else 0.0


def _within_twice_the_existing_entries(c, label):
    new, old, want = _new(c), c["old"], dict(c["want"])
    want["de"] = c["de0"].double() + want["inc"]
    for k in ("v", "aux0", "aux1", "dA2h", "inc", "de"):
        assert torch.isfinite(new[k]).all(), k
        e_new, e_old = _err(new[k], want[k]), _err(old[k], want[k])
        print(f"{label} {k}: max-abs error new {e_new:.3e}, existing entry {e_old:.3e}{' (equal bit for bit)' if torch.equal(new[k], old[k]) else ''}")
        assert e_new <= 2.0 * e_old, (k, e_new, e_old)
    return new


@pytest.mark.parametrize("name", ("degree", "swapped", "one_node"))
@pytest.mark.parametrize("hidden", WIDTHS)
def test_degree_cases_within_twice_the_existing_entries_error(hidden, name):
    c = _case(hidden, name)
    views = c["views"]
    if name != "one_node":
        ptr = views.in_ptr if name == "degree" else views.out_ptr
        assert set(gg.in_degrees(hidden)) <= set((ptr[1:] - ptr[:-1]).tolist())          # the list lengths the kernel's paths turn on
    _within_twice_the_existing_entries(c, f"H={hidden} {name}")


@pytest.mark.parametrize("hidden", WIDTHS)
def test_a_4h_projection_gives_the_5h_projections_bits(hidden):
    """ld_node = 4H (this model's projection) against 5H (the symmetric one's), the same columns: the stride is an address, not a value."""
    c5 = _case(hidden, "degree")
    P4 = c5["P"][:, :4 * hidden].contiguous()
    c4 = dict(c5, P=P4)
    assert P4.stride(0) == 4 * hidden and c5["P"].stride(0) == 5 * hidden
    a, b = _new(c4), _new(c5)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("hidden", WIDTHS)
def test_exact_statements(hidden):
    c = _case(hidden, "degree")
    views, (A1, A2, _) = c["views"], _blocks(c)
    first, again = _new(c), _new(c)
    assert all(torch.equal(first[k], again[k]) for k in first)          # two runs leave equal bits
    no_out = (views.out_ptr[1:] == views.out_ptr[:-1])
    assert bool(no_out.any()) and not bool(first["dA2h"][no_out].any())          # a node without out-edges: an all-zero dA2h row
    # Tf = Uf = 0: de keeps its input, dA2h is zero
    zero = torch.zeros_like(c["Tf"])
    de = c["de0"].clone()
    dA = ops.node_aggregate_in_bwd(c["e"], zero, zero, A2, views, de)
    assert torch.equal(de, c["de0"]) and not bool(dA.any())
    # doubling Tf and Uf doubles dA2h and the de increment exactly
    inc2 = torch.zeros_like(c["e"])
    dA2 = ops.node_aggregate_in_bwd(c["e"], 2.0 * c["Tf"], 2.0 * c["Uf"], A2, views, inc2)
    assert torch.equal(dA2, 2.0 * first["dA2h"]) and torch.equal(inc2, 2.0 * first["inc"])


@pytest.mark.parametrize("hidden", WIDTHS)
def test_no_edges(hidden):
    """E = 0: dA2h all zero, de untouched (it has no rows); raw leaves v = A1h, fwd = 0, aux1 = 1 / 1e-6."""
    for n in (1, 5):
        views = _views([], [], n)
        c = _inputs(views, hidden, 4, seed=n)
        A1, A2, _ = _blocks(c)
        out = torch.full((n, hidden), 7.0, device=dev())
        de = torch.empty((0, hidden), device=dev())
        got = ops.node_aggregate_in_bwd(c["e"], c["Tf"], c["Uf"], A2, views, de, out=out)
        assert got is out and not bool(out.any()) and de.shape == (0, hidden)
        v, a0, a1 = ops.node_aggregate_in_raw(c["e"], A1, A2, views)
        assert torch.equal(v, A1.contiguous()) and not bool(a0.any())
        assert (a1.double() * 1e-6 - 1.0).abs().max().item() < 1e-6          # 1 / float32(1e-6), one rounding of the quotient


@pytest.mark.parametrize("name", ("hub", "hub_swapped"))
def test_one_hub_of_5000_edges(name):
    """gg.hub_graph(): one node with 5000 in-edges (raw, de: one wave streams them; the sums in 128-item blocks) and its swap, one node with
    5000 out-edges (dA2h in 128-item blocks).  H = 128, the same measured bar."""
    c = _case(128, name)
    views = c["views"]
    ptr = views.in_ptr if name == "hub" else views.out_ptr
    assert int((ptr[1:] - ptr[:-1]).max()) == 5000
    first = _within_twice_the_existing_entries(c, f"H=128 {name}")
    again = _new(c)
    assert all(torch.equal(first[k], again[k]) for k in first)
