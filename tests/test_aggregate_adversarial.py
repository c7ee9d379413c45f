"""The gated aggregation (gnnome_amd/csrc/node_aggregate.hip) on the graphs of tests/aggregate_graphs.py: every list length around the
kernels' step sizes, hubs at and around the split threshold, more hubs than the hub list holds.

EXACT checks: gate inputs of GATE_ON / GATE_OFF make the device sigmoid exactly 1 or exactly 0, table rows are small integers - every
gated sum is an integer below 2^24 with the same fp32 bits in any order, so a lost, doubled or misrouted list item shows as an integer
difference at any list length (a hub of 10^4 items hides one item inside every rounding bar).  The first assertions of each exact test
are the premise: one-item probe nodes must give exactly 1.0 and exactly 0.0.

The HALVES recipe (test_exact_backward and the tests after it) extends this to the aggregation's BACKWARD, whose gradient term carries
s (1 - s) and vanishes at both of those gates: a third gate value, GATE_HALF = 0, whose device sigmoid is exactly 0.5 (the premise those
tests open with: a one-item probe gives 0.5), small integer tables, de0, xe and mean, scale in {1, 2}, shift an odd multiple of 0.5.  Then
both node sums, de' per sorted position and the BatchNorm statistics s1, s2 are multiples of 1/4 whose sums of |terms| stay below 2^24
quarters (asserted on the CPU in tests/test_aggregate_graphs.py and again for the inputs of each device test): ONE fp32 bit pattern, in any
order of the additions and with or without fma contraction, for agg_bwd_fused (all five outputs, fp32 and bf16 xe, the amax slot), for
agg_edge_bwd_stats / agg_edge_bwd, for the variants behind set_tuning(4, 88 / 77) and for node_aggregate_in_bwd - on the list lengths,
the hubs, and ag.TAILS (trailing nodes without edges: the clamp of the indices requested ahead).

REAL-VALUED checks: inputs drawn as in test_hip_parity.test_node_aggregate, against the checker (tests/cpu_ops.py) in float64 at that
file's bar (_assert_close: 1e-5 max(scale, 1)), plus the bit-level promises: two runs, num_nodes_out, node ranges, the single-wave
path, the tuning variants documented as "the same bits".

HUB-LIST DETERMINISM: with more than HUB_CAP hubs the split ones are the HUB_CAP lowest node ids, on every rebuild of the views.

Every graph runs as plain views, as .reversed() views (the caller swaps the roles of the tables, as engine.layer_step does) and over
renumbered nodes (node_perm); the references are stated on the views' own sorted arrays."""
import pytest
import torch

import aggregate_graphs as ag
import cpu_ops
from gnnome_amd import ops
from test_hip_parity import _assert_close

pytestmark = pytest.mark.gpu

FORMS = ("plain", "reversed", "perm")
SMALL = [(name, h) for name in ("lists", "hub_edges") for h in (64, 128, 256)]
MANY = [(f"many_hubs{k}", h) for k in ag.MANY_HUBS for h in (64, 128)]      # (e stays near 150 MB)


def dev():
    return torch.device("cuda", 0)


class _Form:
    """One graph in one of the three forms: the device views, the sorted endpoint arrays IN THE ROLES THE FORM GIVES THEM (s, d: for
    reversed views the stored arrays swapped), internal node ids, and the role swaps a caller of transposed views makes."""

    def __init__(self, name, form):
        g = ag.graph(name) if isinstance(name, str) else name      # (a graph of its own, as ag.tails() makes them: plain form, no probes)
        self.g, self.n, self.form = g, g["n"], form
        src, dst = g["src"].to(dev()), g["dst"].to(dev())
        perm = None
        if form == "perm":
            perm = torch.randperm(self.n, generator=torch.Generator().manual_seed(len(name)))       # (named graphs only)
        self.build = lambda: (ops.GraphViews(src, dst, self.n, node_perm=perm).reversed() if form == "reversed"
                              else ops.GraphViews(src, dst, self.n, node_perm=perm))
        self.views = self.build()
        self.t = self.views.transposed
        ss, sd = self.views.srt_src.cpu().long(), self.views.srt_dst.cpu().long()
        self.s, self.d = (sd, ss) if self.t else (ss, sd)
        self.gcv = type("Sorted", (), {"srt_src": self.s.to(dev()), "srt_dst": self.d.to(dev())})()   # what the checker reads of a views object
        self.inner = (lambda v: int(perm[v])) if perm is not None else int
        self.hubs = sorted(self.inner(h) for h in g["hubs"])
        self.e = ss.numel()
        self.pos_on = self.pos_off = self.probe_src = self.probe_on = self.probe_off = None
        if g["probe_on"] is not None:
            in_ptr = self.views.in_ptr.cpu()
            self.pos_on, self.pos_off = int(in_ptr[self.inner(g["probe_on"])]), int(in_ptr[self.inner(g["probe_off"])])
            self.probe_src, self.probe_on, self.probe_off = (self.inner(g[k]) for k in ("probe_src", "probe_on", "probe_off"))

    def swap(self, a, b):
        return (b, a) if self.t else (a, b)

    def aggregate(self, e, A1, A2, A3, h, norm, scale, shift, **kw):
        return ops.node_aggregate(e, A1, *self.swap(A2, A3), self.views, h, norm, scale, shift, **kw)

    def raw2(self, e, A2, A3):
        return self.swap(*ops.node_aggregate_raw(e, None, *self.swap(A2, A3), self.views, 2, self.n))

    def raw1(self, e, A1, A2, A3):
        v, f, rf, b, rb = ops.node_aggregate_raw(e, A1, *self.swap(A2, A3), self.views, 1, self.n)
        return (v,) + self.swap(f, b) + self.swap(rf, rb)      # (v, fwd, bwd, rdf, rdb)


def _exact_case(f, hidden, seed, off=ag.GATE_OFF):
    """The exact inputs with the probes wired in: probe_src's table rows are 1, the two probe edges are open / closed in every channel."""
    gates, A2, A3, X = ag.exact_inputs(f.e, f.n, hidden, seed)
    gates[f.pos_on], gates[f.pos_off] = ag.GATE_ON, off
    A2[f.probe_src], A3[f.probe_src] = 1.0, 1.0
    return gates, A2, A3, X


def _ulp_distance(got, want64):
    """|got - want| in units of the fp32 spacing at want."""
    w32 = want64.float()
    ulp = (torch.nextafter(w32.abs(), torch.full_like(w32, float("inf"))) - w32.abs()).double()
    return ((got.double() - want64).abs() / ulp).max().item()


@pytest.mark.parametrize("hidden", [128])
def test_a_gate_of_minus_64_is_not_exactly_closed(hidden):
    """Why the exact recipe closes its gates with GATE_OFF = -128 and not with -64, as a measurement that stays in the suite.  A gate
    input of +64 gives a device sigmoid of exactly 1.0.  One of -64 does NOT give 0.0: rcp(1 + exp(64)) = 1.603812263028016e-28 on the
    MI355X - exp(64) = 6.2e27 is an ordinary fp32 value, nothing overflows.  That is the arithmetic's right answer (exp(-64) =
    1.6038109e-28), so this test asserts it as such: positive, and within 1e-5 of exp(-64) - the product 64 log2(e) = 92.33 is rounded
    to fp32 before the exp2 (half a spacing of 7.6e-6: a factor 1 +- 2.6e-6 on the result), exp2 and rcp add about an ulp each.  A sum
    that ends at the integer 0 would keep such crumbs in an order-dependent amount; at -128 exp overflows, rcp(inf) = 0, and the probes
    at the head of every exact test hold."""
    import math
    f = _Form("lists", "plain")
    gates, A2, A3, _ = _exact_case(f, hidden, seed=1, off=-64.0)
    a0, _ = f.raw2(gates.to(dev()), A2.to(dev()), A3.to(dev()))
    on, off = a0[f.probe_on].cpu(), a0[f.probe_off].cpu()
    print(f"probe sums: gate +64 -> {on[0].item()!r}, gate -64 -> {off[0].item()!r}")
    assert torch.equal(on, torch.ones(hidden)), on
    assert bool((off > 0).all()) and (off.double() / math.exp(-64.0) - 1.0).abs().max().item() <= 1e-5, off[0].item()


@pytest.mark.parametrize("name,hidden", SMALL + MANY)
def test_exact_sums(name, hidden):
    for form in FORMS:
        f = _Form(name, form)
        gates, A2, A3, X = _exact_case(f, hidden, seed=hidden + len(name))
        to_f = lambda t: t.float()  # noqa: E731
        ge, gA2, gA3, gs, gd = gates.to(dev()), A2.to(dev()), A3.to(dev()), f.s.to(dev()), f.d.to(dev())
        want = ag.exact_sums(gs, gd, ge, gA2, gA3, f.n)      # int64 sums with torch on the device: the host takes a second per index_add at 300k rows
        # mode 2 - first the premise: the probes' one-item sums are exactly 1.0 (open gate) and exactly 0.0 (closed gate)
        a_in, a_out = f.raw2(ge, gA2, gA3)
        probed = a_out if f.t else a_in         # (the probes' stored in-edge is an out-edge in the roles of reversed views)
        assert torch.equal(probed[f.probe_on].cpu(), torch.ones(hidden)), (form, "sigmoid(GATE_ON) is not exactly 1.0", probed[f.probe_on])
        assert torch.equal(probed[f.probe_off].cpu(), torch.zeros(hidden)), (form, "sigmoid(GATE_OFF) is not exactly 0.0", probed[f.probe_off])
        assert torch.equal(a_in, to_f(want["sum_in"])), (form, _where(a_in, to_f(want["sum_in"])))
        assert torch.equal(a_out, to_f(want["sum_out"])), (form, _where(a_out, to_f(want["sum_out"])))
        # mode 1: the reciprocal denominators hold the integer gate counts
        gA1 = A2.flip(0).to(dev())
        _, _, _, rdf, rdb = f.raw1(ge, gA1, gA2, gA3)
        for got, cnt, what in ((rdf, want["cnt_in"], "rdf"), (rdb, want["cnt_out"], "rdb")):
            back = (1.0 / got.double() - 1e-6).round().long()
            assert torch.equal(back, cnt), (form, what, _where(back, cnt))
            assert _ulp_distance(got, 1.0 / (cnt.double() + 1e-6)) <= 2.0, (form, what)
        # the fused aggregation backward: its two node sums (table Tb at the source, Tf at the destination)
        g = torch.Generator().manual_seed(3)
        r = lambda *s: torch.randn(*s, generator=g).to(dev())  # noqa: E731
        Uf, Ub, de, xe = r(f.n, hidden), r(f.n, hidden), r(f.e, hidden), r(f.e, hidden)
        scale, shift, mean = (torch.rand(hidden, generator=g) + 0.5).to(dev()), r(hidden), r(hidden)
        Tb, Tf = f.swap(gA2, gA3)       # (reversed views: the caller's source-side table is the kernel's destination-side one)
        fused = ops.agg_bwd_fused(ge, Tf, Uf, Tb, Ub, gA2, gA3, f.views, de, xe, scale, shift, mean, f.n)
        s_in, s_out = f.swap(fused[0], fused[1])
        assert torch.equal(s_in, to_f(want["sum_in"])), (form, "agg_bwd_fused", _where(s_in, to_f(want["sum_in"])))
        assert torch.equal(s_out, to_f(want["sum_out"])), (form, "agg_bwd_fused", _where(s_out, to_f(want["sum_out"])))
        # segment_sum2 on integer rows
        seg_in, seg_out = f.swap(*ops.segment_sum2(X.to(dev()), f.views, f.n))
        w_in, w_out = ag.exact_segment_sums(gs, gd, X.to(dev()), f.n)
        assert torch.equal(seg_in, to_f(w_in)) and torch.equal(seg_out, to_f(w_out)), (form, "segment_sum2")


def _where(got, want):
    bad = torch.nonzero((got != want).any(1)).flatten()
    i = int(bad[0])
    return f"{bad.numel()} rows differ, first node {i}: got {got[i, :4].tolist()} want {want[i, :4].tolist()}"


def _real_inputs(f, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    return {"e": 3.0 * torch.randn(f.e, hidden, generator=g), "h": torch.randn(f.n, hidden, generator=g),
            "P": torch.randn(f.n, 3 * hidden, generator=g), "scale": 0.5 + torch.rand(hidden, generator=g),
            "shift": torch.randn(hidden, generator=g)}


def _rows_mask(n, rows):
    m = torch.zeros(n, dtype=torch.bool, device=dev())
    if rows:
        m[torch.tensor(rows, device=dev())] = True
    return m


@pytest.mark.parametrize("name,hidden", SMALL + MANY)
def test_real_valued_against_the_checker(name, hidden):
    H = hidden
    for form in FORMS:
        f = _Form(name, form)
        t = _real_inputs(f, H, seed=7 * H + len(name))
        d = {k: v.to(dev()) for k, v in t.items()}
        t64 = {k: v.double() for k, v in d.items()}       # the checker's torch statement in float64, evaluated on the device (the host
        A = lambda x: (x[:, :H], x[:, H:2 * H], x[:, 2 * H:])  # noqa: E731     takes seconds per reference at 300k rows)
        args = (d["e"], *A(d["P"]), d["h"])
        ref = lambda norm, x=t64: cpu_ops.node_aggregate(x["e"], *A(x["P"]), f.gcv, x["h"], norm, x["scale"], x["shift"]).cpu()  # noqa: E731
        refs = {norm: ref(norm) for norm in (ops.NORM_AFFINE, ops.NORM_LAYER)}      # computed once, shared below
        got = f.aggregate(*args, ops.NORM_AFFINE, d["scale"], d["shift"])
        _assert_close(got, refs[ops.NORM_AFFINE], scale=10.0)
        ln = f.aggregate(*args, ops.NORM_LAYER, d["scale"], d["shift"])
        _assert_close(ln, refs[ops.NORM_LAYER], scale=10.0)
        # LayerNorm over the first w < H channels of zero-padded rows
        w = H - 13
        pad = {k: v.clone() for k, v in t.items()}
        pad["h"][:, w:], pad["scale"][w:], pad["shift"][w:] = 0.0, 0.0, 0.0
        pad["P"].view(f.n, 3, H)[:, :, w:] = 0.0
        dp = {k: v.to(dev()) for k, v in pad.items()}
        over = ops.NORM_LAYER | (w << 8)
        got_w = f.aggregate(dp["e"], *A(dp["P"]), dp["h"], over, dp["scale"], dp["shift"])
        _assert_close(got_w, ref(over, {k: v.double() for k, v in dp.items()}), scale=10.0)
        assert not got_w[:, w:].any()
        # the training form
        v, fwd, bwd, rdf, rdb = f.raw1(d["e"], *A(d["P"]))
        wv, wf, wrf, wb, wrb = cpu_ops.node_aggregate_raw(t64["e"], *A(t64["P"]), f.gcv, 1, f.n)
        for g_, w_, sc in ((v, wv, 10.0), (fwd, wf, 10.0), (bwd, wb, 10.0), (rdf, wrf, None), (rdb, wrb, None)):
            _assert_close(g_, w_.cpu(), scale=sc)
        # bits: a second run; the rows written under num_nodes_out; ragged node ranges from node 0 with a hub outside the first range
        for norm, first in ((ops.NORM_AFFINE, got), (ops.NORM_LAYER, ln)):
            assert torch.equal(f.aggregate(*args, norm, d["scale"], d["shift"]), first), (form, norm)
            cut = f.hubs[len(f.hubs) // 2] if f.hubs else f.n // 2          # (hubs below the cut are written, this one and the later ones are not)
            part = f.aggregate(*args, norm, d["scale"], d["shift"], num_nodes_out=cut)
            assert torch.equal(part[:cut], first[:cut]), (form, norm, cut)
            out = torch.full_like(first, float("nan"))
            bounds = sorted({0, 1, f.n // 3, f.n // 3 + 1, min(4096, f.n - 1), f.n})
            assert not f.hubs or f.hubs[-1] >= bounds[1]
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                f.aggregate(*args, norm, d["scale"], d["shift"], node_range=(lo, hi), out=out)
            assert torch.equal(out, first), (form, norm)
            # the single-wave path: every non-hub row keeps its bits, every hub row stays within the bar
            try:
                ops.set_tuning(6, 1)
                single = f.aggregate(*args, norm, d["scale"], d["shift"])
            finally:
                ops.set_tuning(6, 0)
            hub = _rows_mask(f.n, f.hubs)
            assert torch.equal(single[~hub], first[~hub]), (form, norm)
            _assert_close(single, refs[norm], scale=10.0)


@pytest.mark.parametrize("hidden", [64, 128, 256])
def test_tuning_variants_on_the_list_lengths(hidden):
    H = hidden
    for form in FORMS:
        f = _Form("lists", form)
        t = _real_inputs(f, H, seed=H + 1)
        d = {k: v.to(dev()) for k, v in t.items()}
        args = (d["e"], d["P"][:, :H], d["P"][:, H:2 * H], d["P"][:, 2 * H:], d["h"], ops.NORM_AFFINE, d["scale"], d["shift"])
        base = f.aggregate(*args)
        t64 = {k: v.double() for k, v in d.items()}
        want = cpu_ops.node_aggregate(t64["e"], t64["P"][:, :H], t64["P"][:, H:2 * H], t64["P"][:, 2 * H:], f.gcv, t64["h"], ops.NORM_AFFINE,
                                      t64["scale"], t64["shift"]).cpu()
        _assert_close(base, want, scale=10.0)
        try:
            for variant in (1, 2, 3, 4, 5, 6, 8, 14):          # documented as "the same bits"
                ops.set_tuning(7, variant)
                assert torch.equal(f.aggregate(*args), base), (form, variant)
            if H == 128:
                for variant in (9, 10):                        # two nodes per wave: another association
                    ops.set_tuning(7, variant)
                    _assert_close(f.aggregate(*args), want, scale=10.0)
        finally:
            ops.set_tuning(7, 0)


@pytest.mark.parametrize("name,hidden", MANY)
def test_split_hubs_are_a_function_of_the_graph(name, hidden):
    """Which hubs get the split path shows in the bits: a split hub's sums are associated chunk-wise, a single-wave one's item by
    item.  Up to HUB_CAP hubs: all of them differ from the single-wave run.  Beyond: exactly the HUB_CAP lowest node ids - on every
    rebuild of the views (each one drops the cached hub list, the search runs again).  The rows compared are the raw gated sums (mode
    2) next to the node update: in the update a sum's last bits mostly vanish under A1h and the relu, a hub's row can keep its bits by
    chance; 64 raw sums of two thousand terms each do not."""
    H = hidden
    for form in FORMS:
        f = _Form(name, form)
        t = _real_inputs(f, H, seed=H + len(name))
        d = {k: v.to(dev()) for k, v in t.items()}
        run = lambda: f.aggregate(d["e"], d["P"][:, :H], d["P"][:, H:2 * H], d["P"][:, 2 * H:], d["h"], ops.NORM_AFFINE, d["scale"], d["shift"])  # noqa: E731
        sums = lambda: torch.cat(f.raw2(d["e"], d["P"][:, H:2 * H], d["P"][:, 2 * H:]), 1)  # noqa: E731
        outs = []
        for _ in range(3):
            f.views = f.build()
            outs.append((sums(), run()))
        try:
            ops.set_tuning(6, 1)
            single = (sums(), run())
        finally:
            ops.set_tuning(6, 0)
        differs = torch.nonzero((outs[0][0] != single[0]).any(1)).flatten().tolist()
        assert differs == f.hubs[:ag.HUB_CAP], (form, len(differs), sorted(set(differs) ^ set(f.hubs[:ag.HUB_CAP])))
        hub = _rows_mask(f.n, f.hubs)
        assert torch.equal(outs[0][1][~hub], single[1][~hub]), form
        for again in outs[1:]:
            assert torch.equal(again[0], outs[0][0]) and torch.equal(again[1], outs[0][1]), form


# ---------------------------------------------------------------------------------------------- the halves recipe: the backward, exact

BWD_KEYS = ("sum_in", "sum_out", "de", "s1", "s2")


def _halves_case(f, hidden, seed):
    """The halves inputs on the device with the probe wired in (probe_src's rows of both node-sum tables are 1, the probe edges' gates are
    GATE_HALF / GATE_OFF in every channel), and the int64 statement of all five outputs as float32 - after the recipe's CONDITION has been
    asserted for exactly these inputs."""
    t = ag.exact_backward_inputs(f.e, f.n, hidden, seed)
    if f.pos_on is not None:
        t["gates"][f.pos_on], t["gates"][f.pos_off] = ag.GATE_HALF, ag.GATE_OFF
        t["Tb"][f.probe_src], t["Tf"][f.probe_src] = 1.0, 1.0
    t = {k: v.to(dev()) for k, v in t.items()}
    gs, gd = f.s.to(dev()), f.d.to(dev())
    bound = ag.exact_backward_bound(gs, gd, t, f.n)
    assert max(bound.values()) < ag.EXACT_LIMIT, bound
    want = {k: v.float() for k, v in ag.exact_backward(gs, gd, t, f.n).items()}
    return t, want


def _assert_half_premise(f, t, hidden):
    """sigmoid(GATE_HALF) is exactly 0.5 on the device: a node with ONE in-edge of that gate and a table row of 1.0 has a node sum of 0.5
    (mode 2 of node_aggregate_raw, the entry test_exact_sums checks) - on the graph's own probe, or on a one-edge graph where it has none."""
    if f.pos_on is not None:
        a_in, a_out = f.raw2(t["gates"], t["Tb"], t["Tf"])
        probed = (a_out if f.t else a_in)[f.probe_on].cpu()
    else:
        one = ops.GraphViews(torch.zeros(1, dtype=torch.int32, device=dev()), torch.ones(1, dtype=torch.int32, device=dev()), 2)
        ones = torch.ones(2, hidden, device=dev())
        probed = ops.node_aggregate_raw(torch.full((1, hidden), ag.GATE_HALF, device=dev()), None, ones, ones, one, 2, 2)[0][1].cpu()
    print(f"probe sum: gate {ag.GATE_HALF} x table row 1.0 -> {probed[0].item()!r}")
    assert torch.equal(probed, torch.full((hidden,), 0.5)), ("sigmoid(GATE_HALF) is not exactly 0.5", probed)


def _kernel_tables(f, t):
    """The six node tables in the roles the KERNEL gives the stored arrays (reversed views: a caller's source-side table is the kernel's
    destination-side one) -> (Tf, Uf, Tb, Ub, A2h, A3h)."""
    return (t["Tb"], t["Ub"], t["Tf"], t["Uf"], t["A3"], t["A2"]) if f.t else (t["Tf"], t["Uf"], t["Tb"], t["Ub"], t["A2"], t["A3"])


def _fused(f, t, xe, amax=None):
    out = ops.agg_bwd_fused(t["gates"], *_kernel_tables(f, t), f.views, t["de0"].clone(), xe, t["scale"], t["shift"], t["mean"], f.n, amax=amax)
    return dict(zip(BWD_KEYS, f.swap(out[0], out[1]) + tuple(out[2:])))


def _edge_stats(f, t, xe):
    de, s1, s2 = ops.agg_edge_bwd_stats(t["gates"], *_kernel_tables(f, t), f.views, t["de0"].clone(), xe, t["scale"], t["shift"], t["mean"])
    return dict(de=de, s1=s1, s2=s2)


def _where_edge(f, got, want):
    bad = torch.nonzero((got != want).any(1)).flatten()
    p = int(bad[0])
    cols = torch.nonzero(got[p] != want[p]).flatten()[:4]
    return (f"{bad.numel()} de' rows differ, first sorted position {p} of {f.e} = edge ({int(f.s[p])} -> {int(f.d[p])}), channels {cols.tolist()}: "
            f"got {got[p, cols].tolist()} want {want[p, cols].tolist()}")


def _where_columns(got, want):
    bad = torch.nonzero(got != want).flatten()
    c = int(bad[0])
    return f"{bad.numel()} columns differ, first {c}: got {got[c].item()!r} want {want[c].item()!r} (difference {got[c].item() - want[c].item()!r})"


def _assert_outputs(f, got, want, what):
    for k in got:
        if torch.equal(got[k], want[k]):
            continue
        where = _where_edge(f, got[k], want[k]) if k == "de" else _where(got[k], want[k]) if got[k].dim() == 2 else _where_columns(got[k], want[k])
        raise AssertionError((f.form, what, k, where))


def _bits(x):
    return x.float().reshape(1).view(torch.int32)


def _check_backward_entries(f, t, want, hidden):
    """Every entry that forms the aggregation's backward, against the statement, bit for bit."""
    x16 = t["xe"].to(torch.bfloat16)
    assert torch.equal(x16.float(), t["xe"])
    top = torch.maximum(want["sum_in"].abs().max(), want["sum_out"].abs().max())
    first = _fused(f, t, t["xe"])
    _assert_outputs(f, first, want, "agg_bwd_fused")
    # a second run, into an amax slot preset to 0: the same bits, and exactly the bits of max(|sum_in|, |sum_out|) in the slot
    slot = torch.zeros(1, dtype=torch.int32, device=dev())
    again = _fused(f, t, t["xe"], amax=slot)
    _assert_outputs(f, again, first, "agg_bwd_fused, second run")
    assert torch.equal(slot, _bits(top)), (f.form, "amax", slot.view(torch.float32).item(), top.item())
    # xe as bfloat16, into a slot preset ABOVE the maximum: left unchanged
    above = _bits(top + 1.0).clone()
    _assert_outputs(f, _fused(f, t, x16, amax=above), want, "agg_bwd_fused, bf16 xe")
    assert torch.equal(above, _bits(top + 1.0)), (f.form, "amax preset above the maximum", above.view(torch.float32).item())
    edge_want = {k: want[k] for k in ("de", "s1", "s2")}
    _assert_outputs(f, _edge_stats(f, t, t["xe"]), edge_want, "agg_edge_bwd_stats")
    _assert_outputs(f, _edge_stats(f, t, x16), edge_want, "agg_edge_bwd_stats, bf16 xe")
    de = ops.agg_edge_bwd(t["gates"], *_kernel_tables(f, t), f.views, t["de0"].clone())
    _assert_outputs(f, dict(de=de), edge_want, "agg_edge_bwd")


@pytest.mark.parametrize("name,hidden", SMALL)
def test_exact_backward(name, hidden):
    """The HALVES recipe (tests/aggregate_graphs.py): gates of GATE_ON / GATE_OFF / GATE_HALF = 0, small integer tables, de0, xe and mean,
    scale in {1, 2}, shift an odd multiple of 0.5.  Premise, asserted first: the device sigmoid of 0 is exactly 0.5 - a one-item probe
    gives 0.5.  Then s (1 - s) is 1/4 or 0, all five outputs of the backward - both node sums, de' per sorted position, s1, s2 - are
    multiples of 1/4 whose partial sums stay below 2^24 quarters (asserted for these very inputs), and every kernel that forms them
    must return the ONE fp32 bit pattern of the int64 statement: agg_bwd_fused (fp32 and bf16 xe, twice, with the amax slot),
    agg_edge_bwd_stats (fp32 and bf16 xe) and agg_edge_bwd."""
    for form in FORMS:
        f = _Form(name, form)
        t, want = _halves_case(f, hidden, seed=hidden + len(name))
        _assert_half_premise(f, t, hidden)
        _check_backward_entries(f, t, want, hidden)


@pytest.mark.parametrize("hidden", [64, 128, 256])
def test_exact_backward_on_the_clamp_and_tail_graphs(hidden):
    """The halves recipe (premise first: sigmoid(0) = 0.5 exactly) on ag.TAILS: the highest-numbered nodes have no edge, so every index
    the fused kernel requests ahead for them is clamped to position E - 1; the last in-list ends AT E - 1; n in {1, 5, 33} is no multiple
    of a workgroup's four nodes; E goes down to 1."""
    for n, e, last in ag.TAILS:
        f = _Form(ag.tails(n, e, last), "plain")
        t, want = _halves_case(f, hidden, seed=n + e)
        if (n, e) == ag.TAILS[0][:2]:
            _assert_half_premise(f, t, hidden)
        try:
            _check_backward_entries(f, t, want, hidden)
        except AssertionError as err:
            raise AssertionError((f"tails n={n} E={e} last in-list {last}",) + err.args) from None


@pytest.mark.parametrize("hidden", [64, 128, 256])
def test_exact_backward_of_the_kernel_variants_kept_for_measurements(hidden):
    """The halves recipe (premise first) on the two variants still built behind set_tuning(4, .): 88 = the fused kernel's first form
    <2, 4, 4> (other step sizes: 8 / 4 / 2 in-edge and 16 / 8 / 4 out-edge items at H = 64 / 128 / 256, an uncut grid), 77 = the edge pass
    with cached loads."""
    f = _Form("lists", "plain")
    t, want = _halves_case(f, hidden, seed=hidden + 5)
    _assert_half_premise(f, t, hidden)
    edge_want = {k: want[k] for k in ("de", "s1", "s2")}
    try:
        ops.set_tuning(4, 88)
        _assert_outputs(f, _fused(f, t, t["xe"]), want, "agg_bwd_fused <2,4,4>")
        _assert_outputs(f, _fused(f, t, t["xe"].to(torch.bfloat16)), want, "agg_bwd_fused <2,4,4>, bf16 xe")
        ops.set_tuning(4, 77)
        _assert_outputs(f, _edge_stats(f, t, t["xe"]), edge_want, "agg_edge_bwd_stats, cached loads")
        _assert_outputs(f, _edge_stats(f, t, t["xe"].to(torch.bfloat16)), edge_want, "agg_edge_bwd_stats, cached loads, bf16 xe")
    finally:
        ops.set_tuning(4, 0)


@pytest.mark.parametrize("name,hidden", SMALL)
def test_exact_in_edge_backward(name, hidden):
    """node_aggregate_in_bwd on the halves recipe (premise first): its de' is the statement with Tb = Ub = A3 = 0, its dA2h the statement's
    sum_out."""
    f = _Form(name, "plain")
    t, _ = _halves_case(f, hidden, seed=hidden + len(name) + 1)
    _assert_half_premise(f, t, hidden)
    zero = torch.zeros_like(t["Tb"])
    t0 = dict(t, Tb=zero, Ub=zero, A3=zero)
    want = {k: v.float() for k, v in ag.exact_backward(f.s.to(dev()), f.d.to(dev()), t0, f.n).items()}
    de = t["de0"].clone()
    dA2h = ops.node_aggregate_in_bwd(t["gates"], t["Tf"], t["Uf"], t["A2"], f.views, de)
    _assert_outputs(f, dict(de=de, sum_out=dA2h), want, "node_aggregate_in_bwd")


@pytest.mark.parametrize("name,hidden", SMALL)
def test_exact_segment_sums_with_amax_and_one_list_at_a_time(name, hidden):
    """Integer rows (the exact recipe's X): segment_sum2 with the amax slot - the same sums, the bits of their largest |element| in a slot
    preset to 0, a slot preset above it unchanged - and segment_sum over in_ptr and over out_ptr / out_pos."""
    for form in FORMS:
        f = _Form(name, form)
        X = ag.exact_inputs(f.e, f.n, hidden, seed=hidden + len(name))[3].to(dev())
        w_in, w_out = (w.float() for w in ag.exact_segment_sums(f.s.to(dev()), f.d.to(dev()), X, f.n))
        top = torch.maximum(w_in.abs().max(), w_out.abs().max())
        for preset in (torch.zeros((), device=dev()), top + 1.0):
            slot = _bits(preset).clone()
            seg_in, seg_out = f.swap(*ops.segment_sum2(X, f.views, f.n, amax=slot))
            assert torch.equal(seg_in, w_in) and torch.equal(seg_out, w_out), (form, "segment_sum2 with amax", _where(torch.cat([seg_in, seg_out], 1), torch.cat([w_in, w_out], 1)))
            assert torch.equal(slot, _bits(torch.maximum(top, preset))), (form, "amax", slot.view(torch.float32).item(), top.item())
        one_in, one_out = f.swap(ops.segment_sum(X, f.views.in_ptr, None, f.n), ops.segment_sum(X, f.views.out_ptr, f.views.out_pos, f.n))
        assert torch.equal(one_in, w_in), (form, "segment_sum over in_ptr", _where(one_in, w_in))
        assert torch.equal(one_out, w_out), (form, "segment_sum over out_ptr / out_pos", _where(one_out, w_out))
