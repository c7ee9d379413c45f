"""The edge gate's entries against the integer cases of tests/gate_cases.py, bit for bit (torch.equal) on every route.

The cases are built so that the fp64 statement is an fp32 value under every arithmetic the gate has (gate_cases.py's header gives the
argument from the kernels' headers, tests/test_gate_cases.py checks it and shows which mutant each case catches): a gate that gathers a
neighbouring table row, drops or doubles a tile, reads the residual after the write, or rounds bf16 storage the wrong way cannot return
the statement.  Which kernel a call lands on is read from the dispatch in csrc/edge_gate.hip (gate_cases.gate_kernel) and
reference_order.hip (gate_cases.ref_geometry); the edge counts come from that kernel's tile height and the device's persistent grid.

Every test starts with a one-row, one-non-zero premise on each route it runs, so that a failure separates "the recipe is not exact here"
from "the kernel is wrong".  Every output the library writes is a sentinel-filled buffer with 64 guard rows behind the E rows handed in
(the fused statistics' partial rows: 16 guard rows behind gnnome_edge_gate_raw_stats_rows); entries whose ops wrapper allocates the
output itself are called through the library as the wrapper calls them (*_direct below), and the wrapper is compared with that at one
count per graph.  Every exact call is launched twice: same bits.

LayerNorm cannot be exact: those calls run on the same inputs under the bound test_edge_gate applies (_assert_close, scale=20).
Each test prints the record of what it ran (pytest -s).
"""
import ctypes

import numpy as np
import pytest
import torch

import gate_cases as gc
from gnnome_amd import _lib, ops
from gnnome_amd.ops import _ptr, _stream
from test_hip_parity import _assert_close

pytestmark = pytest.mark.gpu
S = gc.SENTINEL


def dev():
    return torch.device("cuda", 0)


def grid():
    return gc.persistent_grid(torch.cuda.get_device_properties(dev()).multi_processor_count)


class DevCase:
    """A gate_cases.Case on the device: the tables as column blocks 3 and 4 of a [N, 5H + 4] projection-like table with sentinel columns
    around them (the model's own use; `shifted` moves both blocks one float to the right, which breaks their 16-byte alignment), and the
    fp64 statements as fp32 tensors."""

    def __init__(self, case, enc=False, norms=()):
        d, H = dev(), case.H
        self.case, self.H, self.E, self.rows, self.name = case, H, case.E, case.rows, case.name
        views = ops.GraphViews(case.src.to(d), case.dst.to(d), case.N, node_perm=case.node_perm)
        assert torch.equal(views.srt_src.cpu(), case.views.srt_src) and torch.equal(views.srt_dst.cpu(), case.views.srt_dst)
        assert torch.equal(views.srt_eid.cpu(), case.views.srt_eid)
        self.views = views.reversed() if case.swapped else views
        self.table = torch.full((case.N, 5 * H + 4), S, device=d)
        self.table[:, 3 * H:4 * H], self.table[:, 4 * H:5 * H] = case.B1h.to(d), case.B2h.to(d)
        self.shifted = torch.full((case.N, 5 * H + 4), S, device=d)
        self.shifted[:, 3 * H + 1:4 * H + 1], self.shifted[:, 4 * H + 1:5 * H + 1] = case.B1h.to(d), case.B2h.to(d)
        self.table_kept = self.table.clone()
        self.e, self.W3, self.scale, self.shift, self.shift_ln = (t.to(d) for t in (case.e, case.W3, case.scale, case.shift, case.shift_ln))
        self.want = gc.statement(case).float().to(d)
        self.want_ln = {n: gc.statement(case, norm=n) for n in norms}
        if enc:
            self.e_raw, self.enc = gc.raw_features(case.rows).to(d), tuple(w.to(d) for w in gc.encoder(H))
            self.want_enc = gc.encode_statement(case).float().to(d)
        if case.width is None:
            case.release_host()
        self._x = None

    def tables(self, shifted=False):
        """(B1h, B2h) as the host hands them in: on reversed views the blocks change roles (engine.layer)."""
        t, o, H = (self.shifted, 1, self.H) if shifted else (self.table, 0, self.H)
        b1, b2 = t[:, 3 * H + o:4 * H + o], t[:, 4 * H + o:5 * H + o]
        return (b2, b1) if self.case.swapped else (b1, b2)

    def x(self):
        """(x in fp64, x rounded to bf16 in fp64, both as device tensors of their storage type), computed once."""
        if self._x is None:
            x64 = self.case.x64(self.E)
            xr = gc.to_bf16_nearest_even(x64)
            self._x = (x64, xr.double(), x64.float().to(dev()), xr.to(dev()))
        return self._x


_CASES = {}


def dev_case(H, E, kind, T, R, recipe="wide", rows=None, enc=False, norms=(), width=None):
    """Built once and shared by the routes of one width; the cache is emptied when the width changes (the tests run width by width)."""
    key = (H, E, kind, T, R, recipe, rows, enc, norms, width)
    if key not in _CASES:
        if any(k[0] != H for k in _CASES):
            _CASES.clear()
        _CASES[key] = DevCase(gc.Case(H, E, kind, T, R, recipe, rows, width), enc, norms)
    return _CASES[key]


def _diff(got, want):
    bad = (got != want).nonzero()
    r, c = bad[0].tolist()
    return f"{bad.shape[0]} of {want.numel()} wrong, first at row {r} channel {c}: got {got[r, c].item()!r}, want {want[r, c].item()!r}"


def _exact(wrong, tag, run, want):
    """run() twice: the statement, and the same bits again."""
    got = run()
    if not torch.equal(got, want):
        wrong.append(f"{tag}: {_diff(got, want)}")
    elif not torch.equal(run(), got):
        wrong.append(f"{tag}: a second launch gives other bits")
    return got


def run_gate(dc, in_place, norm=0, shifted=False):
    """ops.edge_gate on sentinel-guarded buffers -> e'[:E].  Rows from E on (the prefix's rest, the 64 guard rows) must stay as they were."""
    E, rows, H = dc.E, dc.rows, dc.H
    buf = torch.full((rows + 64, H), S, device=dev())
    buf[:rows] = dc.e
    b1, b2 = dc.tables(shifted)
    shift = dc.shift if norm == 0 else dc.shift_ln
    ne = None if E == rows else E
    if in_place:
        res = buf
        assert ops.edge_gate(buf[:rows], b1, b2, dc.views, dc.W3, norm, dc.scale, shift, num_edges=ne).data_ptr() == buf.data_ptr()
    else:
        res = torch.full((rows + 64, H), S, device=dev())
        ops.edge_gate(buf[:rows], b1, b2, dc.views, dc.W3, norm, dc.scale, shift, out=res[:rows], num_edges=ne)
        assert torch.equal(buf[:rows], dc.e) and (res[E:rows] == S).all(), f"{dc.name}: the input rows, or output rows past num_edges, changed"
    assert (buf[rows:] == S).all() and (res[rows:] == S).all() and torch.equal(buf[E:rows], dc.e[E:]), f"{dc.name}: rows past num_edges changed"
    return res[:E]


class Premise:
    """One edge from node 0 to node 0, e = W3 = one 1.0 at [0, 0], zero tables, scale 1, shift 0: x is 1.0 and e' is 2.0 at [0, 0], zeros
    elsewhere.  The folded encoder's e0 is the same one-hot row: e_raw = (1, 0), W1[0, 0] = W2[0, 0] = 1.0, zero biases."""

    def __init__(self, H, shifted=False):
        d = dev()
        self.H, self.E, self.rows, self.name = H, 1, 1, f"premise/H{H}"
        self.views = ops.GraphViews(torch.zeros(1, dtype=torch.int32, device=d), torch.zeros(1, dtype=torch.int32, device=d), 1)
        self.e, self.W3 = torch.zeros(1, H, device=d), torch.zeros(H, H, device=d)
        self.e[0, 0] = self.W3[0, 0] = 1.0
        self.table, self.o = torch.zeros(1, 2 * H + 8, device=d), 1 if shifted else 0
        self.scale, self.shift, self.shift_ln = torch.ones(H, device=d), torch.zeros(H, device=d), torch.zeros(H, device=d)
        self.e_raw = torch.tensor([[1.0, 0.0]], device=d)
        W1, W2 = torch.zeros(16, 2, device=d), torch.zeros(H, 16, device=d)
        W1[0, 0] = W2[0, 0] = 1.0
        self.enc = (W1, torch.zeros(16, device=d), W2, torch.zeros(H, device=d))
        self.x1, self.y2 = self.e.clone(), 2 * self.e

    def tables(self, shifted=False):
        return self.table[:, self.o:self.H + self.o], self.table[:, self.H + self.o:2 * self.H + self.o]

    def check(self, got, want, what="e'"):
        assert torch.equal(got.float(), want), f"the premise fails on the device: {what} of 1.0 * 1.0 is not {want[0, 0].item()} on this route"


def premise_gate(H, in_place, shifted=False):
    p = Premise(H, shifted)
    p.check(run_gate(p, in_place), p.y2)


class tuning:
    """`with tuning({key: value})`: the keys are put back to 0 on the way out."""

    def __init__(self, keys):
        self.keys = keys

    def __enter__(self):
        for k, v in self.keys.items():
            ops.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.keys:
            ops.set_tuning(k, 0)


def geometry(H, key0, oop, aligned=True, affine=True):
    kernel = gc.gate_kernel(H, key0, oop, aligned, affine)
    T, R = gc.tile_height(kernel, H), gc.tiles_per_round(kernel, grid())
    return kernel, T, R, gc.edge_counts(T, R, ring=kernel in ("bf", "pl", "ws", "f16"))


ALL_KEYS = [(k, 0) for k in gc.GATE_KEYS] + [(0, 1)]       # (key 0, key 10)


# ------------------------------------------------------------------------------------------------ ops.edge_gate, affine

@pytest.mark.parametrize("rid,H,key0,switch,oop", gc.GATE_ROUTES, ids=[r[0] for r in gc.GATE_ROUTES])
def test_gate_affine_is_exact_on_every_route(rid, H, key0, switch, oop):
    kernel, T, R, counts = geometry(H, key0, oop)
    wrong, ran = [], 0
    with tuning({0: key0, 10: switch}):
        premise_gate(H, not oop)
        for kind in gc.GRAPHS:
            for E in counts:
                dc = dev_case(H, E, kind, T, R)
                _exact(wrong, dc.name, lambda: run_gate(dc, not oop), dc.want)
                assert torch.equal(dc.table, dc.table_kept), f"{dc.name}: the node table changed"
                ran += 1
    print(f"[{rid}] kernel {kernel}, tile {T}, {R} tiles per round: {ran} cases = {len(gc.GRAPHS)} graphs x E in {counts}; {len(wrong)} wrong")
    assert not wrong, f"{rid} ({kernel}): " + "; ".join(wrong[:5])


@pytest.mark.parametrize("kind", gc.GRAPHS)
def test_h256_streaming_gate_cut_into_pieces(kind):
    """Key 4 = 3: the streaming kernel's launch (stream_launch, edge_gate_stream.hip) is cut into pieces of 3 tiles per workgroup group.
    E = T (2 * 3 * groups + 2) + 5: two full pieces, then a third of three tiles, the last of them five rows.  One graph per test: a
    case is 100 MB."""
    H, kernel = 256, gc.gate_kernel(256, 9, True)
    assert kernel == "stream"
    T, groups = gc.tile_height(kernel, H), max(grid() // 4 - (grid() // 4) % 8, 1)
    E, wrong = T * (2 * 3 * groups + 2) + 5, []
    with tuning({0: 9, 4: 3}):
        premise_gate(H, False)
        dc = dev_case(H, E, kind, T, 3 * groups)
        _exact(wrong, dc.name, lambda: run_gate(dc, False), dc.want)
    print(f"[stream pieces {kind}] {groups} groups x 3 tiles per piece, E = {E}: three launches; {len(wrong)} wrong")
    assert not wrong, "; ".join(wrong)


@pytest.mark.parametrize("oop", [False, True], ids=["inplace", "out"])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_gate_on_a_prefix_of_the_rows(H, oop):
    """num_edges < e.shape[0]: the rows from num_edges on are untouched in e and in out (run_gate asserts it), on every key and graph.  The
    counts end a prefix inside the first tile, on its edge, one row into the fifth tile and after a single row; the buffer goes on for
    up to five more tiles.  (The round-sized counts are left to the whole-buffer test above: a prefix changes num_edges alone.)"""
    wrong, record = [], []
    for key0, switch in ALL_KEYS:
        kernel, T, R, _ = geometry(H, key0, oop)
        with tuning({0: key0, 10: switch}):
            premise_gate(H, not oop)
            for kind in gc.GRAPHS:
                for E, rows in ((T - 1, T + 7), (T, 3 * T), (4 * T + 1, 4 * T + 2), (1, 5 * T)):
                    dc = dev_case(H, E, kind, T, R, rows=rows)
                    _exact(wrong, f"key {key0}/{switch} {dc.name}", lambda: run_gate(dc, not oop), dc.want)
        record.append(f"{key0}{'+bf16x6' if switch else ''}:{kernel}")
    print(f"[prefix H{H} {'out' if oop else 'inplace'}] " + " ".join(record) + f" x {len(gc.GRAPHS)} graphs x 4 (E, rows); {len(wrong)} wrong")
    assert not wrong, "; ".join(wrong[:5])


@pytest.mark.parametrize("oop", [False, True], ids=["inplace", "out"])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_gate_on_misaligned_table_blocks(H, oop):
    """Blocks one float off a 16-byte boundary: ops._rows lets the view through and the dispatch leaves the ring kernels - for the tile
    kernel, or at H = 256 out of place for the streaming kernel, whose table gathers are then unaligned 16-byte loads."""
    wrong, record = [], []
    for key0 in gc.GATE_KEYS:
        kernel, T, R, counts = geometry(H, key0, oop, aligned=False)
        assert kernel == ("stream" if H == 256 and oop and key0 in (0, 9) else "tile")
        with tuning({0: key0}):
            premise_gate(H, not oop, shifted=True)
            for kind in gc.GRAPHS:
                for E in counts:
                    dc = dev_case(H, E, kind, T, R)
                    b1, _ = dc.tables(shifted=True)
                    assert b1.data_ptr() % 16 != 0 and ops._rows(b1, "B1h")[1] % 4 == 0
                    _exact(wrong, f"key {key0} {dc.name}", lambda: run_gate(dc, not oop, shifted=True), dc.want)
        record.append(f"{key0}:{kernel}")
    print(f"[misaligned H{H} {'out' if oop else 'inplace'}] " + " ".join(record) + f" x {len(gc.GRAPHS)} graphs x E in {counts}; {len(wrong)} wrong")
    assert not wrong, "; ".join(wrong[:5])


# ------------------------------------------------------------------------------------------------ ops.edge_gate, LayerNorm

@pytest.mark.parametrize("H", [64, 128, 256])
def test_gate_layernorm_on_the_integer_cases(H):
    """LayerNorm, and LayerNorm over the first w < H channels of a zero-padded narrower model (the entry's premise: the padded channels of
    e, W3 and the tables hold zeros), always run on the tile kernel whatever key 0 says.  Not exact: the bound of test_edge_gate."""
    w = H - 24
    ran = 0
    for key0 in gc.GATE_KEYS:
        kernel, T, R, counts = geometry(H, key0, True, affine=False)
        assert kernel == "tile"
        with tuning({0: key0}):
            for kind in gc.GRAPHS:
                for E in counts:
                    for norm, width in ((ops.NORM_LAYER, None), ((w << 8) | ops.NORM_LAYER, w)):
                        dc = dev_case(H, E, kind, T, R, norms=(norm,), width=width)
                        for in_place in (True, False):
                            _assert_close(run_gate(dc, in_place, norm=norm), dc.want_ln[norm], scale=20.0)
                            ran += 1
    print(f"[layernorm H{H}] tile kernel, keys {gc.GATE_KEYS} x {len(gc.GRAPHS)} graphs x E in {counts}: {ran} launches within 1e-5 * 20")


# ------------------------------------------------------------------------------------------------ ops.edge_gate_encode

def _guard(dc, what, buf, E):
    fill = torch.full_like(buf[E:], S)      # (bf16 storage: the sentinel as bf16 rounds it)
    assert torch.equal(buf[E:], fill), f"{dc.name}: the guard rows behind {what} changed"


def _encode_direct(dc, shifted=False):
    """gnnome_edge_gate_encode_f32 through the library, as ops.edge_gate_encode calls it, on a guarded output."""
    b1, b2 = dc.tables(shifted)
    out = torch.full((dc.E + 64, dc.H), S, device=dev())
    W1, b1e, W2, b2e = dc.enc
    _lib.check(_lib.load().gnnome_edge_gate_encode_f32(_ptr(dc.e_raw), _ptr(dc.views.srt_eid), _ptr(W1), _ptr(b1e), _ptr(W2), _ptr(b2e), _ptr(out), dc.E,
                                                       dc.H, _ptr(b1), _ptr(b2), b1.stride(0), _ptr(dc.views.srt_src), _ptr(dc.views.srt_dst),
                                                       _ptr(dc.W3), dc.W3.stride(0), _ptr(dc.scale), _ptr(dc.shift), _stream(dev())),
               "edge_gate_encode_f32")
    _guard(dc, "e_out", out, dc.E)
    return out[:dc.E]


# (hidden, key 0) -> the kernel gnnome_edge_gate_encode_f32 lands on (edge_gate.hip, edge_gate_bf.hip gate_bf_launch); None: refused
ENCODE_ROUTES = {(64, 0): "bf", (64, 7): "bf", (64, 8): "bf", (64, 5): "ws", (128, 0): "enc16", (128, 7): "pl", (128, 8): "bf", (128, 5): "ws",
                 (256, 0): "f16", (256, 5): None, (256, 7): None, (256, 8): None}


@pytest.mark.parametrize("H,key0", list(ENCODE_ROUTES), ids=[f"H{h}-key{k}" for h, k in ENCODE_ROUTES])
def test_gate_with_folded_encoder_is_exact(H, key0):
    kernel = ENCODE_ROUTES[(H, key0)]
    T = 64 if H == 64 else 32
    R = gc.tiles_per_round("f16" if H == 256 else "bf", grid())
    counts = gc.edge_counts(T, R)
    with tuning({0: key0}):
        if kernel is None:     # H = 256 is built on the default kernels only
            dc = dev_case(H, T + 1, "uniform", T, R, enc=True)
            assert not ops.can_fuse_edge_encoder(dc.e_raw, dc.enc, H, 0, dc.tables()[0])
            with pytest.raises(_lib.GnnomeHipError):
                _encode_direct(dc)
            print(f"[encode H{H} key {key0}] refused by the dispatch")
            return
        p = Premise(H)
        p.check(_encode_direct(p), p.y2)
        wrong = []
        for kind in gc.GRAPHS:
            for E in counts:
                dc = dev_case(H, E, kind, T, R, enc=True)
                assert ops.can_fuse_edge_encoder(dc.e_raw, dc.enc, H, 0, dc.tables()[0])
                got = _exact(wrong, dc.name, lambda: _encode_direct(dc), dc.want_enc)
                if E == counts[4] and not torch.equal(ops.edge_gate_encode(dc.e_raw, dc.enc, *dc.tables(), dc.views, dc.W3, dc.scale, dc.shift), got):
                    wrong.append(f"{dc.name}: ops.edge_gate_encode differs from the direct call")
        with pytest.raises(_lib.GnnomeHipError):      # misaligned tables are refused (GN_REQUIRE), never read
            _encode_direct(dc, shifted=True)
    print(f"[encode H{H} key {key0}] kernel {kernel}, tile {T}, {R} tiles per round: {len(gc.GRAPHS)} graphs x E in {counts}; {len(wrong)} wrong")
    assert not wrong, "; ".join(wrong[:5])


# ------------------------------------------------------------------------------------------------ ops.edge_gate_ref

def _b3(H):
    return ((torch.arange(H) % 9) - 4).float()


def _ref_in_place(dc, b3, shift):
    """ops.edge_gate_ref on a guarded buffer (the wrapper updates the caller's e in place) -> e'[:E]."""
    E, rows = dc.E, dc.rows
    buf = torch.full((rows + 64, dc.H), S, device=dev())
    buf[:rows] = dc.e
    ops.edge_gate_ref(buf[:rows], *dc.tables(), dc.views, dc.W3, b3, dc.scale, shift, num_edges=None if rows == E else E)
    assert torch.equal(buf[E:rows], dc.e[E:]) and (buf[rows:] == S).all(), f"{dc.name}: rows past num_edges changed"
    return buf[:E]


def _ref_raw_edges_direct(dc, b3, shift):
    """gnnome_edge_gate_ref_f32 with e_in = NULL and the raw edge features, as ops.edge_gate_ref(None, ..., raw_edges=) calls it, guarded."""
    b1, b2 = dc.tables()
    out = torch.full((dc.E + 64, dc.H), S, device=dev())
    W1, b1e, W2, b2e = dc.enc
    _lib.check(_lib.load().gnnome_edge_gate_ref_f32(_ptr(None), _ptr(out), dc.E, dc.H, _ptr(b1), _ptr(b2), b1.stride(0), _ptr(dc.views.srt_src),
                                                    _ptr(dc.views.srt_dst), _ptr(dc.W3), dc.W3.stride(0), _ptr(b3), _ptr(dc.scale), _ptr(shift),
                                                    _ptr(dc.e_raw), _ptr(dc.views.srt_eid), _ptr(W1), _ptr(b1e), _ptr(W2), _ptr(b2e), _stream(dev())),
               "edge_gate_ref_f32")
    _guard(dc, "e_out", out, dc.E)
    return out[:dc.E]


def _ref_encode_statement(c, b3, shift):
    e0 = gc.encoded64(c)
    a, b = c.first_second()
    x = e0 @ c.W3.double().t() + b3.double() + c.B1h.double()[a] + c.B2h.double()[b]
    return (torch.relu(x * c.scale.double() + shift.double()) + e0).float()


def _ref_premise(H):
    p, zero = Premise(H), torch.zeros(H, device=dev())
    p.check(_ref_in_place(p, zero, p.shift), p.y2)
    p.check(_ref_raw_edges_direct(p, zero, p.shift), p.y2)


@pytest.mark.parametrize("key8", [0, 1])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_reference_order_gate_is_exact(H, key8):
    """gnnome_edge_gate_ref_f32 (b3 separate, a non-zero integer): in place, the raw_edges form and a num_edges prefix, at the first-tile
    counts of its kernel (gate_cases.ref_geometry).  The round-boundary counts of the persistent form follow in the next test."""
    d, b3 = dev(), _b3(H).to(dev())
    kernel, T, R = gc.ref_geometry(H, key8, grid())
    counts = gc.edge_counts(T, R or 8, ring=False)
    wrong = []
    with tuning({8: key8}):
        _ref_premise(H)
        for kind in gc.GRAPHS:
            for E in counts:
                for rows in (E, E + 37):
                    dc = dev_case(H, E, kind, T, R or 8, rows=rows, enc=True)
                    shift = dc.shift - b3 * dc.scale        # scale * (x + b3) + shift' = scale * x + shift: multiples of 0.5, still exact
                    _exact(wrong, dc.name, lambda: _ref_in_place(dc, b3, shift), dc.want)
                    if rows == E:
                        want = _ref_encode_statement(dc.case, b3.cpu(), shift.cpu()).to(d)
                        got = _exact(wrong, dc.name + " raw_edges", lambda: _ref_raw_edges_direct(dc, b3, shift), want)
                        if E == counts[4] and not torch.equal(ops.edge_gate_ref(None, *dc.tables(), dc.views, dc.W3, b3, dc.scale, shift,
                                                                                raw_edges=(dc.e_raw, dc.enc)), got):
                            wrong.append(f"{dc.name}: ops.edge_gate_ref(raw_edges=) differs from the direct call")
    print(f"[edge_gate_ref H{H} key8={key8}] kernel {kernel}, {T} rows per pass: {len(gc.GRAPHS)} graphs x E in {counts} x (whole, prefix, raw_edges); "
          f"{len(wrong)} wrong")
    assert not wrong, "; ".join(wrong[:5])


@pytest.mark.parametrize("kind", gc.GRAPHS)
@pytest.mark.parametrize("H", [64, 128, 256])
def test_reference_order_gate_at_its_round_boundary(H, kind):
    """k_edge_gate_refm is persistent: 4 * persistent_grid() workgroups, each pass T rows (launch_gate_refm), so from R T + 1 rows on a
    workgroup runs a second pass.  E = R T - 1, R T, R T + 1 in place, R T + 1 of R T + 38 rows as a prefix, and R T + 1 through the
    raw_edges form.  (It keeps no ring: there is no 4 R T count.  The scalar form, key 8 = 1, is one pass of one row per thread and has
    no round.)  One graph per test: a case is 33 MB."""
    d, b3 = dev(), _b3(H).to(dev())
    kernel, T, R = gc.ref_geometry(H, 0, grid())
    wrong = []
    _ref_premise(H)
    for E, rows in ((R * T - 1, None), (R * T, None), (R * T + 1, None), (R * T + 1, R * T + 38)):
        dc = dev_case(H, E, kind, T, R, rows=rows, enc=(E == R * T + 1 and rows is None))
        shift = dc.shift - b3 * dc.scale
        _exact(wrong, dc.name, lambda: _ref_in_place(dc, b3, shift), dc.want)
        if E == R * T + 1 and rows is None:
            want = _ref_encode_statement(dc.case, b3.cpu(), shift.cpu()).to(d)
            _exact(wrong, dc.name + " raw_edges", lambda: _ref_raw_edges_direct(dc, b3, shift), want)
    print(f"[edge_gate_ref round H{H} {kind}] kernel {kernel}, {T} rows per pass, {R} workgroups: E in {R * T - 1, R * T, R * T + 1}, prefix, raw_edges; "
          f"{len(wrong)} wrong")
    assert not wrong, "; ".join(wrong[:5])


# ------------------------------------------------------------------------------------------------ raw gate, statistics, bf16 storage

def _tables_args(dc):
    b1, b2 = dc.tables()
    return (_ptr(b1), _ptr(b2), b1.stride(0), _ptr(dc.views.srt_src), _ptr(dc.views.srt_dst), _ptr(dc.W3), dc.W3.stride(0))


def _raw_direct(dc):
    """gnnome_edge_gate_raw_f32 as ops.edge_gate_raw calls it, on a guarded output."""
    out = torch.full((dc.E + 64, dc.H), S, device=dev())
    _lib.check(_lib.load().gnnome_edge_gate_raw_f32(_ptr(dc.e), _ptr(out), dc.E, dc.H, *_tables_args(dc), _stream(dev())), "edge_gate_raw_f32")
    _guard(dc, "x_out", out, dc.E)
    return out[:dc.E]


def _stats_rows(H):
    rows = ctypes.c_int(0)
    _lib.check(_lib.load().gnnome_edge_gate_raw_stats_rows(H, ctypes.byref(rows)), "edge_gate_raw_stats_rows")
    return rows.value


def _raw_stats_direct(dc, storage, with_x=True):
    """gnnome_edge_gate_raw_stats_f32 / _x16 as ops.edge_gate_raw_moments (with_x) and ops.edge_gate_moments_only call them: the centre from
    gnnome_gate_center_f32, x_out with 64 guard rows, stats_partial with 16 guard rows behind the gnnome_edge_gate_raw_stats_rows(H) rows the
    entry owns -> (xe[:E] or None, (d1, d2, centre, E))."""
    lib, d, H, E = _lib.load(), dev(), dc.H, dc.E
    x16 = storage == torch.bfloat16
    center = torch.empty(H, device=d)
    _lib.check(lib.gnnome_gate_center_f32(_ptr(dc.e), E, H, *_tables_args(dc), _ptr(center), _stream(d)), "gate_center_f32")
    R = _stats_rows(H)
    partial = torch.full((R + 16, 2 * H), S, device=d)
    out = torch.full((E + 64, H), S, device=d, dtype=storage) if with_x else None
    entry = lib.gnnome_edge_gate_raw_stats_x16 if x16 else lib.gnnome_edge_gate_raw_stats_f32
    _lib.check(entry(_ptr(dc.e), _ptr(out), E, H, *_tables_args(dc), _ptr(center), _ptr(partial), _stream(d)), "edge_gate_raw_stats")
    _guard(dc, "stats_partial", partial, R)
    if with_x:
        _guard(dc, "x_out", out, E)
    sums = ops._partial_sums(partial[:R], H)
    return (out[:E] if with_x else None), (sums[:H], sums[H:], center, E)


def _bn_direct(dc, shift, storage):
    """gnnome_edge_gate_bn_f32 / _x16 as ops.edge_gate_bn calls them, e_out and x_out guarded -> (e'[:E], xe[:E])."""
    lib, d, H, E = _lib.load(), dev(), dc.H, dc.E
    e_new = torch.full((E + 64, H), S, device=d)
    xe = torch.full((E + 64, H), S, device=d, dtype=storage)
    entry = lib.gnnome_edge_gate_bn_x16 if storage == torch.bfloat16 else lib.gnnome_edge_gate_bn_f32
    _lib.check(entry(_ptr(dc.e), _ptr(e_new), _ptr(xe), E, H, *_tables_args(dc), _ptr(dc.scale), _ptr(shift), _stream(d)), "edge_gate_bn")
    _guard(dc, "e_out", e_new, E)
    _guard(dc, "x_out", xe, E)
    return e_new[:E], xe[:E]


@pytest.mark.parametrize("key0", [0, 1])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_raw_gate_is_exact(H, key0):
    """gnnome_edge_gate_raw_f32: the tile kernel, and at H = 256 under key 0 the plane form's raw mode (edge_tile_f16.hip)."""
    kernel = "f16" if H == 256 and key0 == 0 else "tile"
    T, R = gc.tile_height(kernel, H), gc.tiles_per_round(kernel, grid())
    counts = gc.edge_counts(T, R, ring=kernel == "f16")
    wrong = []
    with tuning({0: key0}):
        p = Premise(H)
        p.check(_raw_direct(p), p.x1, "x")
        for kind in gc.GRAPHS:
            for E in counts:
                dc = dev_case(H, E, kind, T, R)
                got = _exact(wrong, dc.name, lambda: _raw_direct(dc), dc.x()[2])
                if E == counts[4] and not torch.equal(ops.edge_gate_raw(dc.e, *dc.tables(), dc.views, dc.W3), got):
                    wrong.append(f"{dc.name}: ops.edge_gate_raw differs from the direct call")
    print(f"[edge_gate_raw H{H} key {key0}] kernel {kernel}: {len(gc.GRAPHS)} graphs x E in {counts}; {len(wrong)} wrong")
    assert not wrong, "; ".join(wrong[:5])


def _ulp(t):
    return torch.from_numpy(np.spacing(t.abs().float().numpy())).double()


def _check_stats(name, mean, var, x64, wrong):
    """mean = centre + S1 / E and var = S2 / E - (S1 / E)^2 from exact sums: 2 and 4 ulp of the larger term, the roundings of the three or
    four fp32 operations behind them."""
    c, s1, s2, rows = gc.shifted_sums(x64)
    m64, v64 = gc.mean_var(x64)
    tm = 2 * _ulp(torch.maximum(c.abs(), (s1 / rows).abs()))
    tv = 4 * _ulp(torch.maximum(s2 / rows, (s1 / rows) ** 2))
    em, ev = (mean.double().cpu() - m64).abs(), (var.double().cpu() - v64).abs()
    if (em > tm).any() or (ev > tv).any():
        wrong.append(f"{name}: mean off by {(em / tm.clamp_min(1e-30)).max().item() * 2:.2f} ulp, variance by {(ev / tv.clamp_min(1e-30)).max().item() * 4:.2f} ulp")


def _check_sums(name, moments, rows64, wrong, x64):
    """(d1, d2, centre, rows) against the exact integers.  The centre is sorted row 0 of the statement (with bf16 storage: rounded or not, the
    entry's choice - the sums are taken about the centre it reports)."""
    d1, d2, center, rows = moments
    c = center.double().cpu()
    if not (torch.equal(c, rows64[0]) or torch.equal(c, x64[0])):
        wrong.append(f"{name}: the centre is not sorted row 0")
        return
    d = rows64 - c
    if rows != rows64.shape[0] or not (torch.equal(d1.double().cpu(), d.sum(0)) and torch.equal(d2.double().cpu(), (d * d).sum(0))):
        wrong.append(f"{name}: the shifted sums are not the exact integers")


def _same_moments(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def _stats_kernel(H, key0, x16):
    """raw_stats_impl (edge_gate.hip): H = 256 is the plane form whatever key 0 says; at 64 / 128 keys 0 and 8 are the bf16x6 edge-tile kernels
    (8 partial rows per CU), every other key the exact-fp32 kernel (launch_ws_raw_stats, 1 or 2 rows per CU), which has no bf16 storage:
    refused."""
    if H == 256:
        return "f16"
    if key0 in (0, 8):
        return "pl" if H == 128 and key0 == 0 else "bf"
    return None if x16 else "ws"


STATS_ROUTES = [(H, k) for H in (64, 128) for k in gc.GATE_KEYS] + [(256, 0), (256, 5)]


@pytest.mark.parametrize("H,key0", STATS_ROUTES, ids=[f"H{h}-key{k}" for h, k in STATS_ROUTES])
def test_raw_gate_with_fused_statistics(H, key0):
    """The statistics entries with fp32 and bf16 storage, guarded (the *_direct calls), on every graph: the flat and outlier recipes (every
    shifted sum an integer below 2^24) and - xe and e' alone - the small one, whose rows round in bf16.  ops.edge_gate_raw_stats (fused,
    and unfused on a rows_stats prefix), ops.edge_gate_raw_moments, ops.edge_gate_moments_only and ops.edge_gate_bn are compared with the
    direct calls at 4 T + 1 rows of every graph and on the outlier case."""
    d, wrong = dev(), []
    T = 64 if H == 64 else 32
    R = gc.tiles_per_round("f16" if H == 256 else "bf", grid())
    cases = [("flat", k, n) for k in gc.GRAPHS for n in (1, T - 1, T + 1, 4 * T + 1, R * T + 1)] + \
            [("outlier", "uniform", 4000), ("small", "uniform", 4 * T + 1), ("small", "dups", T - 1), ("small", "straddle", R * T + 1)]
    two_pass = key0 == 0 and H in (128, 256)       # gate_bn_impl / the x_out == NULL form: the default kernels at 128 and (fp32 storage) 256
    with tuning({0: key0}):
        p = Premise(H)
        for storage in (torch.float32, torch.bfloat16):
            if _stats_kernel(H, key0, storage == torch.bfloat16) is None:
                continue
            xe, (d1, d2, c, n) = _raw_stats_direct(p, storage)
            p.check(xe, p.x1, "x")
            assert torch.equal(c, p.x1[0]) and not d1.any() and not d2.any() and n == 1, "the premise fails: the sums about row 0 of one row are not zero"
            if two_pass and (H == 128 or storage == torch.float32):
                e_new, xe = _bn_direct(p, p.shift, storage)
                p.check(e_new, p.y2)
                p.check(xe, p.x1, "x")
        for recipe, kind, E in cases:
            dc = dev_case(H, E, kind, T, R, recipe)
            x64, xr64, x32, x16 = dc.x()
            b1, b2 = dc.tables()
            tag = f"key {key0} {dc.name}"
            wrapper = E == 4 * T + 1 or recipe == "outlier"
            exact_sums = recipe != "small"
            if wrapper:
                xe, mean, var = ops.edge_gate_raw_stats(dc.e, b1, b2, dc.views, dc.W3)
                if not torch.equal(xe, x32):
                    wrong.append(f"{tag} ops.edge_gate_raw_stats xe: {_diff(xe, x32)}")
                if exact_sums:
                    _check_stats(tag + " raw_stats", mean, var, x64, wrong)
                    xe2, mean2, var2 = ops.edge_gate_raw_stats(dc.e, b1, b2, dc.views, dc.W3, rows_stats=E - 3)      # a prefix: the unfused route
                    if not torch.equal(xe2, x32):
                        wrong.append(f"{tag} rows_stats: xe differs")
                    _check_stats(tag + " rows_stats", mean2, var2, x64[:E - 3], wrong)
            for storage, rows64, rows_dev in ((torch.float32, x64, x32), (torch.bfloat16, xr64, x16)):
                sname = "bf16" if storage == torch.bfloat16 else "fp32"
                built = _stats_kernel(H, key0, storage == torch.bfloat16) is not None
                assert ops.can_fuse_gate_moments(dc.e, b1, b2, storage=storage) == built, f"{tag} {sname}: can_fuse_gate_moments"
                if not built:
                    with pytest.raises(_lib.GnnomeHipError):
                        _raw_stats_direct(dc, storage)
                    continue
                xs, mom = _raw_stats_direct(dc, storage)
                xs_again, mom_again = _raw_stats_direct(dc, storage)
                if not torch.equal(xs, rows_dev):
                    wrong.append(f"{tag} raw_stats {sname}: xe is not the {'rounded ' if sname == 'bf16' else ''}statement")
                if not torch.equal(xs_again, xs) or not _same_moments(mom, mom_again):
                    wrong.append(f"{tag} raw_stats {sname}: a second launch gives other bits")
                if exact_sums:
                    _check_sums(f"{tag} raw_stats {sname}", mom, rows64, wrong, x64)
                if wrapper:
                    xs_w, mom_w = ops.edge_gate_raw_moments(dc.e, b1, b2, dc.views, dc.W3, storage=storage)
                    if not torch.equal(xs_w, xs) or not _same_moments(mom_w, mom):
                        wrong.append(f"{tag} ops.edge_gate_raw_moments {sname} differs from the direct call")
                can_two = ops.can_two_pass_gate(dc.e, b1, b2, storage=storage)
                assert can_two == (two_pass and (H == 128 or storage == torch.float32)), f"{tag} {sname}: can_two_pass_gate"
                if not can_two:
                    continue
                _, only = _raw_stats_direct(dc, storage, with_x=False)
                if not _same_moments(only, mom) or not _same_moments(_raw_stats_direct(dc, storage, with_x=False)[1], only):
                    wrong.append(f"{tag} moments_only {sname}: not the sums of the pass that writes xe, or not the same bits twice")
                shift = dc.shift if recipe != "small" else torch.full_like(dc.shift, -600.0)
                want = (torch.relu(rows64 * dc.case.scale.double() + shift.double().cpu()) + dc.e.double().cpu()).float().to(d)
                e_new, xs2 = _bn_direct(dc, shift, storage)
                e_again, xs_again = _bn_direct(dc, shift, storage)
                if not torch.equal(xs2, rows_dev) or not torch.equal(e_new, want):
                    wrong.append(f"{tag} edge_gate_bn {sname}: xe or e' differ from the statement on the {'rounded ' if sname == 'bf16' else ''}rows")
                if not torch.equal(e_again, e_new) or not torch.equal(xs_again, xs2):
                    wrong.append(f"{tag} edge_gate_bn {sname}: a second launch gives other bits")
                if wrapper:
                    if not _same_moments(ops.edge_gate_moments_only(dc.e, b1, b2, dc.views, dc.W3, storage=storage), only):
                        wrong.append(f"{tag} ops.edge_gate_moments_only {sname} differs from the direct call")
                    e_w, xs_w = ops.edge_gate_bn(dc.e, b1, b2, dc.views, dc.W3, dc.scale, shift, storage=storage)
                    if not torch.equal(e_w, e_new) or not torch.equal(xs_w, xs2):
                        wrong.append(f"{tag} ops.edge_gate_bn {sname} differs from the direct call")
    print(f"[raw_stats / moments / bn H{H} key {key0}] fp32: {_stats_kernel(H, key0, False)}, bf16: {_stats_kernel(H, key0, True) or 'refused'}, "
          f"two-pass forms {'run' if two_pass else 'refused'}: {len(cases)} cases = {len(gc.GRAPHS)} graphs x 5 counts flat + outlier + 3 small; {len(wrong)} wrong")
    assert not wrong, "; ".join(wrong[:6])


def test_stats_entries_refuse_what_they_do_not_build():
    """GN_REQUIRE in raw_stats_impl / gate_bn_impl: the two-pass forms exist on the default kernels only, bf16 storage at 256 not under key 10."""
    H = 64
    dc = dev_case(H, 65, "uniform", 64, 8, "flat")
    with pytest.raises(_lib.GnnomeHipError):
        _bn_direct(dc, dc.shift, torch.float32)
    with pytest.raises(_lib.GnnomeHipError):
        _raw_stats_direct(dc, torch.float32, with_x=False)
    dc = dev_case(128, 33, "uniform", 32, 8, "flat")
    with tuning({0: 5}):
        assert not ops.can_two_pass_gate(dc.e, *dc.tables())
        with pytest.raises(_lib.GnnomeHipError):
            _bn_direct(dc, dc.shift, torch.float32)
    with pytest.raises(_lib.GnnomeHipError):      # the raw gate must not run in place
        _lib.check(_lib.load().gnnome_edge_gate_raw_f32(_ptr(dc.e), _ptr(dc.e), dc.E, 128, *_tables_args(dc), _stream(dev())), "edge_gate_raw_f32")
