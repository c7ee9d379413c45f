"""Contig spelling against its statement, byte for byte, at the edges of the kernel (csrc/contig_spell.hip): tile, chunk and line
borders, the 64-lane search over more than 64 and 64^2 contigs and over runs of equal keys, zero-length reads, pieces and contigs,
an unaligned or truncated output, caller-defined gaps, the whole complement table, and the check kernel's grid-stride loop.

The cases and the statement live in tests/contig_cases.py.  The CPU tests below hold every case to the edge it claims, from the
expected image alone; the GPU tests compare the device's bytes with that image.  Every comparison is an exact equality."""
import ctypes

import numpy as np
import pytest
import torch

import contig_cases as cc
from gnnome_amd import _lib, contigs

SENTINEL = 0xA5


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_an_empty_contig_is_its_header_line_alone(tmp_path):
    """FastaWriter writes '>title\\n' and then no line at all for an empty sequence (its wrap loop runs zero times)."""
    contigs.write_fasta(["", "AC", "", ""], tmp_path / "e.fasta", line_width=60)
    want = b">contig_1 length=0\n>contig_2 length=2\nAC\n>contig_3 length=0\n>contig_4 length=0\n"
    assert (tmp_path / "e.fasta").read_bytes() == want
    assert cc.expected_image(["", "AC", "", ""], 60) == want
    assert cc.expected_image(["", "AC", "", ""], 0) == b"AC"
    lay = cc.Layout(["", "AC", "", ""], 60)
    assert lay.body_off == [19, 38, 60, 79] and lay.body_len == [0, 3, 0, 0] and lay.rec_off == [0, 19, 41, 60]


def test_the_image_by_hand():
    assert cc.expected_image(["ACGTA", "G"], 2) == b">contig_1 length=5\nAC\nGT\nA\n>contig_2 length=1\nG\n"
    assert cc.wrap("ACGTA", 2) == b"AC\nGT\nA\n" and cc.wrap("ACGT", 2) == b"AC\nGT\n" and cc.wrap("", 2) == b""
    every = bytes(b for b in range(1, 256) if b != 10).decode("latin-1")       # one character = one byte, whatever the host's encoding
    assert cc.expected_image([every], 300) == b">contig_1 length=254\n" + every.encode("latin-1") + b"\n"
    # the statement on the odd strand: Bio.Seq's table in both cases, every other byte unchanged
    assert cc.node_seq(["ACGTMRWSYKVHDBXNUacgtmrwsykvhdbxnu\x01\xff*-"], 1) == "-*\xff\x01anxvhdbmrswykacgtANXVHDBMRSWYKACGT"


@pytest.mark.parametrize("name", sorted(cc.BUILDERS))
def test_every_case_reaches_the_edge_it_claims(name):
    case = cc.case(name)
    assert case.claims and all(lw >= 0 for lw in case.line_widths)
    assert all(10 not in r for r in case.reads)
    for claim in case.claims:
        assert "lw" not in claim or claim["lw"] in case.line_widths, f"{name}: {claim} names a layout the case does not run"
        assert cc.claim_holds(case, claim), f"{name}: the case no longer reaches {claim}"


def test_a_claim_can_fail():
    """The evaluator is not vacuous: each kind is false on a case that does not reach it."""
    case = cc.Case("plain", ([b"ACGTACGTAC" * 4, b"GG"], [0], [2], [7], [[0, 2], [3], [1]], (0, 60), []))
    assert case.contigs == ["ACGTACGGG", "CC", "GTACGTACGT" * 4]
    for claim in [{"kind": "walks_more_than", "n": 3}, {"kind": "zero_length_contig"}, {"kind": "zero_length_read_walked"},
                  {"kind": "zero_contig_run", "n": 1, "where": "first"}, {"kind": "zero_piece_run", "n": 1, "how": "prefix0"},
                  {"kind": "contig_lengths_include", "lengths": [3]}, {"kind": "width_exceeds_every_contig", "lw": 40},
                  {"kind": "every_byte_value", "parity": 0}, {"kind": "chunk_with_contig_starts", "lw": 0, "n": 4},
                  {"kind": "tile_without_body_byte", "lw": 60}, {"kind": "tile_inside_one_piece", "lw": 0},
                  {"kind": "newline_at_multiple", "lw": 60, "of": cc.TILE}, {"kind": "last_data_byte_at", "lw": 0, "of": cc.TILE, "plus": 0},
                  {"kind": "header_straddles", "lw": 60, "of": cc.TILE}, {"kind": "body_starts_at_multiple", "lw": 60, "of": cc.TILE}]:
        assert not cc.claim_holds(case, claim), claim
    assert cc.claim_holds(case, {"kind": "walks_more_than", "n": 2}) and cc.claim_holds(case, {"kind": "chunk_with_contig_starts", "lw": 0, "n": 3})
    # line width 60: headers at [0, 19), [29, 48), [51, 71); bodies at [19, 29), [48, 51), [71, 112); last data bytes at 27, 49, 110
    assert cc.claim_holds(case, {"kind": "last_data_byte_at", "lw": 60, "of": 7, "plus": 0})
    assert cc.claim_holds(case, {"kind": "last_data_byte_at", "lw": 60, "of": 11, "plus": 5}) and \
        not cc.claim_holds(case, {"kind": "last_data_byte_at", "lw": 60, "of": 11, "plus": 4})
    assert cc.claim_holds(case, {"kind": "header_straddles", "lw": 60, "of": 32}) and not cc.claim_holds(case, {"kind": "header_straddles", "lw": 60, "of": 49})
    assert cc.claim_holds(case, {"kind": "body_starts_at_multiple", "lw": 60, "of": 48})
    assert cc.claim_holds(case, {"kind": "newline_at_multiple", "lw": 60, "of": 28})              # the newline behind contig 1's only line


def test_unit_walks_are_walks_of_the_unit_graph():
    reads, src, dst, prefix = cc.unit_graph(50)
    nodes, off = cc.unit_walks(40, 100)
    walks = cc.split_walks(nodes, off)
    pairs = dict(zip(zip(src, dst), prefix))
    assert [len(w) for w in walks[:4]] == [1, 2, 1, 2] and int(off[-1]) == 60
    assert all(len(w) == 1 or (w[0], w[1]) in pairs for w in walks) and {pairs[(w[0], w[1])] for w in walks if len(w) == 2} == {0, 1}
    assert all((u, (u + 5) % 100) not in pairs for u in range(100))


# ---------------------------------------------------------------------------------------------------------------- GPU

def dev():
    return torch.device("cuda", 0)


_DEVICE = {}


def on_device(reads, src, dst, prefix, key=None):
    """(DecodeGraph, ReadStore) of a case, built once per session."""
    from gnnome_amd.decode import DecodeGraph
    if key is not None and key in _DEVICE:
        return _DEVICE[key]
    n = 2 * len(reads)
    dg = DecodeGraph(src, dst, n, prefix, [len(reads[u >> 1]) for u in range(n)], device=dev())
    store = contigs.ReadStore.from_sequences(reads, device=dev())
    if key is not None:
        _DEVICE[key] = (dg, store)
    return dg, store


def assert_image(got, want, lay, what):
    """got: uint8 tensor or bytes; want: bytes.  On a mismatch: the first differing offset and where it lies."""
    got = got.cpu().numpy().tobytes() if torch.is_tensor(got) else bytes(got)
    assert len(got) == len(want), f"{what}: {len(got)} bytes, expected {len(want)}"
    if got == want:
        return
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    bad = np.flatnonzero(a != b)
    o = int(bad[0])
    raise AssertionError(f"{what}: {bad.size} of {len(want)} bytes differ, first at {lay.describe(o) if lay else o}: got {got[o:o + 1]!r} "
                         f"({got[max(o - 8, 0):o + 8]!r}), expected {want[o:o + 1]!r} ({want[max(o - 8, 0):o + 8]!r})")


def _sample(n):
    return range(n) if n <= 512 else sorted(set(range(0, n, max(n // 200, 1))) | {0, 1, n - 2, n - 1})


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cc.BUILDERS))
def test_bytes_equal_the_statement(name):
    """For every layout the case names: the image, byte for byte; lengths, offsets and sequence(i); respell from line width 0."""
    case = cc.case(name)
    dg, store = on_device(case.reads, case.src, case.dst, case.prefix, key=name)
    lengths = [len(s) for s in case.contigs]
    c0 = contigs.spell_contigs(dg, case.walks, store)
    assert c0.lengths.cpu().tolist() == lengths
    assert c0.offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    assert_image(c0.data, case.layout(0).image, case.layout(0), f"{name}, contigs concatenated")
    for lw in case.line_widths:
        lay = case.layout(lw)
        c = contigs.spell_contigs(dg, case.walks, store, line_width=lw)
        assert_image(c.data, lay.image, lay, f"{name}, line width {lw}")
        assert c.lengths.cpu().tolist() == lengths and len(c) == len(lengths)
        if lw > 0:
            assert c.body_off.tolist() == lay.body_off
            assert_image(c0.respell(lw).data, lay.image, lay, f"{name}, respell({lw})")
        for i in _sample(len(lengths)):
            assert c.sequence(i) == case.contigs[i], f"{name}, line width {lw}: sequence({i})"


@pytest.mark.gpu
def test_a_graph_without_edges_spells_single_node_walks():
    """Every contig a single read: the successor arrays are empty, which the host wrapper used to hand over as null pointers."""
    reads = [b"ACGTN", b"", b"ggR"]
    dg, store = on_device(reads, [], [], [])
    got = contigs.spell_contigs(dg, [[0], [5], [2], [1]], store, line_width=2)
    assert got.fasta_bytes().tobytes() == cc.expected_image(["ACGTN", "Ycc", "", "NACGT"], 2)
    with pytest.raises(_lib.GnnomeHipError, match=r"walk 1: \(0, 2\) is not an edge"):
        contigs.spell_contigs(dg, [[3], [0, 2]], store)


# ---- through the C ABI: an unaligned `out`, caller-defined gaps, a truncated out_bytes

def _plan(name):
    case = cc.case(name)
    dg, store = on_device(case.reads, case.src, case.dst, case.prefix, key=name)
    return case, store, contigs.spell_contigs(dg, case.walks, store)._plan


def _spell(plan, store, body_off, lw, out_ptr, out_bytes):
    lib = _lib.load()
    bo = None if body_off is None else torch.tensor(body_off, dtype=torch.int64, device=dev())
    _lib.check(lib.gnnome_contig_spell(ctypes.c_void_p(plan["nodes"].data_ptr()), int(plan["nodes"].numel()),
                                       ctypes.c_void_p(plan["walk_off"].data_ptr()), int(plan["walk_off"].numel()) - 1,
                                       ctypes.c_void_p(plan["piece_off"].data_ptr()), ctypes.c_void_p(store.data.data_ptr()),
                                       ctypes.c_void_p(store.off.data_ptr()), store.num_reads,
                                       None if bo is None else ctypes.c_void_p(bo.data_ptr()), lw, ctypes.c_void_p(out_ptr), out_bytes,
                                       ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)), "contig_spell")
    torch.cuda.synchronize()


def _bodies_only(lay, cut=None):
    """The expected buffer when only the kernel writes: body bytes below `cut` from the image, the sentinel everywhere else."""
    want = np.full(len(lay.image), SENTINEL, dtype=np.uint8)
    img = np.frombuffer(lay.image, dtype=np.uint8)
    for bo, bl in zip(lay.body_off, lay.body_len):
        want[bo:bo + bl] = img[bo:bo + bl]
    if cut is not None:
        want[cut:] = SENTINEL
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny-many-65", "border-newline_at_tile-lw60"])
@pytest.mark.parametrize("lw", [0, 60])
def test_unaligned_out_takes_the_byte_stores(name, lw):
    """out = a 16-byte aligned buffer + d: the bodies equal the aligned run's, header gaps, the d bytes before and everything from
    out_bytes on keep the sentinel."""
    case, store, plan = _plan(name)
    lay = case.layout(lw)
    total = len(lay.image)
    want = _bodies_only(lay)
    for d in (1, 7, 15):
        buf = torch.full((total + 32,), SENTINEL, dtype=torch.uint8, device=dev())
        assert buf.data_ptr() % 16 == 0
        _spell(plan, store, lay.body_off if lw else None, lw, buf.data_ptr() + d, total)
        got = buf.cpu().numpy()
        assert (got[:d] == SENTINEL).all() and (got[d + total:] == SENTINEL).all(), f"d = {d}: bytes outside [out, out + out_bytes) written"
        assert_image(got[d:d + total].tobytes(), want.tobytes(), lay, f"{name}, line width {lw}, out + {d}")


@pytest.mark.gpu
@pytest.mark.parametrize("lw", [17, 60])
def test_caller_defined_gaps_are_left_alone(lw):
    """body_off with gaps of 0, 1, 15, 16, 17 and 40 000 bytes between bodies (the last: more than two whole tiles inside a gap):
    every body is the wrapped contig, every other byte keeps the sentinel."""
    case, store, plan = _plan("width-edges")
    gaps = (0, 1, 15, 16, 17, 40000)
    bodies = [cc.wrap(s, lw) for s in case.contigs]
    for lead in range(3, cc.TILE, 257):               # the first body's offset, moved until a 40 000-byte gap holds two whole tiles
        body_off, pos, whole = [], lead, 0
        for i, b in enumerate(bodies):
            body_off.append(pos)
            end = pos + len(b)
            pos = end + gaps[i % len(gaps)]
            whole = max(whole, pos // cc.TILE - -(-end // cc.TILE))
        if whole >= 2:
            break
    assert whole >= 2 and any(len(b) == 0 for b in bodies)
    total = pos + 5
    want = np.full(total, SENTINEL, dtype=np.uint8)
    for bo, b in zip(body_off, bodies):
        want[bo:bo + len(b)] = np.frombuffer(b, dtype=np.uint8)
    buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev())
    _spell(plan, store, body_off, lw, buf.data_ptr(), total)
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"line width {lw}: {bad.size} bytes differ, first at offset {int(bad[0])} (tile {int(bad[0]) // cc.TILE}, chunk "
                           f"{int(bad[0]) // cc.CHUNK}), bodies start at {body_off}")


@pytest.mark.gpu
def test_truncated_out_bytes():
    """out_bytes below the image, cut mid-line, on a newline, inside a header gap, at 16384 k and at 16384 k + 1: bytes below the
    cut equal the image (header gaps: untouched), bytes from the cut on keep the sentinel."""
    case, store, plan = _plan("long-piece")
    lay = case.layout(60)
    b1 = lay.body_off[1]
    cuts = {"mid-line": b1 + 61 * 7 + 30, "on a newline": b1 + 61 * 9 + 60, "inside a gap": lay.rec_off[1] + 4, "at a tile": 2 * cc.TILE,
            "one byte into a tile": 4 * cc.TILE + 1}
    assert lay.image[cuts["on a newline"]] == 10 and lay.image[cuts["mid-line"]] != 10 and lay.rec_off[1] < cuts["inside a gap"] < b1
    for layout, lw, where in [(lay, 60, cuts), (case.layout(0), 0, {"at a tile": 3 * cc.TILE, "one byte into a tile": cc.TILE + 1,
                                                                    "mid-chunk": 2 * cc.TILE + 7})]:
        total = len(layout.image)
        for what, cut in where.items():
            assert 0 < cut < total
            buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev())
            _spell(plan, store, layout.body_off if lw else None, lw, buf.data_ptr(), cut)
            assert_image(buf, _bodies_only(layout, cut).tobytes(), layout, f"line width {lw}, cut {what} ({cut})")


# ---- the check kernel: items [0, W) are the walk offsets, items [W, W + S) the steps; the smallest failing item is reported

@pytest.fixture(scope="module")
def unit():
    reads, src, dst, prefix = cc.unit_graph()
    dg, store = on_device(reads, src, dst, prefix)
    return reads, src, dst, prefix, dg, store


def _still_spells(unit):
    reads, src, dst, prefix, dg, store = unit
    walks = [[4, 6, 9], [7]]
    got = contigs.spell_contigs(dg, walks, store)
    assert [got.sequence(i) for i in range(2)] == cc.spell_checker(walks, src, dst, prefix, cc.as_strs(reads))


@pytest.mark.gpu
def test_no_failure_at_more_than_two_trips_of_the_check_grid(unit):
    """W > 64^3 walks and W + S > 2 x 262 144 items, all valid: every thread of the check kernel makes a third trip, and the
    spelled bytes equal the statement."""
    reads, src, dst, prefix, dg, store = unit
    W = cc.WAVE ** 3 + 1000
    nodes, off = cc.unit_walks(W, dg.num_nodes)
    assert W + nodes.size > 2 * cc.CHECK_GRID and W > cc.WAVE ** 3
    want = cc.spell_checker(cc.split_walks(nodes, off), src, dst, prefix, cc.as_strs(reads))
    assert {len(s) for s in want} == {1, 2}
    c = contigs.spell_contigs(dg, (torch.from_numpy(nodes), torch.from_numpy(off)), store)
    assert c.lengths.cpu().tolist() == [len(s) for s in want]
    assert_image(c.data, "".join(want).encode("latin-1"), None, "unit walks")


def _plant(nodes, off, item, W, N):
    """make the step at item index `item` a non-edge: it must be the first node of a two-node walk"""
    s = item - W
    w = int(np.searchsorted(off, s, side="right")) - 1
    assert off[w] == s and off[w + 1] == s + 2, f"item {item} is not the first step of a two-node walk"
    nodes[s + 1] = (nodes[s] + 5) % N
    return w, int(nodes[s]), int(nodes[s + 1])


@pytest.mark.gpu
def test_the_first_of_two_non_edges_is_named(unit):
    """Item order: the W walk-offset items first, then the S steps in order.  One non-edge at item 262 144 + 7 (thread 7 of block 0
    on its second trip), one at a larger item of another block: the error names the first.  Then the last pair of all alone, and a
    node out of range at the very last item."""
    reads, src, dst, prefix, dg, store = unit
    W = 100001
    nodes, off = cc.unit_walks(W, dg.num_nodes, two_node=lambda i: i >= 0)
    S = nodes.size
    assert S == 2 * W and W + S > cc.CHECK_GRID + 7
    first, second = cc.CHECK_GRID + 7, cc.CHECK_GRID + 7 + 108 * cc.CHECK_THREADS + 2
    assert (first % cc.CHECK_GRID) // cc.CHECK_THREADS == 0 and (second % cc.CHECK_GRID) // cc.CHECK_THREADS == 108 and second < W + S

    def run(n):
        return contigs.spell_contigs(dg, (torch.from_numpy(n), torch.from_numpy(off)), store)

    two = nodes.copy()
    w1, u1, v1 = _plant(two, off, first, W, dg.num_nodes)
    w2, _, _ = _plant(two, off, second, W, dg.num_nodes)
    assert w1 < w2
    with pytest.raises(_lib.GnnomeHipError, match=rf"walk {w1}: \({u1}, {v1}\) is not an edge"):
        run(two)
    _still_spells(unit)
    last = nodes.copy()
    w, u, v = _plant(last, off, W + S - 2, W, dg.num_nodes)
    assert w == W - 1
    with pytest.raises(_lib.GnnomeHipError, match=rf"walk {W - 1}: \({u}, {v}\) is not an edge"):
        run(last)
    _still_spells(unit)
    both = two.copy()
    both[S - 2:] = last[S - 2:]
    with pytest.raises(_lib.GnnomeHipError, match=rf"walk {w1}: \({u1}, {v1}\) is not an edge"):
        run(both)
    assert len(run(nodes)) == W
    end, end_off = cc.unit_walks(W, dg.num_nodes, two_node=lambda i: i < W - 1)
    end[-1] = dg.num_nodes + 3                        # the very last item: compared with the range, never used as an index
    with pytest.raises(_lib.GnnomeHipError, match=rf"walk {W - 1}: node {dg.num_nodes + 3} outside"):
        contigs.spell_contigs(dg, (torch.from_numpy(end), torch.from_numpy(end_off)), store)
    _still_spells(unit)


@pytest.mark.gpu
def test_a_bad_offset_is_named_before_a_bad_step(unit):
    """Offset items come before step items, so an empty walk j is reported although walk 0 holds a non-edge."""
    reads, src, dst, prefix, dg, store = unit
    W, j = 300, 211
    nodes, off = cc.unit_walks(W, dg.num_nodes, two_node=lambda i: i >= 0)
    nodes[1] = (nodes[0] + 5) % dg.num_nodes
    bad = off.copy()
    bad[j + 1] = bad[j]
    with pytest.raises(_lib.GnnomeHipError, match=rf"walk {j} is empty"):
        contigs.spell_contigs(dg, (torch.from_numpy(nodes), torch.from_numpy(bad)), store)
    with pytest.raises(_lib.GnnomeHipError, match=rf"walk 0: \({int(nodes[0])}, {int(nodes[1])}\) is not an edge"):
        contigs.spell_contigs(dg, (torch.from_numpy(nodes), torch.from_numpy(off)), store)
    _still_spells(unit)


@pytest.mark.gpu
def test_bad_walk_offsets(unit):
    """Offsets are only compared in the kernel, never used as indices beyond [0, S) and [0, W]: each form is declined by name."""
    reads, src, dst, prefix, dg, store = unit
    nodes = torch.tensor([0, 2, 4, 6, 8, 10, 12, 14], dtype=torch.int32)       # any consecutive pair is an edge (+ 2)
    S = 8
    rise = rf"walk offsets must rise strictly from 0 to num_steps = {S} \(walk %d\)"
    for off, message in [([0, 3, 3, 5, 8], "walk 1 is empty"), ([0, 5, 3, 8], rise % 1), ([1, 3, 8], rise % 0), ([-1, 3, 8], rise % 0),
                         ([0, 3, 7], rise % 1), ([0, 3, 9], rise % 1), ([0, 3, 3, 3, 8], "walk 1 is empty"), ([0, 8, 8], "walk 1 is empty")]:
        with pytest.raises(_lib.GnnomeHipError, match=message):
            contigs.spell_contigs(dg, (nodes, torch.tensor(off, dtype=torch.int64)), store)
        _still_spells(unit)
    good = contigs.spell_contigs(dg, (nodes, torch.tensor([0, 3, 8], dtype=torch.int64)), store)
    assert good.lengths.cpu().tolist() == [3, 5]
