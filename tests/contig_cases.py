"""Adversarial cases for contig spelling (csrc/contig_spell.hip) and the statement they are held to.  CPU only: no kernel is called here.

The statement is `spell_checker` (evaluate.py:38-48 in plain Python) and the host path of `contigs.write_fasta`; `expected_image` turns
a list of contigs into the bytes the device must produce.  Every builder returns

    (reads, src, dst, prefix, walks, line_widths, claims)

reads: list of bytes (read r; node 2r is read r, node 2r+1 its reverse complement); src / dst / prefix: the edge list; walks: lists of
node ids; line_widths: the layouts the case is meant for (0 = contigs concatenated, > 0 = a FASTA image); claims: a list of dicts that
say IN DATA which edge of the kernel the case is built to hit.  `claim_holds` evaluates a claim from the inputs, the expected image and
the offsets read off that image - never from the kernel - so a case cannot quietly stop reaching its edge when a constant changes."""
import bisect
import functools
import os
import tempfile

import numpy as np

from gnnome_amd import contigs

# The kernel's constants, in one place (gnnome_amd/csrc/contig_spell.hip):
TILE = 16384           # kSpellTile = kSpellThreads * 16 * kSpellChunks: output bytes one workgroup owns
CHUNK = 16             # bytes one lane builds and stores at a time (the uint4 store)
WAVE = 64              # lanes of one wavefront: probes per round of wave_last_le
CHECK_GRID = 262144    # kCheckBlocksMax * kCheckThreads: items one trip of the check kernel's grid-stride loop covers
CHECK_THREADS = 256    # kCheckThreads: items of one block per trip

_COMP = str.maketrans("ACGTMRWSYKVHDBXNUacgtmrwsykvhdbxnu", "TGCAKYWSRMBDHVXNAtgcakywsrmbdhvxna")   # Bio.Seq's IUPAC table


def node_seq(seqs, u):
    s = seqs[u >> 1]
    return s if u % 2 == 0 else s.translate(_COMP)[::-1]


def spell_pieces(walks, src, dst, prefix, seqs):
    """evaluate.py:38-48, piece by piece: edges[(u, v)] is the LAST edge id inserted for the pair (graph_parser.py:77-80)."""
    edges = {}
    for i, (u, v) in enumerate(zip(src, dst)):
        edges[(u, v)] = i
    out = []
    for w in walks:
        pieces = [node_seq(seqs, a)[:prefix[edges[(a, b)]]] for a, b in zip(w[:-1], w[1:])]
        out.append(pieces + [node_seq(seqs, w[-1])])
    return out


def spell_checker(walks, src, dst, prefix, seqs):
    """evaluate.py:38-48.  seqs: the reads as str (latin-1 for bytes beyond ASCII)."""
    return ["".join(p) for p in spell_pieces(walks, src, dst, prefix, seqs)]


def as_strs(reads):
    return [r.decode("latin-1") for r in reads]


def expected_image(contig_strs, line_width):
    """The bytes the device must hold: the contigs concatenated (line_width == 0) or the file the host path of write_fasta writes for
    them (line_width > 0; read back as text, so that one character is one byte whatever encoding the host writes files in)."""
    if line_width == 0:
        return "".join(contig_strs).encode("latin-1")
    fd, path = tempfile.mkstemp(suffix=".fasta")
    os.close(fd)
    try:
        contigs.write_fasta(list(contig_strs), path, line_width=line_width)
        with open(path, "r", newline="") as f:
            return f.read().encode("latin-1")
    finally:
        os.unlink(path)


def wrap(seq, line_width):
    """One FASTA body: '\\n' after every line_width characters and after a final partial line; nothing for an empty contig."""
    return "".join(seq[k:k + line_width] + "\n" for k in range(0, len(seq), line_width)).encode("latin-1")


class Layout:
    """Where the bodies lie in an expected image, read off the image itself: body_off[w], body_len[w] (newlines included) and
    rec_off[w] (where contig w's header line starts; = body_off[w] at line_width 0)."""

    def __init__(self, contig_strs, line_width):
        self.lw = line_width
        self.n = [len(s) for s in contig_strs]
        self.image = expected_image(contig_strs, line_width)
        self.rec_off, self.body_off, self.body_len = [], [], []
        pos = 0
        for n in self.n:
            self.rec_off.append(pos)
            if line_width > 0:
                assert self.image[pos:pos + 1] == b">", f"no header at {pos}"
                pos = self.image.index(b"\n", pos) + 1
            blen = n + (-(-n // line_width) if line_width > 0 else 0)
            self.body_off.append(pos)
            self.body_len.append(blen)
            pos += blen
        assert pos == len(self.image), f"bodies end at {pos}, the image at {len(self.image)}"

    def contig_at(self, o):
        """(w, inside a body?) of output offset o: the last contig whose record starts at or before o."""
        w = max(bisect.bisect_right(self.rec_off, o) - 1, 0)
        while w + 1 < len(self.n) and self.rec_off[w + 1] <= o:   # zero-length records at line_width 0
            w += 1
        return w, self.body_off[w] <= o < self.body_off[w] + self.body_len[w]

    def unwrapped(self, w, o):
        """Data bytes of contig w that lie before output offset o (the reads hold no newline)."""
        return (o - self.body_off[w]) - self.image.count(b"\n", self.body_off[w], o)

    def describe(self, o):
        w, inside = self.contig_at(o)
        return (f"offset {o}: tile {o // TILE} (+{o % TILE}), chunk {o // CHUNK} (+{o % CHUNK}), contig {w} of {self.n[w]} bytes, "
                f"{'body byte ' + str(o - self.body_off[w]) + ' of ' + str(self.body_len[w]) if inside else 'outside its body'}")


class Case:
    def __init__(self, name, built):
        self.name = name
        self.reads, self.src, self.dst, self.prefix, self.walks, self.line_widths, self.claims = built
        self.seqs = as_strs(self.reads)
        self.pieces = spell_pieces(self.walks, self.src, self.dst, self.prefix, self.seqs)
        self.contigs = ["".join(p) for p in self.pieces]
        self._layouts = {}

    def layout(self, lw):
        if lw not in self._layouts:
            self._layouts[lw] = Layout(self.contigs, lw)
        return self._layouts[lw]

    def piece_off(self):
        """Start of every piece in the unwrapped stream, walk after walk (S + 1 entries)."""
        off = [0]
        for p in self.pieces:
            for s in p:
                off.append(off[-1] + len(s))
        return off


# ------------------------------------------------------------------------------------------------------------------ claims

def _multiples(of, lo, hi):
    """multiples k * of with k >= 1 in [lo, hi)"""
    k = max(1, -(-lo // of))
    return range(k * of, hi, of)


def _zero_runs(lengths):
    """(start, length) of every maximal run of zero-length contigs"""
    runs, i = [], 0
    while i < len(lengths):
        if lengths[i] == 0:
            j = i
            while j < len(lengths) and lengths[j] == 0:
                j += 1
            runs.append((i, j - i))
            i = j
        else:
            i += 1
    return runs


def claim_holds(case, claim):
    kind = claim["kind"]
    lengths = [len(s) for s in case.contigs]
    W = len(case.walks)
    if kind == "walks_more_than":
        return W > claim["n"]
    if kind == "walks_exactly":
        return W == claim["n"]
    if kind == "zero_length_contig":
        return 0 in lengths
    if kind == "zero_length_read_walked":
        return any(len(case.reads[u >> 1]) == 0 for w in case.walks for u in w)
    if kind == "zero_contig_run":
        for start, n in _zero_runs(lengths):
            if n < claim["n"]:
                continue
            before, after = any(lengths[:start]), any(lengths[start + n:])
            where = claim["where"]
            if (where == "first" and start == 0 and after) or (where == "between" and before and after) or \
                    (where == "last" and start + n == W and before):
                return True
        return False
    if kind == "zero_piece_run":
        edges = {(u, v): i for i, (u, v) in enumerate(zip(case.src, case.dst))}
        for w, p in zip(case.walks, case.pieces):
            k = claim["n"]
            if len(p) <= k or any(p[:k]) or not any(p):
                continue
            pre = [case.prefix[edges[(a, b)]] for a, b in zip(w[:k], w[1:k + 1])]
            rl = [len(case.reads[a >> 1]) for a in w[:k]]
            if claim["how"] == "prefix0" and all(x == 0 for x in pre) and all(rl):
                return True
            if claim["how"] == "negative" and all(x < -n for x, n in zip(pre, rl)) and all(rl):
                return True
        return False
    if kind == "contig_lengths_include":
        return set(claim["lengths"]) <= set(lengths)
    if kind == "width_exceeds_every_contig":
        return claim["lw"] > max(lengths)
    if kind == "every_byte_value":
        want = set(range(1, 256)) - {10}
        seen = set()
        for w, p in zip(case.walks, case.pieces):
            for u, s in zip(w, p):
                if u % 2 == claim["parity"]:
                    r = case.reads[u >> 1]
                    seen |= set(r[:len(s)] if u % 2 == 0 else r[len(r) - len(s):])
        return seen == want
    lay = case.layout(claim["lw"])
    img, total = lay.image, len(lay.image)
    bodies = [(w, bo, bl) for w, (bo, bl) in enumerate(zip(lay.body_off, lay.body_len))]
    if kind == "chunk_with_contig_starts":
        count = {}
        for w, bo, bl in bodies:
            if bl:
                count[bo // CHUNK] = count.get(bo // CHUNK, 0) + 1
        return max(count.values(), default=0) >= claim["n"]
    if kind == "tile_without_body_byte":
        covered = set()
        for w, bo, bl in bodies:
            if bl:
                covered |= set(range(bo // TILE, (bo + bl - 1) // TILE + 1))
        return any(t not in covered for t in range(total // TILE))       # whole tiles only
    if kind == "tile_inside_one_piece":
        po = case.piece_off()
        cst = np.concatenate([[0], np.cumsum(lengths)])
        for w, bo, bl in bodies:
            for t0 in _multiples(TILE, bo, bo + bl - TILE + 1):
                first, last = t0, t0 + TILE - 1
                while img[first] == 10:
                    first += 1
                while img[last] == 10:
                    last -= 1
                a = bisect.bisect_right(po, int(cst[w]) + lay.unwrapped(w, first)) - 1
                b = bisect.bisect_right(po, int(cst[w]) + lay.unwrapped(w, last)) - 1
                if a == b:
                    return True
        return False
    if kind == "newline_at_multiple":       # a newline of a BODY, not of a header line
        return any(img[o] == 10 and bo <= o for w, bo, bl in bodies if bl for o in _multiples(claim["of"], bo, bo + bl))
    if kind == "last_data_byte_at":
        for w, bo, bl in bodies:
            if bl:
                last = bo + bl - 1 - (1 if claim["lw"] > 0 else 0)
                assert img[last] != 10
                if last - claim["plus"] >= claim["of"] and (last - claim["plus"]) % claim["of"] == 0:
                    return True
        return False
    if kind == "header_straddles":
        return any(any(True for _ in _multiples(claim["of"], ro + 1, bo)) for ro, bo in zip(lay.rec_off, lay.body_off))
    if kind == "body_starts_at_multiple":
        return any(bl and bo >= claim["of"] and bo % claim["of"] == 0 for w, bo, bl in bodies)
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------- builders

_LETTERS = np.frombuffer(b"ACGTNacgtnRYKMSWrykmsw", dtype=np.uint8)


def _random_read(rng, n):
    return rng.choice(_LETTERS, size=n).tobytes()


def tiny_many(W):
    """Reads of 0-3 bytes, every prefix form of Python's slice rule, W short walks: many contigs inside one 16-byte chunk,
    zero-length reads, pieces and contigs, and W on either side of one and two rounds of the 64-lane search."""
    rng = np.random.default_rng(W)
    R = 300
    lens = [int(x) for x in rng.integers(0, 4, size=R)]
    reads = [_random_read(rng, n) for n in lens]
    N = 2 * R
    src, dst, prefix = [], [], []
    succ = [[] for _ in range(N)]
    for u in range(N):
        n = lens[u >> 1]
        for _ in range(2):
            v = int(rng.integers(N))
            src.append(u), dst.append(v), succ[u].append(v)
            prefix.append([0, 1, 2, -1, -n, -n - 1, n, n + 1][int(rng.integers(8))])
    for i in range(0, 120, 3):                      # parallel pairs: the last id of a pair decides
        src.append(src[i]), dst.append(dst[i]), prefix.append([2, 0, -1, 1][i % 4])
    walks = []
    for k in range(W):
        u = (int(rng.integers(R)) << 1) | (k & 1)   # even and odd starts
        w = [u]
        for _ in range(int(rng.integers(0, 4))):    # 1-4 nodes
            w.append(succ[w[-1]][int(rng.integers(2))])
        walks.append(w)
    short = [r for r in range(R) if lens[r] in (1, 2)]
    for k in range(8):                              # eight contigs of 1-2 bytes in a row: at least five starts in one chunk
        walks[8 + k] = [2 * short[k] + (k & 1)]
    claims = [{"kind": "chunk_with_contig_starts", "lw": 0, "n": 5}, {"kind": "zero_length_contig"}, {"kind": "zero_length_read_walked"},
              {"kind": "contig_lengths_include", "lengths": [0, 1, 2, 3]}]
    claims.append({"kind": "walks_exactly", "n": WAVE} if W == WAVE else {"kind": "walks_more_than", "n": WAVE})
    if W > WAVE * WAVE:
        claims.append({"kind": "walks_more_than", "n": WAVE * WAVE})
    return reads, src, dst, prefix, walks, (0, 1, 2, 60), claims


def zero_runs():
    """Walks whose first 70-odd steps contribute nothing (prefix 0; a negative prefix beyond the read), and blocks of 70 and more
    walks that spell the empty string - first, between non-empty contigs and as the very last ones; one block is long enough that
    a whole tile of the FASTA image holds header lines only."""
    rng = np.random.default_rng(11)
    Z, R = 10, 160
    reads = [b""] * Z + [_random_read(rng, int(n)) for n in rng.integers(20, 121, size=R - Z)]
    src, dst, prefix = [], [], []

    def edge(u, v, p):
        src.append(u), dst.append(v), prefix.append(p)

    chain_a = [2 * r + (r & 1) for r in range(10, 85)]          # 75 nodes, both parities
    for i, (u, v) in enumerate(zip(chain_a[:-1], chain_a[1:])):
        edge(u, v, 0 if i < 72 else (5, 7)[i - 72])
    chain_b = [2 * r + ((r + 1) & 1) for r in range(85, 160)]
    for i, (u, v) in enumerate(zip(chain_b[:-1], chain_b[1:])):
        edge(u, v, -len(reads[u >> 1]) - 1 - (i % 3) if i < 73 else -3)
    empties = [[u] for u in range(2 * Z)]                       # a zero-length read, either strand
    for z in range(Z):
        x = 2 * (20 + z) + (z & 1)
        edge(x, 2 * z, 0)                                       # a read cut to nothing, then a zero-length read
        empties.append([x, 2 * z])
        edge(2 * z + 1, (2 * z + 2) % (2 * Z), 5 if z & 1 else -2)   # any prefix of a zero-length read is empty
        empties.append([2 * z + 1, (2 * z + 2) % (2 * Z)])
    edge(41, 42, 9), edge(42, 45, -4)                           # pairs that neither chain uses

    def block(n):
        return [list(empties[k % len(empties)]) for k in range(n)]

    walks = (block(70) + [chain_a, [30], [41, 42, 45]] + block(2000) + [chain_b, [51]] + block(WAVE) + [[41, 42]] + block(75))
    claims = [{"kind": "zero_contig_run", "n": 70, "where": "first"}, {"kind": "zero_contig_run", "n": 70, "where": "between"},
              {"kind": "zero_contig_run", "n": 70, "where": "last"}, {"kind": "zero_piece_run", "n": 70, "how": "prefix0"},
              {"kind": "zero_piece_run", "n": 70, "how": "negative"}, {"kind": "tile_without_body_byte", "lw": 60},
              {"kind": "walks_more_than", "n": WAVE}, {"kind": "zero_length_read_walked"}]
    return reads, src, dst, prefix, walks, (0, 60), claims


BORDER_PLACEMENTS = {
    "last_byte_before_tile": {"kind": "last_data_byte_at", "of": TILE, "plus": -1},
    "last_byte_at_tile": {"kind": "last_data_byte_at", "of": TILE, "plus": 0},
    "last_byte_after_tile": {"kind": "last_data_byte_at", "of": TILE, "plus": 1},
    "newline_at_tile": {"kind": "newline_at_multiple", "of": TILE},
    "newline_at_chunk": {"kind": "newline_at_multiple", "of": CHUNK},
    "header_straddles_tile": {"kind": "header_straddles", "of": TILE},
    "body_starts_at_tile": {"kind": "body_starts_at_multiple", "of": TILE},
}
BORDER_CASES = [(p, lw) for p in ("last_byte_before_tile", "last_byte_at_tile", "last_byte_after_tile", "body_starts_at_tile") for lw in (0, 60)] \
    + [(p, 60) for p in ("newline_at_tile", "newline_at_chunk", "header_straddles_tile")]
BORDER_TRIES = 400


def _anchors(lay, claim):
    """the offsets (of contigs after the first) that the placement wants at a multiple of claim["of"]"""
    later = range(1, len(lay.n))
    if claim["kind"] == "last_data_byte_at":
        return [lay.body_off[w] + lay.body_len[w] - 1 - (1 if lay.lw > 0 else 0) - claim["plus"] for w in later if lay.body_len[w]]
    if claim["kind"] == "body_starts_at_multiple":
        return [lay.body_off[w] for w in later if lay.body_len[w]]
    if claim["kind"] == "header_straddles":
        return [lay.rec_off[w] + 1 for w in later]
    return [lay.body_off[w] + lay.lw for w in later if lay.body_len[w] > lay.lw]      # the first newline of a body


def border_placement(placement, lw):
    """Reads of a few thousand bases; the length of read 0 (contig 0 is that read alone, so every later byte moves with it) is
    searched until the placement holds in the layout `lw`: from the length at which the nearest candidate offset is about to reach
    its multiple (a byte more in read 0 moves a later offset by one byte, and by one more per 60 at line width 60), one byte at a
    time, for at most BORDER_TRIES lengths.  Raises when they do not reach it."""
    claim = dict(BORDER_PLACEMENTS[placement], lw=lw)
    rng = np.random.default_rng(23)
    first = _random_read(rng, 2000 + TILE // 4 + BORDER_TRIES)
    rest = [_random_read(rng, int(n)) for n in rng.integers(2500, 3501, size=11)]
    src = [3, 2, 7, 9, 12, 15]
    dst = [4, 7, 8, 10, 15, 16]
    prefix = [-100, 1700, 4000, 2222, -3000, 1]
    walks = [[0], [3, 4], [5], [2, 7, 8], [6], [9, 10], [13], [12, 15, 16], [17], [19], [20], [23], [22], [11]]

    def build(t):
        return [first[:2000 + t]] + rest, src, dst, prefix, walks, (lw,), [claim]

    name = f"border-{placement}-lw{lw}"
    away = min((-a) % claim["of"] for a in _anchors(Case(name, build(0)).layout(lw), claim))
    start = min(max(away - away // 50 - 20, 0), TILE // 4)
    for t in range(start, start + BORDER_TRIES):
        if claim_holds(Case(name, build(t)), claim):
            return build(t)
    raise AssertionError(f"border placement {placement} at line width {lw}: not reached in {BORDER_TRIES} tries from {2000 + start}")


LONG_READ = 3 * TILE + 5


def long_piece():
    """One read of 3 tiles + 5 bytes as a whole contig on its even and on its odd node: whole tiles inside one piece, in every
    layout from 15 columns to one wider than the read.  A third walk puts a piece border three bytes behind a tile border."""
    rng = np.random.default_rng(31)
    reads = [_random_read(rng, LONG_READ)]
    lws = (0, 15, 16, 17, 60, TILE - 1, LONG_READ + 10)
    claims = [{"kind": "tile_inside_one_piece", "lw": lw} for lw in lws] + [{"kind": "width_exceeds_every_contig", "lw": 3 * LONG_READ}]
    return reads, [0], [1], [TILE + 3], [[0], [1], [0, 1]], lws + (3 * LONG_READ,), claims


WIDTH_EDGES = (1, 15, 16, 17, 31, 60)


def width_edges():
    """Contigs of lw - 1, lw, lw + 1, 2 lw and 2 lw + 1 bytes for every line width, on alternating strands."""
    rng = np.random.default_rng(41)
    lengths = sorted({n for lw in WIDTH_EDGES for n in (lw - 1, lw, lw + 1, 2 * lw, 2 * lw + 1)})
    reads = [_random_read(rng, n) for n in lengths]
    walks = [[2 * i + (i & 1)] for i in range(len(lengths))]
    claims = [{"kind": "contig_lengths_include", "lengths": [lw - 1, lw, lw + 1, 2 * lw, 2 * lw + 1]} for lw in WIDTH_EDGES]
    return reads, [], [], [], walks, (0,) + WIDTH_EDGES, claims


def alphabet():
    """Reads that hold every byte value but 0 and '\\n': all 17 IUPAC pairs in both cases and every byte the table leaves alone,
    walked on both strands."""
    rng = np.random.default_rng(51)
    values = np.array([b for b in range(1, 256) if b != 10], dtype=np.uint8)
    reads = [rng.permutation(values).tobytes() for _ in range(4)]
    src = [0, 1, 2, 3, 5, 7]
    dst = [2, 3, 5, 0, 6, 1]
    prefix = [100, 200, -54, 255, 17, 33]
    walks = [[0, 2, 5, 6], [1, 3, 0], [7, 1], [4], [7]]
    claims = [{"kind": "every_byte_value", "parity": 0}, {"kind": "every_byte_value", "parity": 1}]
    return reads, src, dst, prefix, walks, (0, 60), claims


BUILDERS = {"tiny-many-64": lambda: tiny_many(WAVE), "tiny-many-65": lambda: tiny_many(WAVE + 1),
            "tiny-many-4097": lambda: tiny_many(WAVE * WAVE + 1), "zero-runs": zero_runs, "long-piece": long_piece,
            "width-edges": width_edges, "alphabet": alphabet}
for _p, _lw in BORDER_CASES:
    BUILDERS[f"border-{_p}-lw{_lw}"] = functools.partial(border_placement, _p, _lw)


@functools.lru_cache(maxsize=None)
def case(name):
    """The built case (shared by every test of a session: building is a search for some)."""
    return Case(name, BUILDERS[name]())


# ---------------------------------------------------------------------------------------------- inputs of the check kernel

def unit_graph(R=1000):
    """R reads of one byte; every node u has the edges u -> u + 2 (prefix 1: one byte) and u -> u + 3 (prefix 0: nothing), mod 2R.
    No other pair is an edge: (u, u + 5) is the non-edge the tests plant."""
    rng = np.random.default_rng(61)
    reads = [_random_read(rng, 1) for _ in range(R)]
    N = 2 * R
    u = np.arange(N)
    src = np.concatenate([u, u]).tolist()
    dst = np.concatenate([(u + 2) % N, (u + 3) % N]).tolist()
    prefix = [1] * N + [0] * N
    return reads, src, dst, prefix


def unit_walks(W, N, two_node=lambda i: i % 2 == 1):
    """(int32 nodes, int64 offsets) of W valid walks over unit_graph: walk i starts at node 7 i mod N and, where two_node(i),
    goes on over the edge + 2 (i % 4 == 1) or + 3."""
    i = np.arange(W, dtype=np.int64)
    two = two_node(i)
    first = (7 * i) % N
    second = (first + np.where(i % 4 == 1, 2, 3)) % N
    off = np.zeros(W + 1, dtype=np.int64)
    np.cumsum(1 + two.astype(np.int64), out=off[1:])
    nodes = np.zeros(int(off[-1]), dtype=np.int32)
    nodes[off[:-1]] = first
    nodes[off[:-1][two] + 1] = second[two]
    return nodes, off


def split_walks(nodes, off):
    flat = nodes.tolist()
    return [flat[a:b] for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
