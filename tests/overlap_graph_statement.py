"""The overlap graph from reads, restated stage by stage in NumPy / plain Python (no GPU, no torch): what gnnome_amd.overlapper and
csrc/overlap_graph.hip must reproduce bit for bit.  Integers only; every output order is part of the statement.

Sketch.  Bases ACGT in either case are 0..3; any other byte makes every k-mer over it invalid; k <= 31.  A k-mer's code is the smaller
of its forward (first base most significant) and reverse-complement 2k-bit codes, strand = 1 where that is the reverse complement;
equal codes (palindromes) are invalid.  The hash is Thomas Wang's 64-bit integer mix with every step masked to m = 2^(2k) - 1 (`mix`),
a bijection of [0, m].  Position p is a minimizer when some window of w consecutive k-mer starts inside the read has its smallest
valid hash at p, ties to the leftmost; each position once, output by (read, pos); reads shorter than k + w - 1 give nothing.

Pairs.  Seeds sorted stably by hash; a hash with more than max_occ seeds is dropped; every other bucket gives each pair of its seeds in
different reads, a < b the reads: rel = strand_a ^ strand_b, pb' = pb if rel == 0 else len_b - k - pb, d = pa - pb'; the records
(a, b, rel, d, pa) sorted by that tuple.

Chains.  Within one (a, b, rel), in order: a band starts at a record and takes every following record whose d is at most `band` above
the band's first d; per band n_seeds, span_beg = min pa, span_end = max pa + k, d_beg = d at the smallest pa (ties: smallest d), d_end
= d at the largest pa (ties: largest d); the group's overlap is the band with the most seeds (ties: the first), kept if n_seeds >=
min_seeds.  Classification: `classify`.  Graph: `graph`."""
import numpy as np

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
FIELDS = ("a", "b", "rel", "kind", "d_beg", "d_end", "n_seeds", "span_beg", "span_end", "overlap_length")


def mix(x, k):
    """The hash of the code(s) x (uint64 array) on 2k bits."""
    u = np.uint64
    m = u((1 << (2 * k)) - 1)
    x = x.astype(np.uint64)
    x = (~x + (x << u(21))) & m
    x = x ^ (x >> u(24))
    x = (x + (x << u(3)) + (x << u(8))) & m
    x = x ^ (x >> u(14))
    x = (x + (x << u(2)) + (x << u(4))) & m
    x = x ^ (x >> u(28))
    x = (x + (x << u(31))) & m
    return x


def as_bytes(reads):
    return [np.frombuffer(r.encode("ascii") if isinstance(r, str) else bytes(r), dtype=np.uint8) for r in reads]


def kmer_hashes(seq, k):
    """(hash uint64[n], strand uint8[n]) of the n = len - k + 1 k-mers of one read; INVALID where the k-mer is."""
    u = np.uint64
    n = len(seq) - k + 1
    code = _CODE[seq]
    bad = code > 3
    c = np.where(bad, 0, code).astype(np.uint64)
    fwd, rev, inval = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool)
    for j in range(k):
        fwd = (fwd << u(2)) | c[j:j + n]
        rev = rev | ((u(3) - c[j:j + n]) << u(2 * j))
        inval |= bad[j:j + n]
    inval |= fwd == rev
    h = mix(np.minimum(fwd, rev), k)
    h[inval] = INVALID
    return h, (rev < fwd).astype(np.uint8)


def sketch(reads, k, w):
    """-> dict(hash uint64[M], read int32[M], pos int32[M], strand uint8[M], off int64[R+1]) ordered by (read, pos)."""
    assert 1 <= k <= 31 and w >= 1
    hs, rs, ps, ss, off = [], [], [], [], [0]
    with np.errstate(over="ignore"):
        for r, seq in enumerate(as_bytes(reads)):
            if len(seq) >= k + w - 1:
                h, strand = kmer_hashes(seq, k)
                nw = len(h) - w + 1
                best, arg = h[:nw].copy(), np.zeros(nw, dtype=np.int64)
                for j in range(1, w):
                    cand = h[j:j + nw]
                    less = cand < best          # strictly: ties stay with the leftmost
                    best, arg = np.where(less, cand, best), np.where(less, j, arg)
                pos = np.unique((np.arange(nw) + arg)[best != INVALID])
                hs.append(h[pos]); rs.append(np.full(len(pos), r)); ps.append(pos); ss.append(strand[pos])
            off.append(off[-1] + (len(ps[-1]) if len(seq) >= k + w - 1 else 0))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)   # noqa: E731
    return {"hash": cat(hs, np.uint64), "read": cat(rs, np.int32), "pos": cat(ps, np.int32), "strand": cat(ss, np.uint8),
            "off": np.array(off, dtype=np.int64)}


def pair_count(sk, max_occ):
    """The exact number of records, from the bucket sizes alone."""
    order = np.argsort(sk["hash"], kind="stable")
    h, rd = sk["hash"][order], sk["read"][order].astype(np.int64)
    _, start, size = np.unique(h, return_index=True, return_counts=True)
    total = 0
    for s, n in zip(start.tolist(), size.tolist()):
        if n <= max_occ:
            same = np.unique(rd[s:s + n], return_counts=True)[1]
            total += n * (n - 1) // 2 - int((same * (same - 1) // 2).sum())
    return total


def pairs(sk, lengths, k, max_occ):
    """-> int64[P, 5]: the records (a, b, rel, d, pa), sorted by that tuple."""
    order = np.argsort(sk["hash"], kind="stable")
    h, rd, ps, st = sk["hash"][order], sk["read"][order].tolist(), sk["pos"][order].tolist(), sk["strand"][order].tolist()
    _, start, size = np.unique(h, return_index=True, return_counts=True)
    rec = []
    for s, n in zip(start.tolist(), size.tolist()):
        if n > max_occ:
            continue
        for i in range(s, s + n):
            for j in range(i + 1, s + n):
                if rd[i] == rd[j]:
                    continue
                x, y = (i, j) if rd[i] < rd[j] else (j, i)
                rel = st[x] ^ st[y]
                pb = ps[y] if rel == 0 else lengths[rd[y]] - k - ps[y]
                rec.append((rd[x], rd[y], rel, ps[x] - pb, ps[x]))
    rec.sort()
    return np.array(rec, dtype=np.int64).reshape(-1, 5)


def chains(rec, k, band, min_seeds):
    """-> list of (a, b, rel, d_beg, d_end, n_seeds, span_beg, span_end), one per (a, b, rel) group whose best band has >= min_seeds
    seeds, in group order."""
    out, rows, i = [], rec.tolist(), 0
    while i < len(rows):
        j = i
        while j < len(rows) and rows[j][:3] == rows[i][:3]:
            j += 1
        best, s = None, i
        while s < j:
            e = s
            while e < j and rows[e][3] <= rows[s][3] + band:
                e += 1
            members = [(r[4], r[3]) for r in rows[s:e]]        # (pa, d)
            lo, hi = min(members), max(members)
            cand = (e - s, lo[0], hi[0] + k, lo[1], hi[1])
            if best is None or cand[0] > best[0]:
                best = cand
            s = e
        if best[0] >= min_seeds:
            out.append(tuple(rows[i][:3]) + (best[3], best[4], best[0], best[1], best[2]))
        i = j
    return out


def classify(chain, lengths, min_overlap, max_hang):
    """One chain -> (kind, overlap_length): 0 internal match, 1 b contained, 2 a contained, 3 a -> b', 4 b' -> a; a kind 3 or 4 with
    overlap_length < min_overlap is kind 6 (dropped)."""
    a, b, rel, d_beg, d_end, n, span_beg, span_end = chain
    la, lb = lengths[a], lengths[b]
    a_s, a_e = max(0, d_beg), min(la, lb + d_end)
    if span_beg - a_s > max_hang or a_e - span_end > max_hang:
        return 0, 0
    if d_beg >= 0 and lb + d_end <= la:
        return 1, 0
    if d_beg <= 0 and la <= lb + d_end:
        return 2, 0
    kind, ol = (3, min(la - d_beg, lb)) if d_beg > 0 else (4, min(lb + d_beg, la))
    return (kind, ol) if ol >= min_overlap else (6, ol)


def overlaps(reads, k=19, w=10, max_occ=64, band=500, min_seeds=3, min_overlap=1000, max_hang=1000, max_pairs=None):
    """-> dict: `sketch`, `records`, one int64 array per FIELDS entry over the kept overlaps (kinds 1..4, group order) and `contained`
    bool[R].  max_pairs: the exact record count above it raises ValueError before any record exists."""
    lengths = [len(s) for s in as_bytes(reads)]
    sk = sketch(reads, k, w)
    if max_pairs is not None and pair_count(sk, max_occ) > max_pairs:
        raise ValueError(f"{pair_count(sk, max_occ)} seed pairs exceed max_pairs={max_pairs}: lower max_occ or raise max_pairs")
    rec = pairs(sk, lengths, k, max_occ)
    rows, contained = [], np.zeros(len(lengths), dtype=bool)
    for ch in chains(rec, k, band, min_seeds):
        kind, ol = classify(ch, lengths, min_overlap, max_hang)
        if 1 <= kind <= 4:
            rows.append(ch[:3] + (kind,) + ch[3:] + (ol,))
            if kind == 1:
                contained[ch[1]] = True
            if kind == 2:
                contained[ch[0]] = True
    table = np.array(rows, dtype=np.int64).reshape(-1, len(FIELDS))
    out = {f: table[:, i] for i, f in enumerate(FIELDS)}
    out.update(sketch=sk, records=rec, contained=contained, lengths=np.array(lengths, dtype=np.int64))
    return out


def graph(ov, drop_contained=True):
    """The edges of the kept kind-3 / kind-4 overlaps -> dict(src, dst, overlap_length, prefix_length, read_length, num_nodes).  Node 2r is
    read r, 2r + 1 its reverse complement; overlap j gives the events 2j (its real edge) and 2j + 1 (the mate (v ^ 1, u ^ 1)); the edges
    come by source node, then by event.  drop_contained: overlaps with a contained read give no edge; node numbers stay."""
    events = []
    for a, b, rel, kind, ol in zip(*(ov[f].tolist() for f in ("a", "b", "rel", "kind", "overlap_length"))):
        if kind < 3 or (drop_contained and (ov["contained"][a] or ov["contained"][b])):
            continue
        u, v = (2 * a, 2 * b + rel) if kind == 3 else (2 * b + rel, 2 * a)
        events += [(u, v, ol), (v ^ 1, u ^ 1, ol)]
    order = sorted(range(len(events)), key=lambda e: (events[e][0], e))
    col = lambda i: np.array([events[e][i] for e in order], dtype=np.int64)   # noqa: E731
    read_length = np.repeat(ov["lengths"], 2)
    src, dst, ol = col(0), col(1), col(2)
    return {"src": src, "dst": dst, "overlap_length": ol, "prefix_length": read_length[src] - ol, "read_length": read_length,
            "num_nodes": 2 * len(ov["lengths"])}


# ---- the simulated read set the tests share --------------------------------------------------------------------------------------------

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def simulate(seed=10, genome_len=20000, n_reads=120, lo=300, hi=2500):
    """A random genome and error-free reads on both strands -> (genome bytes, reads list of bytes, strand +1 / -1, start, end)."""
    rng = np.random.default_rng(seed)
    genome = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, genome_len)])
    length = rng.integers(lo, hi + 1, n_reads)
    start = np.array([rng.integers(0, genome_len - int(n) + 1) for n in length])
    strand = np.where(rng.integers(0, 2, n_reads) == 1, 1, -1)
    reads = [genome[s:s + n] if t == 1 else revcomp(genome[s:s + n]) for s, n, t in zip(start.tolist(), length.tolist(), strand.tolist())]
    return genome, reads, strand.astype(np.int64), start.astype(np.int64), (start + length).astype(np.int64)


def canonical_kmers_unique(genome, k):
    """No k-mer of the genome equals another, or the reverse complement of another or of itself."""
    seen = set()
    for i in range(len(genome) - k + 1):
        km = genome[i:i + k]
        rc = revcomp(km)
        if km == rc or km in seen or rc in seen:
            return False
        seen.add(km)
    return True


def positional_truth(strand, start, end, min_overlap):
    """From the read positions alone: (edges {(u, v): overlap}, contained bool[R]).  Read j lies inside read i when its interval does
    (equal intervals: the later read is the contained one).  Two reads that overlap by >= min_overlap with neither inside the other give
    the edge from the one that starts first to the other, between the nodes that read the genome forwards, and its mate."""
    R = len(start)
    inside = lambda j, i: start[i] <= start[j] and end[j] <= end[i] and ((start[i], end[i]) != (start[j], end[j]) or i < j)   # noqa: E731
    contained = np.array([any(inside(j, i) for i in range(R) if i != j) for j in range(R)])
    fwd = [2 * r if strand[r] == 1 else 2 * r + 1 for r in range(R)]
    edges = {}
    for i in range(R):
        for j in range(R):
            ov = int(min(end[i], end[j]) - max(start[i], start[j]))
            if i != j and start[i] < start[j] and ov >= min_overlap and not inside(j, i) and not inside(i, j):
                edges[(fwd[i], fwd[j])] = ov
                edges[(fwd[j] ^ 1, fwd[i] ^ 1)] = ov
    return edges, contained
