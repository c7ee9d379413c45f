"""From reads to the overlap graph on the MI355X: the step the reference leaves to hifiasm / raven (graph_dataset.py:76-186).

    sk = sketch_reads(reads, k=19, w=10)                 # MinimizerSketch: the (k, w) minimizers of every read, by (read, pos)
    ov = find_overlaps(reads, sk)                        # Overlaps: one per read pair and relative strand that chains enough seeds
    g = overlap_graph(reads)                             # read_gfa's dict: src, dst, num_nodes, overlap_length, prefix_length, ...

`reads`: a contigs.ReadStore, a (uint8 data, int64 off) pair as overlap.pack_reads returns it, or a list of sequences.  The statement -
hash, minimizer rule, pair records, bands, classification, every output order - is in include/gnnome_hip.h and, executable, in
tests/overlap_graph_statement.py; the kernels are csrc/overlap_graph.hip.  torch does the plumbing between them: the
stable sort of the seeds by hash, the sort of the pair records, the starts of the (a, b, rel) groups, the compaction of the kept overlaps
and gfa.assemble_edges.  The graph is the raw dovetail graph unless overlap_graph(simplify=) hands it to simplify.simplify_graph
(transitive edges, tips, with bubbles= the simple bubbles, the reads left without an edge) and overlap_graph(unitigs=) to
unitigs.compact_unitigs; a read set
whose seed pairs do not fit the device at once is refused (ValueError naming max_occ and max_pairs), not processed in blocks."""
import ctypes

import torch

from . import _lib
from .contigs import ReadStore
from .gfa import assemble_edges
from .ops import _on, _ptr, _stream
from .overlap import overlap_similarity, pack_reads

FIELDS = ("a", "b", "rel", "kind", "d_beg", "d_end", "n_seeds", "span_beg", "span_end", "overlap_length")
MAX_HALO = 256           # k + w - 1 may not exceed it (the LDS image of a sketch tile)
_RECORD_BYTES = 64       # device bytes one seed pair costs while it is sorted: two int64 keys, their sorted copies, the sorts' indices
_DIAG_BIAS = 1 << 30


class MinimizerSketch:
    """hash uint64[M], read int32[M], pos int32[M], strand uint8[M] ordered by (read, pos), off int64[R+1]: read r's minimizers are the
    slice off[r]:off[r+1].  All on the device."""

    def __init__(self, k, w, hash, read, pos, strand, off):   # noqa: A002
        self.k, self.w, self.hash, self.read, self.pos, self.strand, self.off = k, w, hash, read, pos, strand, off

    def __len__(self):
        return int(self.hash.numel())


class Overlaps:
    """The kept overlaps (kinds 1 .. 4), ordered by (a, b, rel); int32 device tensors a < b (reads), rel (1: b reverse-complemented),
    kind (1: b contained, 2: a contained, 3: a -> b', 4: b' -> a), d_beg, d_end, n_seeds, span_beg, span_end, overlap_length (kinds 3
    and 4), and contained bool[R].  records: (key_ab, key_dp), the sorted seed-pair records; record_fields() unpacks them."""

    def __init__(self, table, contained, records, sketch, num_reads):
        for i, f in enumerate(FIELDS):
            setattr(self, f, table[i])
        self.contained, self.records, self.sketch, self.num_reads = contained, records, sketch, num_reads

    def __len__(self):
        return int(self.a.numel())

    def record_fields(self):
        """int64[P, 5]: the records (a, b, rel, d, pa) in sorted order."""
        ab, dp = self.records
        return torch.stack([ab >> 32, (ab & 0xFFFFFFFF) >> 1, ab & 1, (dp >> 32) - _DIAG_BIAS, dp & 0xFFFFFFFF], 1)


class _Stages:
    """Device-event times of a call's stages into `stats` (a dict: "<stage>_ms", one synchronise at the end); stats=None records nothing."""

    def __init__(self, stats, device):
        self.stats, self.device, self.marks = stats, device, []
        self.mark("start")

    def mark(self, name):
        """The stage `name` ends here."""
        if self.stats is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(self.device))
            self.marks.append((name, ev))

    def finish(self):
        if self.stats is not None:
            self.marks[-1][1].synchronize()
            for (_, a), (name, b) in zip(self.marks, self.marks[1:]):
                self.stats[name + "_ms"] = a.elapsed_time(b)


def sketch_tile_size():
    """Windows per workgroup of the sketch kernel; results do not depend on it, the tests place their edges by it."""
    tile = ctypes.c_int(0)
    _lib.check(_lib.load().gnnome_sketch_tile_size(ctypes.byref(tile)), "sketch_tile_size")
    return int(tile.value)


def _packed(reads, device):
    """-> (uint8 data, int64 off) on the device."""
    if isinstance(reads, ReadStore):
        if reads.missing is not None and bool(reads.missing.any()):
            raise ValueError("the ReadStore leaves reads out (keep=): an overlapper needs every read")
        data, off = reads.data, reads.off
    elif isinstance(reads, tuple):
        data, off = reads
    else:
        data, off = pack_reads(reads)
    device = torch.device(device) if device is not None else (data.device if data.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    data, off = data.to(device).contiguous(), off.to(device, torch.int64).contiguous()
    if off.numel() - 1 >= (1 << 30) or (off.numel() > 1 and int((off[1:] - off[:-1]).max()) >= (1 << 30)):
        raise ValueError("the overlapper takes fewer than 2^30 reads, each shorter than 2^30 bases")
    return data, off


def _check_kw(k, w):
    if not (1 <= int(k) <= 31 and int(w) >= 1 and int(k) + int(w) - 1 <= MAX_HALO):
        raise ValueError(f"k={k} w={w}: need 1 <= k <= 31, w >= 1 and k + w - 1 <= {MAX_HALO}")


def sketch_reads(reads, k=19, w=10, device=None, stats=None):
    """-> MinimizerSketch (gnnome_sketch_reads: a count launch, a scan, a write launch; one synchronisation for the size).  stats: a dict
    that receives the device-event times tiles_ms (the tile table), count_ms (count launch, scan, the size read back) and write_ms (the
    write launch)."""
    _check_kw(k, w)
    lib = _lib.load()
    data, off = _packed(reads, device)
    dev = data.device
    stages = _Stages(stats, dev)
    R, T = int(off.numel()) - 1, sketch_tile_size()
    windows = (off[1:] - off[:-1] - (k + w - 2)).clamp(min=0)
    tile_first = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    torch.cumsum((windows + T - 1) // T, 0, out=tile_first[1:])
    tiles = int(tile_first[-1]) if R else 0
    need = ctypes.c_size_t(0)
    _lib.check(lib.gnnome_sketch_workspace_bytes(tiles, ctypes.byref(need)), "sketch_workspace_bytes")
    ws = torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=dev)
    result = (ctypes.c_int64 * 1)()
    args = (_ptr(data), _ptr(off), R, int(k), int(w), _ptr(tile_first), tiles)
    stages.mark("tiles")
    with _on(dev):
        _lib.check(lib.gnnome_sketch_reads(*args, None, None, None, None, 0, result, _ptr(ws), ws.numel(), _stream(dev)), "sketch_reads")
        M = int(result[0])
        stages.mark("count")
        hash_ = torch.empty(M, dtype=torch.uint64, device=dev)
        read, pos = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
        strand = torch.empty(M, dtype=torch.uint8, device=dev)
        if M:
            _lib.check(lib.gnnome_sketch_reads(*args, _ptr(hash_), _ptr(read), _ptr(pos), _ptr(strand), M, result, _ptr(ws), ws.numel(),
                                               _stream(dev)), "sketch_reads")
        stages.mark("write")
    stages.finish()
    tile_base = ws[:8 * (tiles + 1)].view(torch.int64) if tiles else torch.zeros(1, dtype=torch.int64, device=dev)
    return MinimizerSketch(int(k), int(w), hash_, read, pos, strand, tile_base[tile_first])


def _default_max_pairs(device):
    return torch.cuda.mem_get_info(device)[0] // _RECORD_BYTES


def find_overlaps(reads, sk=None, k=19, w=10, max_occ=64, band=500, min_seeds=3, min_overlap=1000, max_hang=1000, max_pairs=None,
                  device=None, stats=None):
    """-> Overlaps.  sk: a MinimizerSketch of these reads (its k and w are used; one of another read count is refused), or None to sketch
    them here.  max_pairs: the most seed pairs to hold at once (default: what the free device memory takes while they are sorted); the
    exact count is known before any record is written, and a count above it raises ValueError.  stats: a dict that receives the
    device-event times of the stages: seed_sort_ms (torch), pairs_count_ms (count kernel, scan, the size read back), pairs_write_ms (the
    record kernel), record_sort_ms (torch: two stable sorts and the gathers), group_starts_ms (torch), chain_ms (the chain kernel),
    compaction_ms (torch)."""
    lib = _lib.load()
    data, off = _packed(reads, device)
    dev = data.device
    if sk is None:
        sk = sketch_reads((data, off), k, w, dev)
    k, R, M = sk.k, int(off.numel()) - 1, len(sk)
    if int(sk.off.numel()) != R + 1 or sk.hash.device != dev:
        raise ValueError(f"the sketch is of {int(sk.off.numel()) - 1} reads on {sk.hash.device}, the reads are {R} on {dev}")
    stages = _Stages(stats, dev)
    if not (1 <= int(max_occ) <= (1 << 20)) or band < 0 or min_seeds < 1 or min_overlap < 0 or max_hang < 0:
        raise ValueError(f"max_occ={max_occ} band={band} min_seeds={min_seeds} min_overlap={min_overlap} max_hang={max_hang}: out of range")
    # plumbing: the stable sort by hash (hashes are below 2^62: they order alike as int64)
    order = torch.sort(sk.hash.view(torch.int64), stable=True).indices
    hs, rs, ps, ss = (t[order].contiguous() for t in (sk.hash.view(torch.int64), sk.read, sk.pos, sk.strand))
    need = ctypes.c_size_t(0)
    _lib.check(lib.gnnome_seed_pairs_workspace_bytes(M, ctypes.byref(need)), "seed_pairs_workspace_bytes")
    ws = torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=dev)
    result = (ctypes.c_int64 * 1)()
    args = (_ptr(hs), _ptr(rs), _ptr(ps), _ptr(ss), M, _ptr(off), R, k, int(max_occ))
    limit = int(max_pairs) if max_pairs is not None else _default_max_pairs(dev)
    stages.mark("seed_sort")
    with _on(dev):
        _lib.check(lib.gnnome_seed_pairs(*args, None, None, 0, result, _ptr(ws), ws.numel(), _stream(dev)), "seed_pairs")
        P = int(result[0])
        stages.mark("pairs_count")
        if P > limit:
            raise ValueError(f"{P} seed pairs exceed max_pairs={limit}: lower max_occ (now {max_occ}) so that repeated k-mers are dropped, "
                             f"or raise max_pairs if the device has the memory ({_RECORD_BYTES} bytes per pair)")
        key_ab, key_dp = torch.empty(P, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
        if P:
            _lib.check(lib.gnnome_seed_pairs(*args, _ptr(key_ab), _ptr(key_dp), P, result, _ptr(ws), ws.numel(), _stream(dev)), "seed_pairs")
    stages.mark("pairs_write")
    del ws
    # plumbing: the records in (a, b, rel, d, pa) order, and where every (a, b, rel) group starts
    by = torch.sort(key_dp, stable=True).indices
    by = by[torch.sort(key_ab[by], stable=True).indices]
    key_ab, key_dp = key_ab[by].contiguous(), key_dp[by].contiguous()
    del by
    stages.mark("record_sort")
    head = torch.ones(P, dtype=torch.bool, device=dev)
    if P:
        head[1:] = key_ab[1:] != key_ab[:-1]
    start = torch.nonzero(head).squeeze(1)
    G = int(start.numel())
    group_start = torch.cat([start, start.new_tensor([P])])
    out = torch.empty(len(FIELDS), G, dtype=torch.int32, device=dev)
    stages.mark("group_starts")
    if G:
        with _on(dev):
            _lib.check(lib.gnnome_chain_overlaps(_ptr(key_ab), _ptr(key_dp), P, _ptr(group_start), G, _ptr(off), R, k, int(band), int(min_seeds),
                                                 int(min_overlap), int(max_hang), _ptr(out), _stream(dev)), "chain_overlaps")
    stages.mark("chain")
    kind = out[3]
    table = out[:, (kind >= 1) & (kind <= 4)].contiguous()
    contained = torch.zeros(R, dtype=torch.bool, device=dev)
    contained[table[1][table[3] == 1].long()] = True
    contained[table[0][table[3] == 2].long()] = True
    stages.mark("compaction")
    stages.finish()
    if stats is not None:
        stats.update(seeds=M, pairs=P, groups=G)
    return Overlaps(table, contained, (key_ab, key_dp), sk, R)


def overlap_graph(reads, sk=None, k=19, w=10, max_occ=64, band=500, min_seeds=3, min_overlap=1000, max_hang=1000, max_pairs=None,
                  similarity=True, drop_contained=True, annotations=None, device=None, long_overlaps=False, simplify=None, unitigs=False):
    """-> the dict gfa.read_gfa_device returns (src, dst, num_nodes = 2R, overlap_length, prefix_length, read_length, overlap_similarity or
    None, reads = the packed reads; the name tables are None), tensors on the device, plus `contained` bool[R] and `overlaps`.  Node 2r
    is read r, 2r + 1 its reverse complement; overlap j gives the events 2j (its real edge) and 2j + 1 (the mate (v ^ 1, u ^ 1)) to
    gfa.assemble_edges.  similarity: overlap.overlap_similarity on every edge (long_overlaps is handed to it).  drop_contained: contained
    reads keep their node numbers and lose their edges.  annotations: (read_strand, read_start, read_end, read_chr), int64[2R] as
    reads.node_annotations_device gives them - the dict then carries them and labels.process_graph(g) works on it.  simplify: True, or a
    dict of simplify.simplify_graph's keywords (fuzz, max_tip, tips, bubbles, compact, check_mates, stats) - the graph is handed through it before
    it is returned (transitive edges and tips dropped; with compact the reads left without an edge removed, `kept_reads` naming the
    others); None, the default, returns the raw dovetail graph.  unitigs: True, or a dict of unitigs.compact_unitigs' keywords (stats) -
    after `simplify`, the graph's non-branching paths are merged and the unitig graph is returned in its place (its `reads` are the
    unitig sequences, its name tables read_gfa's unitig form; `contained`, `overlaps` and the read_* columns are not carried); False,
    the default, changes nothing."""
    if simplify is not None and simplify is not True and not isinstance(simplify, dict):
        raise ValueError(f"simplify={simplify!r}: expected None, True or a dict of simplify_graph's keywords")
    if unitigs is not False and unitigs is not True and not isinstance(unitigs, dict):
        raise ValueError(f"unitigs={unitigs!r}: expected False, True or a dict of compact_unitigs' keywords")
    data, off = _packed(reads, device)
    dev = data.device
    ov = find_overlaps((data, off), sk, k, w, max_occ, band, min_seeds, min_overlap, max_hang, max_pairs, dev)
    R = ov.num_reads
    keep = ov.kind >= 3
    if drop_contained:
        keep &= ~(ov.contained[ov.a.long()] | ov.contained[ov.b.long()])
    a, b, rel, ol = (t[keep].long() for t in (ov.a, ov.b, ov.rel, ov.overlap_length))
    forward = ov.kind[keep] == 3
    u, v = torch.where(forward, 2 * a, 2 * b + rel), torch.where(forward, 2 * b + rel, 2 * a)
    ev_u, ev_v = torch.stack([u, v ^ 1], 1).reshape(-1), torch.stack([v, u ^ 1], 1).reshape(-1)
    src, dst, ol, _ = assemble_edges(ev_u, ev_v, torch.repeat_interleave(ol, 2), torch.arange(ev_u.numel(), device=dev) >> 1, 2 * R)
    read_length = torch.repeat_interleave(off[1:] - off[:-1], 2)
    g = {"src": src, "dst": dst, "num_nodes": 2 * R, "overlap_length": ol, "prefix_length": read_length[src] - ol, "read_length": read_length,
         "read_to_node": None, "node_to_read": None, "read_to_node2": None, "read_seqs": None, "overlap_similarity": None,
         "reads": (data, off), "contained": ov.contained, "overlaps": ov}
    if similarity:
        g["overlap_similarity"] = overlap_similarity((data, off), src, dst, ol, dev, long_overlaps=long_overlaps)
    if annotations is not None:
        cols = [torch.as_tensor(c).reshape(-1).to(torch.int64) for c in annotations]
        if len(cols) != 4 or any(c.numel() != 2 * R for c in cols):
            raise ValueError(f"annotations: expected read_strand, read_start, read_end, read_chr with {2 * R} entries each")
        g.update(zip(("read_strand", "read_start", "read_end", "read_chr"), cols))
    if simplify is not None:
        from .simplify import simplify_graph
        g = simplify_graph(g, device=dev, **(simplify if isinstance(simplify, dict) else {}))
    if unitigs is not False:
        from .unitigs import compact_unitigs
        g = compact_unitigs(g, device=dev, **(unitigs if isinstance(unitigs, dict) else {}))
    return g
