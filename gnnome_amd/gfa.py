"""GFA -> the arrays the scoring path and the decoder need, without DGL / networkx / Biopython
(graph_parser.py:120-411, only_from_gfa).

    g = read_gfa("asm.bp.raw.r_utg.noseq.gfa")
    g["src"], g["dst"]                       edge list in the order DGL would number the edges (see below)
    g["overlap_length"], g["prefix_length"]  per edge;  g["read_length"] per node
    g["overlap_similarity"]                  per edge, or None (see below)
    views = gnnome_amd.graph.views_for((g["src"], g["dst"], g["num_nodes"]), device)
    x = features.degree_features(views);  e = features.edge_features(g["overlap_length"], g["overlap_similarity"])

What is reproduced from the reference, line by line:
  * every `S` line makes two nodes, 2k (the read) and 2k+1 (its reverse complement), in file order (:167-181);
    `LN:i:` gives both their length (:173, :186-187);
  * `A` lines following a `utg*` segment are consumed and recorded in read_to_node2 / node_to_read (:189-208);
  * `L` lines with 6 (raven / GFA 1), 7 (hifiasm: the `:a-b` suffix of the ids is dropped) or 8 (newer hifiasm) fields
    (:278-290); the overlap length is the integer in front of the CIGAR's letter (:292-296); zero-length overlaps are
    skipped (:299-300); the four orientation cases give the edge and its reverse-complement mate (:302-321);
  * the graph is a networkx DiGraph there: a repeated (u, v) is ONE edge whose attributes are the last ones written
    (:323-340), and prefix_length = read_length[src] - overlap_length (:339-340);
  * edge numbering: dgl.from_networkx relabels the nodes in sorted order and numbers the edges as networkx iterates
    them - by source node, and for one source in the order its out-edges were first inserted (:407).  That order is
    what `src`, `dst` and every per-edge array here follow.  (DGL itself cannot be run here; this is its documented
    behaviour, pinned in tests/golden/g10_gfa.pt through networkx's own iteration order - see make_golden_gfa.py.)

overlap_similarity (:101-117, :372-376) is 1 - editDistance(suffix, prefix) / overlap_length, which the reference gets
from the third-party aligner edlib on the CPU.  Here (`similarity="auto"`, the default) it comes, in this order, from
`SI:f:` tags on the `L` lines where the GFA carries them (our own extension, written by `write_similarity_tags`), else - for
a GFA with sequences - from the device kernel gnnome_overlap_edit_distance (gnnome_amd/overlap.py: exact edit distances,
one wavefront per overlap; needs the MI355X, there is no CPU version in this package; an overlap longer than 65 536 bases is
refused unless long_overlaps=True, which aligns it strip by strip - overlap.edit_distances); a caller-supplied
`similarity(src_seq, dst_seq, overlap_length)` callable overrides both.  A GFA without sequences and without tags gives
None - never a guess (hyperparameters.py:17 `use_similarities`: a model trained with them needs them).

training=True (:120-138, :213-272, :387-400) adds what a training step needs.  The titles of the records in `reads_path` (FASTA or
FASTQ, plain or .gz, by suffix as contigs.reads_file_type) carry `strand=`, `start=`, `end=` and `chr=` as the simulator writes them
(generate_data.py:43-60); every S line takes them from its read's title, a unitig with A lines combines its reads (strand: the sum of
title strand x A-line orientation, >= 0 -> +1; start: min; end: max; chromosome: the most common, ties to the first seen), node 2k gets
the strand and 2k+1 its opposite.  New keys read_strand, read_start, read_end, read_chr (int64[N]) and y (float32[E], edge-id order),
the labels of utils/labels.py computed on the device by gnnome_amd.labels (csrc/edge_labels.hip).  With `maf=` (the MAF file pbsim3
writes next to its FASTQ, and `maf_chr=`) the four columns come from the alignment blocks instead of the titles - gnnome_amd/maf.py, the
step generate_data.py:43-60 does with Biopython - and reads_path is not needed.  `labels` follows `similarity`:
"auto" labels on the device when there is one, else y is None with a warning; "device" insists; False leaves y None.  A read missing
from the file, or a title without one of the four fields, raises ValueError naming the read and the file.

read_gfa_device / read_gfa(parser="device" | "auto") is a second implementation of the same statement on the MI355X
(csrc/gfa_parse.hip): the file's bytes go to the device once and come back as the same dict, tensors on the device, plus
"reads" - the S-line sequences packed as overlap.pack_reads packs them.  What it declines (GfaDeviceError names the line) is
listed at _DECLINED; parser="auto" then runs the host parser, which returns or raises as it always did."""
import gzip
import re
import warnings
from collections import Counter

import numpy as np
import torch

from .textscan import DeviceDecline, first_decline, pack, read_bytes, texts, tokenise

_HIFIASM_ID = re.compile(r"(.*):\d-\d*")
# Bio.Seq.reverse_complement's table (IUPAC ambiguity codes, both cases) - the same one gnnome_amd/overlap.py hands the device
_COMPLEMENT = str.maketrans("ACGTMRWSYKVHDBXNUacgtmrwsykvhdbxnu", "TGCAKYWSRMBDHVXNAtgcakywsrmbdhvxna")


_STRAND = re.compile(r"strand=(\+|\-)")
_START = re.compile(r"start=(\d+)")
_END = re.compile(r"end=(\d+)")
_CHR = re.compile(r"chr=([0-9XYM]+)")
_CHR_CODES = {"X": -1, "Y": -2, "M": -3}


def _annotation(titles, rid, reads_path):
    """(strand, start, end, chromosome) of read `rid` from its title (graph_parser.py:213-228): the first match of each field."""
    if rid not in titles:
        raise ValueError(f"read {rid!r} is not in {reads_path}")
    title = titles[rid]
    found = [rx.search(title) for rx in (_STRAND, _START, _END, _CHR)]
    missing = [name for name, m in zip(("strand=", "start=", "end=", "chr="), found) if m is None]
    if missing:
        raise ValueError(f"read {rid!r} in {reads_path}: the title {title!r} has no {', '.join(missing)} field")
    strand, start, end, chrom = (m.group(1) for m in found)
    try:
        chrom = _CHR_CODES[chrom] if chrom in _CHR_CODES else int(chrom)
    except ValueError:
        raise ValueError(f"read {rid!r} in {reads_path}: chr={chrom} is neither a number nor X, Y or M") from None
    return (1 if strand == "+" else -1), int(start), int(end), chrom


def _node_annotations(node_to_read, num_nodes, reads_path):
    """read_strand, read_start, read_end, read_chr int64[N] (graph_parser.py:213-272)."""
    from .contigs import read_titles
    titles = read_titles(reads_path)
    cols = [[0] * num_nodes for _ in range(4)]
    for real in range(0, num_nodes, 2):
        rid = node_to_read[real]
        if isinstance(rid, list):   # a unitig: its reads from the A lines, (read id, orientation)
            if not rid:
                raise ValueError(f"unitig node {real}: no A lines name its reads, so it has no position in {reads_path}")
            anns = [_annotation(titles, r, reads_path) for r, _ in rid]
            strands = [a[0] * (1 if o == "+" else -1) for a, (_, o) in zip(anns, rid)]
            ann = (1 if sum(strands) >= 0 else -1, min(a[1] for a in anns), max(a[2] for a in anns),
                   Counter(a[3] for a in anns).most_common()[0][0])
        else:
            ann = _annotation(titles, rid, reads_path)
        strand, start, end, chrom = ann
        for col, a, b in zip(cols, (strand, start, end, chrom), (-strand, start, end, chrom)):
            col[real], col[real + 1] = a, b
    return [torch.tensor(c, dtype=torch.int64) for c in cols]


def _add_training(out, reads_path, labels, reads_parser="host", maf=None, maf_chr=None, maf_parser="host"):
    """read_strand, read_start, read_end, read_chr and y into `out` (the module docstring's training=True).  reads_parser: who reads
    the titles - "host" (_node_annotations), "device" (reads.node_annotations_device) or "auto".  With `maf` the four columns come from
    maf.node_annotations(maf, maf_chr, parser=maf_parser) and no title is read."""
    keys = ("read_strand", "read_start", "read_end", "read_chr")
    cols = None
    if maf is not None:
        from .maf import node_annotations
        cols = node_annotations(out["node_to_read"], out["num_nodes"], maf, maf_chr, parser=maf_parser)
    elif reads_parser == "device" or (reads_parser == "auto" and torch.cuda.is_available()):
        from .reads import node_annotations_device
        try:
            cols = node_annotations_device(out["node_to_read"], out["num_nodes"], reads_path)
        except Exception:   # noqa: BLE001 ("auto": whatever the device reader reports, the host code answers)
            if reads_parser == "device":
                raise
    if cols is None:
        cols = _node_annotations(out["node_to_read"], out["num_nodes"], reads_path)
    out.update(zip(keys, cols))
    out["y"] = None
    if labels == "device":
        from .labels import process_graph
        out["y"] = process_graph(out)[1].cpu()
    elif labels == "auto":
        if torch.cuda.is_available():
            from .labels import process_graph
            try:
                out["y"] = process_graph(out)[1].cpu()
            except (RuntimeError, OSError) as ex:
                warnings.warn(f"read_gfa: edge labels not computed on the device ({ex}); y is None")
        else:
            warnings.warn("read_gfa: no GPU, so the edge labels (y) were not computed; y is None")


def read_gfa(path, similarity="auto", keep_sequences=False, reads_path=None, training=False, labels="auto", parser="host",
             reads_parser="host", long_overlaps=False, maf=None, maf_chr=None, maf_parser="host"):
    """-> dict(src, dst int64[E]; num_nodes; overlap_length, prefix_length int64[E]; read_length int64[N];
    overlap_similarity float32[E] | None; read_to_node, node_to_read, read_to_node2; read_seqs | None);
    training=True adds read_strand, read_start, read_end, read_chr int64[N] and y float32[E] | None (see the module docstring).
    parser: "host" (this function's own loop), "device" (read_gfa_device, its tensors moved to the CPU: the same dict key for key,
    or GfaDeviceError where the device parser declines the file), "auto" (the device when there is one, the host parser whenever
    the device parser reports anything at all).  reads_parser: who reads the titles of `reads_path` for training=True - "host"
    (contigs.read_titles and a regex per read), "device" (gnnome_amd/reads.py: the same four tensors, the same ValueError for a read
    that is absent or lacks a field, or ReadsDeviceError where the device reader declines the file) or "auto" likewise.
    long_overlaps: handed to the device similarity call (overlap.edit_distances): True aligns overlaps beyond 65 536 bases strip by
    strip, False (the default) refuses them - similarity="device" raises, "auto" warns and leaves None.
    maf, maf_chr, maf_parser: for training=True, a pbsim3 MAF file (or a list of (path, chr) pairs, maf_chr None) as the source of the
    four read_* columns instead of the titles (gnnome_amd/maf.py; maf_parser "host", "device" or "auto" as there); reads_path is then not
    needed and no title is read.  Without `maf` nothing changes."""
    if training and reads_path is None and maf is None:
        raise ValueError("read_gfa(training=True) needs reads_path: the FASTA / FASTQ whose titles carry the read positions "
                         "(or maf=: the simulator's MAF file)")
    if maf_parser not in ("host", "device", "auto"):
        raise ValueError(f"maf_parser={maf_parser!r}: expected 'host', 'device' or 'auto'")
    if labels not in ("auto", "device", False, None):
        raise ValueError(f"labels={labels!r}: expected 'auto', 'device' or False")
    if parser not in ("host", "device", "auto"):
        raise ValueError(f"parser={parser!r}: expected 'host', 'device' or 'auto'")
    if reads_parser not in ("host", "device", "auto"):
        raise ValueError(f"reads_parser={reads_parser!r}: expected 'host', 'device' or 'auto'")
    if parser == "device" or (parser == "auto" and not callable(similarity) and torch.cuda.is_available()):
        try:
            return _read_gfa_through_device(path, similarity, keep_sequences, reads_path, training, labels, reads_parser, long_overlaps,
                                            maf, maf_chr, maf_parser)
        except Exception:   # noqa: BLE001 ("auto": whatever the device parser reports, the host parser answers)
            if parser == "device":
                raise
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as f:
        lines = f.readlines()
    read_to_node, node_to_read, read_to_node2 = {}, {}, {}
    read_lengths, read_seqs, forward = [], {}, []
    adj = []                      # adj[u]: dict v -> (overlap_length, similarity tag or None); insertion-ordered like networkx's adjacency
    no_seqs = False
    node_idx, i = 0, 0
    while i < len(lines):
        line = lines[i].strip().split()
        i += 1
        if not line:
            continue
        if line[0] == "S":
            _, rid, sequence, length = line[:4]
            if sequence == "*":
                no_seqs = True
            real, virt = node_idx, node_idx + 1
            read_to_node[rid] = (real, virt)
            node_to_read[real] = node_to_read[virt] = rid
            if similarity not in (None, False):
                forward.append(sequence)
            if keep_sequences or callable(similarity):
                read_seqs[real] = sequence
                read_seqs[virt] = sequence.translate(_COMPLEMENT)[::-1]
            ln = int(length[5:])
            read_lengths += [ln, ln]
            adj += [{}, {}]
            if rid.startswith("utg"):
                ids = []
                while i < len(lines):
                    nxt = lines[i].strip().split()
                    if not nxt or nxt[0] != "A":
                        break
                    i += 1
                    ids.append((nxt[4], nxt[3]))
                    read_to_node2[nxt[4]] = (real, virt)
                node_to_read[real] = node_to_read[virt] = ids
            node_idx += 2
        elif line[0] == "L":
            tags = []
            if len(line) >= 6 and any(t.startswith("SI:f:") for t in line[6:]):
                tags = [t for t in line[6:] if t.startswith("SI:f:")]
                line = [t for t in line if not t.startswith("SI:f:")]
            if len(line) == 6:
                _, id1, o1, id2, o2, cigar = line
            elif len(line) == 7:
                _, id1, o1, id2, o2, cigar, _ = line
                id1, id2 = _HIFIASM_ID.findall(id1)[0], _HIFIASM_ID.findall(id2)[0]
            elif len(line) == 8:
                _, id1, o1, id2, o2, cigar, _, _ = line
            else:
                raise ValueError("Unknown GFA format!")
            ol = int(cigar[:-1])
            if ol == 0:
                continue
            a, b = read_to_node[id1], read_to_node[id2]
            if o1 == "+" and o2 == "+":
                sr, dr, sv, dv = a[0], b[0], b[1], a[1]
            elif o1 == "+" and o2 == "-":
                sr, dr, sv, dv = a[0], b[1], b[0], a[1]
            elif o1 == "-" and o2 == "+":
                sr, dr, sv, dv = a[1], b[0], b[1], a[0]
            else:
                sr, dr, sv, dv = a[1], b[1], b[0], a[0]
            sim = float(tags[0][5:]) if tags else None
            adj[sr][dr] = (ol, sim)     # a repeated pair keeps its first position and takes the last attributes (networkx)
            adj[sv][dv] = (ol, sim)
    src, dst, ols, sims = [], [], [], []
    for u, nbrs in enumerate(adj):
        for v, (ol, sim) in nbrs.items():
            src.append(u)
            dst.append(v)
            ols.append(ol)
            sims.append(sim)
    read_length = torch.tensor(read_lengths, dtype=torch.int64)
    src_t, dst_t = torch.tensor(src, dtype=torch.int64), torch.tensor(dst, dtype=torch.int64)
    ol_t = torch.tensor(ols, dtype=torch.int64)
    out = {"src": src_t, "dst": dst_t, "num_nodes": node_idx, "overlap_length": ol_t,
           "prefix_length": (read_length[src_t] - ol_t) if src else ol_t.clone(), "read_length": read_length,
           "read_to_node": read_to_node, "node_to_read": node_to_read, "read_to_node2": read_to_node2,
           "read_seqs": read_seqs if keep_sequences else None, "overlap_similarity": None}
    if callable(similarity) and not no_seqs:    # an explicit aligner overrides SI:f: tags (the docstring said so, the code did not)
        out["overlap_similarity"] = torch.tensor([similarity(read_seqs[u], read_seqs[v], ol) if ol > 0 else 0.5 for u, v, ol in zip(src, dst, ols)],
                                                 dtype=torch.float32)
    elif sims and all(s is not None for s in sims):
        out["overlap_similarity"] = torch.tensor(sims, dtype=torch.float32)
    elif similarity not in (None, False) and not no_seqs and (similarity == "device" or torch.cuda.is_available()):
        from .overlap import overlap_similarity   # the MI355X kernel
        if similarity == "device":              # "device" insists: a missing library, > 32 symbols or (without long_overlaps) an overlap beyond 65 536 bases raise
            out["overlap_similarity"] = overlap_similarity(forward, src_t, dst_t, ol_t, long_overlaps=long_overlaps).cpu()
        else:                                   # "auto": what cannot be aligned here is reported and left to the caller, as before the kernel existed
            try:
                out["overlap_similarity"] = overlap_similarity(forward, src_t, dst_t, ol_t, long_overlaps=long_overlaps).cpu()
            except (RuntimeError, ValueError, OSError) as ex:
                warnings.warn(f"read_gfa: overlap similarities not computed on the device ({ex}); overlap_similarity is None")
    if training:
        _add_training(out, reads_path, labels, reads_parser, maf, maf_chr, maf_parser)
    return out


def write_similarity_tags(gfa_in, gfa_out, similarity):
    """Copy a GFA, appending `SI:f:<similarity>` to every L line: a way to carry similarities computed once (with edlib,
    on a machine that has it) inside the GFA, so that this reader needs no aligner.  `similarity[(src, dst)]` is keyed by
    node ids as read_gfa numbers them."""
    g = read_gfa(gfa_in, similarity=None)
    r2n = g["read_to_node"]
    with open(gfa_in) as f, open(gfa_out, "w") as o:
        for raw in f:
            line = raw.strip().split()
            if line and line[0] == "L":
                id1, o1, id2, o2 = line[1:5]
                if len(line) == 7:
                    id1, id2 = _HIFIASM_ID.findall(id1)[0], _HIFIASM_ID.findall(id2)[0]
                a, b = r2n[id1], r2n[id2]
                key = (a[0] if o1 == "+" else a[1], b[0] if o2 == "+" else b[1])
                if key in similarity:
                    raw = raw.rstrip("\n") + f"\tSI:f:{similarity[key]:.9g}\n"
            o.write(raw)


# ---- the device parser (csrc/gfa_parse.hip; the bytes, their tokens and the rule for the reported decline: textscan.py) ----------------

TOKENISE_TILE = 4096    # bytes one workgroup of gnnome_gfa_mark covers (gnnome_gfa_tile_sizes reports the library's own)
PACK_TILE = 16384       # output bytes one workgroup of gnnome_gfa_pack writes
TAG_SLOT = 32           # bytes of the slot an SI:f: value is packed into (the value itself: at most 31)
_REC = 8

# What the device parser declines, by the code gnnome_gfa_classify / _names_insert / _links leave on the line
_DECLINED = {
    1: "an S line with fewer than 4 fields",
    2: "the length after LN:i: is not 1-18 plain digits",
    3: "an L line without 6, 7 or 8 fields",
    4: "a 7-field link whose segment name has no :<digit>- suffix",
    5: "the overlap in front of the CIGAR letter is not 1-18 plain digits",
    6: "an SI:f: value longer than 31 bytes",
    7: "an SI:f: value that is not plain decimal text",
    8: "an A line of a unitig's run with fewer than 5 fields",
    9: "a second S line with this segment name",
    10: "an L line naming an unknown segment",
    11: "an L line naming a segment that is defined on a later line",
    12: "a byte >= 0x80",
    13: "a carriage return that no line feed follows",
    14: "field descriptors that do not belong to this buffer",
    15: "the name table is full",
}


class GfaDeviceError(DeviceDecline):
    """The device parser declines the file: .line (1-based) and .reason; read_gfa's host parser takes any GFA."""
    SERVED_BY = "the device parser (read_gfa(parser='host') or 'auto')"


def assemble_edges(u, v, overlap, tag, num_nodes):
    """Events in file order -> (src, dst, overlap_length, tag) of the edges, on the events' device (torch sorts and segment firsts /
    lasts only, so it runs on CPU tensors as well).  Event 2j is line j's (sr, dr), 2j+1 its (sv, dv).  A repeated (u, v) is one edge
    at the position of its FIRST event with the overlap and tag of its LAST (networkx's adjacency dicts, graph_parser.py:323-340);
    the edges come by u, then by first event (dgl.from_networkx, :407).  `tag`: any per-event tensor."""
    T = int(u.numel())
    if T == 0:
        return u, v, overlap, tag
    ks, order = torch.sort(u * int(num_nodes) + v, stable=True)   # ties keep file order
    start = torch.ones(T, dtype=torch.bool, device=u.device)
    start[1:] = ks[1:] != ks[:-1]
    first_pos = torch.nonzero(start).squeeze(1)
    last_pos = torch.cat([first_pos[1:] - 1, first_pos.new_tensor([T - 1])])
    first_ev, last_ev = order[first_pos], order[last_pos]
    by = torch.argsort(u[first_ev] * T + first_ev)                # distinct keys
    first_ev, last_ev = first_ev[by], last_ev[by]
    return u[first_ev], v[first_ev], overlap[last_ev], tag[last_ev]


def _parse_on_device(data, device, path="<bytes>", table_capacity=None):
    """uint8 bytes of a GFA (numpy or tensor) -> the device-side parse: dict(num_nodes, src, dst, overlap_length, tag_begin, tag_length
    per edge, read_length, buf, seg / arun records for the names, reads).  Raises GfaDeviceError for what _DECLINED lists."""
    from . import _lib
    from .ops import _on, _ptr, _stream
    lib = _lib.load()
    tok = tokenise(data, device)
    buf, n, ff, L, first_bad = tok.buf, tok.n, tok.ff, tok.L, tok.first_bad
    err = tok.err[:L]   # no line, no pointer: the library refuses the empty file (the parsers' callers get RuntimeError), as it always did
    i64 = dict(dtype=torch.int64, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    kind = torch.zeros(L, **i32)
    rec = torch.empty(L, _REC, **i64)
    with _on(device):
        _lib.check(lib.gnnome_gfa_classify(*tok.line_args(), _ptr(kind), _ptr(rec), _ptr(err), _ptr(first_bad), _stream(device)),
                   "gfa_classify")
    nf = ff[1:] - ff[:-1]
    s_line = torch.nonzero(kind == 1).squeeze(1)
    l_line = torch.nonzero(kind == 2).squeeze(1)
    R, M = int(s_line.numel()), int(l_line.numel())
    srec, lrec = rec[s_line].contiguous(), rec[l_line].contiguous()
    cap = int(table_capacity) if table_capacity is not None else max(2, 1 << (2 * R).bit_length())
    table = torch.full((cap,), -1, **i32)
    ev_u, ev_v = torch.empty(2 * M, **i64), torch.empty(2 * M, **i64)
    with _on(device):
        _lib.check(lib.gnnome_gfa_names_insert(_ptr(buf), n, _ptr(srec), _ptr(s_line), R, _ptr(table), cap, _ptr(err), L, _ptr(first_bad),
                                               _stream(device)), "gfa_names_insert")
        _lib.check(lib.gnnome_gfa_links(_ptr(buf), n, _ptr(lrec), _ptr(l_line), M, _ptr(srec), _ptr(s_line), R, _ptr(table), cap, _ptr(err),
                                        L, _ptr(first_bad), _ptr(ev_u), _ptr(ev_v), _stream(device)), "gfa_links")
    # A lines: one belongs to a segment when the nearest line above that is not an A line is a utg* S line (gfa.py's inner loop)
    line_id = torch.arange(L, **i64)
    is_a = kind == 3
    above = torch.cummax(torch.where(is_a, line_id.new_full((), -1), line_id), 0)[0] if L else line_id
    owner_ok = above >= 0
    above = above.clamp(min=0)
    in_run = is_a & owner_ok & (kind[above] == 1) & ((rec[above, 5] & 2) != 0) if L else is_a
    a_line = torch.nonzero(in_run).squeeze(1)
    a_short = a_line[nf[a_line] < 5]
    big = torch.iinfo(torch.int64).max
    found, _ = first_decline(tok, 12, 13, extra_scalars=(a_short.min() if a_short.numel() else a_short.new_tensor(big),),
                             extra_candidates=lambda a_bad: [(a_bad, 2, 8)] if a_bad != big else [])
    if found is not None:
        raise GfaDeviceError(path, found[0] + 1, _DECLINED.get(found[1], f"code {found[1]}"))
    valid = ev_u >= 0
    ev = torch.nonzero(valid).squeeze(1)
    u, v = ev_u[ev], ev_v[ev]
    ol_ev = lrec[:, 4][ev >> 1] if M else ev
    src, dst, ol, last = assemble_edges(u, v, ol_ev, ev >> 1, 2 * R)
    ln = srec[:, 4]
    out = {"num_nodes": 2 * R, "src": src, "dst": dst, "overlap_length": ol, "read_length": torch.repeat_interleave(ln, 2),
           "tag_begin": lrec[last, 6] if M else last, "tag_length": lrec[last, 7] if M else last,
           "buf": buf, "lib": lib, "seg_rec": srec, "arun_rec": rec[a_line], "reads": None}
    out["arun_owner"] = (torch.cumsum((kind == 1).long(), 0) - 1)[above[a_line]] if L else a_line
    if R and not bool((srec[:, 5] & 1).any()):
        out["reads"] = pack(lib, buf, srec[:, 2], srec[:, 3] - srec[:, 2], device)
    elif R == 0:
        out["reads"] = (torch.zeros(0, dtype=torch.uint8, device=device), torch.zeros(1, **i64))
    return out


def _names(p, device):
    """read_to_node, node_to_read, read_to_node2 from the parse (host dicts; per-item Python only over the utg* segments)."""
    lib, buf, srec, arec = p["lib"], p["buf"], p["seg_rec"], p["arun_rec"]
    names = texts(lib, buf, srec[:, 0], srec[:, 1], device)
    R = len(names)
    pairs = list(zip(range(0, 2 * R, 2), range(1, 2 * R, 2)))
    read_to_node = dict(zip(names, pairs))
    node_to_read = dict(zip(range(2 * R), (nm for nm in names for _ in (0, 1))))
    read_to_node2 = {}
    utg = torch.nonzero((srec[:, 5] & 2) != 0).squeeze(1).cpu().tolist() if R else []
    if utg:
        a_reads = texts(lib, buf, arec[:, 0], arec[:, 1], device)
        a_orient = texts(lib, buf, arec[:, 2], arec[:, 3], device)
        owner = p["arun_owner"].cpu().numpy()
        count = np.bincount(owner, minlength=R) if owner.size else np.zeros(R, dtype=np.int64)
        first = np.concatenate([[0], np.cumsum(count)])
        read_to_node2 = dict(zip(a_reads, (pairs[k] for k in owner.tolist())))
        items = list(zip(a_reads, a_orient))
        for k in utg:
            node_to_read[2 * k] = node_to_read[2 * k + 1] = items[first[k]:first[k + 1]]
    return read_to_node, node_to_read, read_to_node2


def _tag_values(p, device):
    """float32[E] from the SI:f: text of every edge: 32-byte slots gathered on the device, ONE vectorised cast on the host."""
    E = int(p["src"].numel())
    buf, beg, length = p["buf"], p["tag_begin"], p["tag_length"]
    col = torch.arange(TAG_SLOT, dtype=torch.int64, device=device)
    idx = (beg[:, None] + col[None, :]).clamp(max=int(buf.numel()) - 1)
    slots = torch.where(col[None, :] < length[:, None], buf[idx], buf.new_zeros(()))
    values = np.frombuffer(slots.cpu().numpy().tobytes(), dtype=f"S{TAG_SLOT}").astype(np.float64).astype(np.float32)
    assert values.size == E
    return torch.from_numpy(values).to(device)


def read_gfa_device(path, similarity="auto", device=None, keep_names=True, long_overlaps=False):
    """read_gfa's dict from the device parser, every tensor on `device` (same keys, dtypes and edge order; read_seqs is None), plus
    "reads": (uint8[total], int64[R+1]) on the device - the S-line sequences, forward strand, in S-line order as overlap.pack_reads
    lays them out - or None when an S line says '*'.  similarity: "auto", "device", None or False (SI:f: tags when every edge carries
    one; else, with sequences and similarity not None / False, overlap.edit_distances on g["reads"] - "device" insists, "auto" warns
    and leaves None; long_overlaps is handed to it: True aligns overlaps beyond 65 536 bases strip by strip, False refuses them); a
    callable belongs to read_gfa's host parser.  keep_names=False leaves read_to_node, node_to_read and
    read_to_node2 None (for a caller that only scores).  Raises GfaDeviceError for the inputs _DECLINED lists."""
    if callable(similarity):
        raise ValueError("read_gfa_device takes no similarity callable (it would need every read on the host): use read_gfa(path, "
                         "similarity=callable), the host parser")
    if similarity not in ("auto", "device", None, False):
        raise ValueError(f"similarity={similarity!r}: expected 'auto', 'device', None or False")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    p = _parse_on_device(read_bytes(path), device, path=str(path))
    src, dst, ol = p["src"], p["dst"], p["overlap_length"]
    out = {"src": src, "dst": dst, "num_nodes": p["num_nodes"], "overlap_length": ol,
           "prefix_length": (p["read_length"][src] - ol) if src.numel() else ol.clone(), "read_length": p["read_length"],
           "read_to_node": None, "node_to_read": None, "read_to_node2": None, "read_seqs": None, "overlap_similarity": None,
           "reads": p["reads"]}
    if keep_names:
        out["read_to_node"], out["node_to_read"], out["read_to_node2"] = _names(p, device)
    if src.numel() and bool((p["tag_length"] >= 0).all()):
        out["overlap_similarity"] = _tag_values(p, device)
    elif similarity not in (None, False) and p["reads"] is not None and p["num_nodes"]:
        from .overlap import edit_distances
        if similarity == "device":
            out["overlap_similarity"] = edit_distances(p["reads"], src, dst, ol, device, long_overlaps=long_overlaps)[1]
        else:
            try:
                out["overlap_similarity"] = edit_distances(p["reads"], src, dst, ol, device, long_overlaps=long_overlaps)[1]
            except (RuntimeError, ValueError, OSError) as ex:
                warnings.warn(f"read_gfa_device: overlap similarities not computed on the device ({ex}); overlap_similarity is None")
    return out


def _read_gfa_through_device(path, similarity, keep_sequences, reads_path, training, labels, reads_parser="host", long_overlaps=False,
                             maf=None, maf_chr=None, maf_parser="host"):
    """read_gfa(parser="device"): read_gfa_device's dict on the CPU, with read_seqs and the training keys built on the host."""
    g = read_gfa_device(path, similarity=similarity, long_overlaps=long_overlaps)
    reads = g.pop("reads")
    out = {k: (t.cpu() if torch.is_tensor(t) else t) for k, t in g.items()}
    if keep_sequences:
        if reads is None:
            raise GfaDeviceError(path, 1, "keep_sequences with S lines that say '*'")
        text, off = reads[0].cpu().numpy().tobytes().decode("ascii"), reads[1].cpu().tolist()
        seqs = {}
        for r in range(len(off) - 1):
            seqs[2 * r] = text[off[r]:off[r + 1]]
            seqs[2 * r + 1] = seqs[2 * r].translate(_COMPLEMENT)[::-1]
        out["read_seqs"] = seqs
    if training:
        _add_training(out, reads_path, labels, reads_parser, maf, maf_chr, maf_parser)
    return out
