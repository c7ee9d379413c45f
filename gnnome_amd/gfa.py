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
one wavefront per overlap; needs the MI355X, there is no CPU version in this package); a caller-supplied
`similarity(src_seq, dst_seq, overlap_length)` callable overrides both.  A GFA without sequences and without tags gives
None - never a guess (hyperparameters.py:17 `use_similarities`: a model trained with them needs them).

training=True (:120-138, :213-272, :387-400) adds what a training step needs.  The titles of the records in `reads_path` (FASTA or
FASTQ, plain or .gz, by suffix as contigs.reads_file_type) carry `strand=`, `start=`, `end=` and `chr=` as the simulator writes them
(generate_data.py:43-60); every S line takes them from its read's title, a unitig with A lines combines its reads (strand: the sum of
title strand x A-line orientation, >= 0 -> +1; start: min; end: max; chromosome: the most common, ties to the first seen), node 2k gets
the strand and 2k+1 its opposite.  New keys read_strand, read_start, read_end, read_chr (int64[N]) and y (float32[E], edge-id order),
the labels of utils/labels.py computed on the device by gnnome_amd.labels (csrc/edge_labels.hip).  `labels` follows `similarity`:
"auto" labels on the device when there is one, else y is None with a warning; "device" insists; False leaves y None.  A read missing
from the file, or a title without one of the four fields, raises ValueError naming the read and the file."""
import gzip
import re
import warnings
from collections import Counter

import torch

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


def read_gfa(path, similarity="auto", keep_sequences=False, reads_path=None, training=False, labels="auto"):
    """-> dict(src, dst int64[E]; num_nodes; overlap_length, prefix_length int64[E]; read_length int64[N];
    overlap_similarity float32[E] | None; read_to_node, node_to_read, read_to_node2; read_seqs | None);
    training=True adds read_strand, read_start, read_end, read_chr int64[N] and y float32[E] | None (see the module docstring)."""
    if training and reads_path is None:
        raise ValueError("read_gfa(training=True) needs reads_path: the FASTA / FASTQ whose titles carry the read positions")
    if labels not in ("auto", "device", False, None):
        raise ValueError(f"labels={labels!r}: expected 'auto', 'device' or False")
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
        if similarity == "device":              # "device" insists: a missing library, > 32 symbols or an overlap beyond 65 536 bases raise
            out["overlap_similarity"] = overlap_similarity(forward, src_t, dst_t, ol_t).cpu()
        else:                                   # "auto": what cannot be aligned here is reported and left to the caller, as before the kernel existed
            try:
                out["overlap_similarity"] = overlap_similarity(forward, src_t, dst_t, ol_t).cpu()
            except (RuntimeError, ValueError, OSError) as ex:
                warnings.warn(f"read_gfa: overlap similarities not computed on the device ({ex}); overlap_similarity is None")
    if training:
        keys = ("read_strand", "read_start", "read_end", "read_chr")
        out.update(zip(keys, _node_annotations(node_to_read, node_idx, reads_path)))
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
