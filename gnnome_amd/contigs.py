"""Walks -> contig sequences, FASTA and N50 / NG50 on the MI355X (utils/evaluate.py:38-105; inference.py:475-489).

    store = ReadStore.from_gfa("asm.gfa")                                     # or from_reads_file(...) for a GFA without sequences
    contigs = spell_contigs(dg, walks, store)                                 # dg: the decode.DecodeGraph the walks came from
    write_fasta(contigs, "0_assembly.fasta")                                  # = SeqIO.write(records, path, "fasta")
    n50, ng50 = calculate_N50(contigs), calculate_NG50(contigs, ref_length)

The reference spells each contig in Python from a dict that holds every read twice, once per strand (graph_parser.py:183-184,
:365), and writes it with Biopython.  Here the read store holds the forward strand once, on the device (overlap.pack_reads);
gnnome_contig_pieces (csrc/contig_spell.hip) checks every walk and turns each step into the length of the piece it contributes,
torch scans those lengths into offsets, and gnnome_contig_spell copies the pieces - the reverse complement of an odd node is read
backwards through the complement table, never stored.  For FASTA the kernel writes the 60-column bodies straight into the file
image; the host builds the header lines, and the file is one device-to-host copy and one write.
"""
import ctypes
import gzip
import numbers
import os

import numpy as np
import torch

from . import _lib
from .ops import _on, _ptr, _stream
from .overlap import pack_reads

FASTA_WRAP = 60   # Bio.SeqIO.FastaIO.FastaWriter's default wrap, which SeqIO.write(..., "fasta") uses (evaluate.py:53)

# graph_parser.py:346-358: the reads file's type from its suffix
_FASTA_SUFFIXES = ("fasta", "fna", "fa")
_FASTQ_SUFFIXES = ("fastq", "fnq", "fq")


def _default_device():
    return torch.device("cuda", torch.cuda.current_device())


def _keep_mask(keep, num_reads):
    if keep is None:
        return None
    mask = np.zeros(num_reads, dtype=bool)
    idx = np.asarray(list(keep) if not isinstance(keep, (np.ndarray, torch.Tensor)) else keep)
    if idx.dtype == bool:
        mask[:] = idx[:num_reads]
    elif idx.size:
        mask[idx.astype(np.int64)] = True
    return mask


class ReadStore:
    """The reads, forward strand only, concatenated on the device: read r is data[off[r]:off[r+1]]; node 2r is read r and node
    2r+1 its reverse complement.  `missing` (bool[R] or None): reads left out of the store as zero-length slots (constructors'
    `keep=`), so that device memory follows the assembly rather than the read set; spelling a walk through one raises."""

    def __init__(self, data, off, missing=None):
        self.data, self.off = data, off
        self.num_reads = int(off.numel()) - 1
        self.missing = missing

    @classmethod
    def from_sequences(cls, sequences, keep=None, device=None):
        """sequences[r] = read r (str or bytes).  keep: read indices (or a bool mask) to store; None = all."""
        sequences = list(sequences)
        mask = _keep_mask(keep, len(sequences))
        if mask is not None:
            sequences = [s if m else b"" for s, m in zip(sequences, mask)]
        data, off = pack_reads(sequences)
        device = device or _default_device()
        return cls(data.to(device), off.to(device), None if mask is None else ~mask)

    @classmethod
    def from_gfa(cls, path, keep=None, device=None):
        """The S-line sequences of a GFA, in S-line order (read r = the r-th S line, graph_parser.py:167-181)."""
        seqs = gfa_sequences(path)
        if seqs is None:
            raise ValueError(f"{path}: the S lines carry no sequences ('*'); use ReadStore.from_reads_file with the reads")
        return cls.from_sequences(seqs, keep=keep, device=device)

    @classmethod
    def from_reads_file(cls, path, node_to_read, num_nodes, keep=None, device=None, parser="host"):
        """For a GFA whose S lines say '*': read r is the record of the FASTA / FASTQ file (plain or .gz) whose id is
        node_to_read[2r] (graph_parser.py:341-366; read_gfa's "node_to_read").  A unitig segment with A-lines maps to several
        reads and has no single record: that raises, as in the reference (there a TypeError).  parser: "host" (the per-record loop
        below), "device" (reads.read_reads_device: the same data, off and missing, the same errors, or ReadsDeviceError where the
        device reader declines the file), "auto" (the device when there is one, the host loop whenever it reports anything at all)."""
        if parser not in ("host", "device", "auto"):
            raise ValueError(f"parser={parser!r}: expected 'host', 'device' or 'auto'")
        num_reads = int(num_nodes) // 2
        ids = []
        for r in range(num_reads):
            rid = node_to_read[2 * r]
            if not isinstance(rid, str):
                raise ValueError(f"node {2 * r} is a unitig segment made of {len(rid)} reads (A-lines): its sequence is not one record "
                                 f"of {path}; use a GFA that carries the unitig sequences on its S lines")
            ids.append(rid)
        mask = _keep_mask(keep, num_reads)
        if parser == "device" or (parser == "auto" and torch.cuda.is_available()):
            from .reads import read_store_arrays
            try:
                data, off = read_store_arrays(path, ids, mask, device or _default_device())
                return cls(data, off, None if mask is None else ~mask)
            except Exception:   # noqa: BLE001 ("auto": whatever the device reader reports, the host loop answers)
                if parser == "device":
                    raise
        wanted = set(ids) if mask is None else {rid for rid, m in zip(ids, mask) if m}
        found = read_sequences(path, wanted)
        seqs = []
        for r, rid in enumerate(ids):
            if mask is not None and not mask[r]:
                seqs.append(b"")
                continue
            if rid not in found:
                raise KeyError(f"read {rid!r} (node {2 * r}) is not in {path}")
            seqs.append(found[rid])
        return cls.from_sequences(seqs, keep=mask, device=device)

    @classmethod
    def from_packed(cls, data, off, keep=None):
        """From reads already packed on the device - gfa.read_gfa_device's g["reads"]: (uint8[total], int64[R+1]).  keep: read indices
        (or a bool mask) to store; the others become zero-length slots and `missing` is set, as in the other constructors.  The
        restriction is one gnnome_gfa_pack over the kept lengths; nothing visits the host."""
        if keep is None:
            return cls(data, off)
        from .textscan import pack
        mask = _keep_mask(keep, int(off.numel()) - 1)
        lengths = (off[1:] - off[:-1]) * torch.from_numpy(mask).to(off.device)
        kept, kept_off = pack(_lib.load(), data, off[:-1], lengths, data.device)
        return cls(kept, kept_off, ~mask)

    def sequence(self, node):
        """Node `node` as a str (host; for checks)."""
        r = node >> 1
        a, b = int(self.off[r]), int(self.off[r + 1])
        s = self.data[a:b].cpu().numpy().tobytes().decode("latin-1")
        return s if node % 2 == 0 else s.translate(_COMPLEMENT_STR)[::-1]


_COMPLEMENT_STR = str.maketrans("ACGTMRWSYKVHDBXNUacgtmrwsykvhdbxnu", "TGCAKYWSRMBDHVXNAtgcakywsrmbdhvxna")


def gfa_sequences(path):
    """S-line sequences of a GFA in file order (bytes), or None if any S line says '*'.  read_gfa's own outputs are not involved."""
    opener = gzip.open if str(path).endswith(".gz") else open
    seqs = []
    with opener(path, "rt") as f:
        for line in f:
            if not line.startswith("S"):
                continue
            parts = line.split()
            if parts[0] != "S":
                continue
            if len(parts) < 3 or parts[2] == "*":
                return None
            seqs.append(parts[2].encode("ascii"))
    return seqs


def reads_file_type(path):
    """'fasta' or 'fastq' from the suffix, as graph_parser.py:346-358 chooses it."""
    p = str(path)
    if p.endswith("gz"):
        if p.endswith(tuple(s + ".gz" for s in _FASTA_SUFFIXES)):
            return "fasta"
        if p.endswith(tuple(s + ".gz" for s in _FASTQ_SUFFIXES)):
            return "fastq"
    else:
        if p.endswith(_FASTA_SUFFIXES):
            return "fasta"
        if p.endswith(_FASTQ_SUFFIXES):
            return "fastq"
    raise ValueError(f"{path}: not a reads file by its suffix (fasta / fna / fa / fastq / fnq / fq, optionally .gz)")


def _records(path, sequences=True):
    """(title, sequence lines | None) of every record of a FASTA (multi-line) or FASTQ file, plain or gzip, in file order.  The title
    is the header line without its marker and trailing whitespace (Biopython's record.description); sequences=False keeps no
    sequence (the FASTQ checks still run)."""
    kind = reads_file_type(path)
    opener = gzip.open if str(path).endswith("gz") else open
    with opener(path, "rt") as f:
        if kind == "fasta":        # Bio.SeqIO.FastaIO.SimpleFastaParser
            title, chunks = None, []
            for line in f:
                if line.startswith(">"):
                    if title is not None:
                        yield title, chunks if sequences else None
                    title, chunks = line[1:].rstrip(), []
                elif title is not None and sequences:
                    chunks.append(line.strip())
            if title is not None:
                yield title, chunks if sequences else None
        else:                      # Bio.SeqIO.QualityIO.FastqGeneralIterator: sequence lines up to '+', as many quality characters
            line = f.readline()
            while line:
                if not line.strip():
                    line = f.readline()
                    continue
                if not line.startswith("@"):
                    raise ValueError(f"{path}: FASTQ record does not start with '@': {line[:40]!r}")
                title, chunks, n = line[1:].rstrip(), [], 0
                line = f.readline()
                while line and not line.startswith("+"):
                    n += len(line.strip())
                    if sequences:
                        chunks.append(line.strip())
                    line = f.readline()
                if not line:
                    raise ValueError(f"{path}: FASTQ record {title.split()[0] if title.split() else ''!r} ends before its '+' line")
                q = 0
                line = f.readline()
                while line and q < n:
                    q += len(line.strip())
                    line = f.readline()
                if q != n:
                    raise ValueError(f"{path}: FASTQ record {title!r}: {n} bases but {q} quality values")
                yield title, chunks if sequences else None


def _record_id(title):
    return title.split(None, 1)[0] if title.strip() else ""


def read_sequences(path, wanted=None):
    """{record id: sequence bytes} of a FASTA (multi-line) or FASTQ file, plain or gzip.  The id is the first whitespace-separated
    token of the header (Biopython's record.id); a repeated id keeps its last record, like the reference's dict.  `wanted`: keep
    only these ids."""
    out = {}
    for title, chunks in _records(path):
        rid = _record_id(title)
        if wanted is None or rid in wanted:
            out[rid] = "".join(chunks).replace(" ", "").replace("\r", "").encode("ascii")
    return out


def read_titles(path):
    """{record id: whole title} of a FASTA or FASTQ file, plain or gzip - the reference's {read.id: read.description for read in
    SeqIO.parse(...)} (graph_parser.py:121-136).  No sequence is kept; a repeated id keeps its last record."""
    return {_record_id(title): title for title, _ in _records(path, sequences=False)}


class ContigRecord:
    """What evaluate.py:44-46 makes of a contig: .id, .description, .seq (a str here; a Bio.Seq there)."""

    __slots__ = ("id", "description", "seq")

    def __init__(self, id, description, seq):   # noqa: A002 (the reference's attribute name)
        self.id, self.description, self.seq = id, description, seq

    def __len__(self):
        return len(self.seq)

    def __repr__(self):
        return f"ContigRecord(id={self.id!r}, description={self.description!r}, len={len(self.seq)})"


def _header(i, n):
    return f">contig_{i + 1} length={n}\n"   # FastaWriter: '>' + id + ' ' + description (evaluate.py:44-46)


class Contigs:
    """Spelled contigs on the device.  line_width == 0: `data` is the contigs concatenated, contig i = data[offsets[i]:offsets[i+1]].
    line_width > 0: `data` is the whole FASTA file image (headers + wrapped bodies; contig i's body starts at body_off[i]).
    Iterating yields ContigRecords, so a Contigs stands wherever the reference passes its list of SeqRecords."""

    def __init__(self, plan, line_width):
        self._plan, self.line_width = plan, int(line_width)
        self.offsets = plan["contig_off"]                       # int64[W+1], device, unwrapped layout
        self.lengths = self.offsets[1:] - self.offsets[:-1]     # int64[W], device
        self._lengths_host = None
        self.body_off = None
        self.data = None

    def __len__(self):
        return int(self.offsets.numel()) - 1

    def lengths_host(self):
        if self._lengths_host is None:
            self._lengths_host = self.lengths.cpu().numpy()
        return self._lengths_host

    def sequence(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        if self.line_width == 0:
            a, b = int(self.offsets[i]), int(self.offsets[i + 1])
            return self.data[a:b].cpu().numpy().tobytes().decode("latin-1")
        n = int(self.lengths_host()[i])
        a = int(self.body_off[i])
        body = self.data[a:a + n + -(-n // self.line_width)].cpu().numpy().tobytes()
        return body.replace(b"\n", b"").decode("latin-1")

    def record(self, i):
        n = int(self.lengths_host()[i])
        return ContigRecord(f"contig_{i + 1}", f"length={n}", self.sequence(i))

    def records(self):
        for i in range(len(self)):
            yield self.record(i)

    __iter__ = records

    def __getitem__(self, i):
        return self.record(i if i >= 0 else len(self) + i)

    def respell(self, line_width):
        """The same contigs in another layout (one more copy kernel; pieces and offsets are reused)."""
        return _materialise(self._plan, line_width)

    def fasta_bytes(self):
        """The FASTA file image on the host (one device-to-host copy)."""
        if self.line_width == 0:
            raise ValueError("a FASTA image needs line_width > 0: use respell(60)")
        return self.data.cpu().numpy()


def _materialise(plan, line_width):
    if line_width < 0:
        raise ValueError("line_width must be >= 0")
    lib = _lib.load()
    c = Contigs(plan, line_width)
    dev, store = plan["device"], plan["reads"]
    W, S = len(c), int(plan["nodes"].numel())
    body_off = None
    if line_width == 0:
        total = int(c.offsets[-1]) if W else 0
        c.data = torch.empty(total, dtype=torch.uint8, device=dev)
    else:
        n = c.lengths_host().astype(np.int64)
        heads = [_header(i, int(k)).encode("ascii") for i, k in enumerate(n)]
        hl = np.fromiter((len(h) for h in heads), dtype=np.int64, count=W)
        blen = n + (n + line_width - 1) // line_width
        rec = hl + blen
        rec_off = np.zeros(W + 1, dtype=np.int64)
        np.cumsum(rec, out=rec_off[1:])
        c.body_off = rec_off[:-1] + hl
        total = int(rec_off[-1])
        c.data = torch.empty(total, dtype=torch.uint8, device=dev)
        if W:   # the header lines: built here, placed into the image by one scatter
            hbytes = np.frombuffer(b"".join(heads), dtype=np.uint8)
            hstart = np.zeros(W, dtype=np.int64)
            np.cumsum(hl[:-1], out=hstart[1:])
            pos = np.repeat(rec_off[:-1] - hstart, hl) + np.arange(hbytes.size, dtype=np.int64)
            c.data[torch.from_numpy(pos).to(dev)] = torch.from_numpy(hbytes.copy()).to(dev)
        body_off = torch.from_numpy(c.body_off).to(dev)
    if W and total:
        with _on(dev):
            _lib.check(lib.gnnome_contig_spell(_ptr(plan["nodes"]), S, _ptr(plan["walk_off"]), W, _ptr(plan["piece_off"]), _ptr(store.data),
                                               _ptr(store.off), store.num_reads, _ptr(body_off), line_width, _ptr(c.data), total,
                                               _stream(dev)), "contig_spell")
    return c


def _walk_arrays(walks):
    if isinstance(walks, tuple) and len(walks) == 2 and torch.is_tensor(walks[0]):
        return torch.as_tensor(walks[0]), torch.as_tensor(walks[1])
    walks = [list(map(int, w)) if not torch.is_tensor(w) else w.tolist() for w in walks]
    off = np.zeros(len(walks) + 1, dtype=np.int64)
    np.cumsum([len(w) for w in walks], out=off[1:])
    flat = np.fromiter((v for w in walks for v in w), dtype=np.int64, count=int(off[-1]))
    if flat.size and (flat.min() < -2 ** 31 or flat.max() >= 2 ** 31):
        raise OverflowError("a node id does not fit int32")
    return torch.from_numpy(flat.astype(np.int32)), torch.from_numpy(off)


def spell_contigs(dg, walks, reads, line_width=0):
    """evaluate.py:38-48 on the device.  dg: decode.DecodeGraph (its successor lists, succ_eid and prefix lengths - the prefixes
    as given: pipeline.assemble masks them, inference.py:463); walks: lists of node ids, or (int32 nodes, int64 offsets[W+1]);
    reads: a ReadStore with R = dg.num_nodes / 2.  -> Contigs.  A pair that is not an edge, a node outside [0, 2R) or an empty
    walk raises (GnnomeHipError naming the walk and the pair) before anything is written."""
    lib = _lib.load()
    dev = dg.device
    if 2 * reads.num_reads != dg.num_nodes:
        raise ValueError(f"the graph has {dg.num_nodes} nodes, the read store {reads.num_reads} reads (node 2r is read r)")
    nodes, walk_off = _walk_arrays(walks)
    if reads.missing is not None and nodes.numel():
        hn = nodes.cpu().long().numpy()
        inr = (hn >= 0) & (hn < dg.num_nodes)
        gap = np.zeros(hn.size, dtype=bool)
        gap[inr] = reads.missing[hn[inr] >> 1]
        if gap.any():
            j = int(np.argmax(gap))
            w = int(np.searchsorted(walk_off.cpu().numpy(), j, side="right")) - 1
            raise ValueError(f"walk {w}: node {int(hn[j])} needs read {int(hn[j]) >> 1}, which the read store left out (keep=)")
    nodes = nodes.to(dev, torch.int32).contiguous()
    walk_off = walk_off.to(dev, torch.int64).contiguous()
    W, S = int(walk_off.numel()) - 1, int(nodes.numel())
    piece_len = torch.empty(S, dtype=torch.int64, device=dev)
    nbr, eid, pre = dg.succ_nbr, dg.succ_eid, dg.prefix_length
    if dg.num_edges == 0:   # every walk a single node: the arrays are empty and never read, but the C entry declines a null pointer
        nbr = eid = pre = torch.zeros(1, dtype=torch.int32, device=dev)
    need = ctypes.c_size_t(0)
    _lib.check(lib.gnnome_contig_pieces_workspace_bytes(W, S, ctypes.byref(need)), "contig_pieces_workspace_bytes")
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(lib.gnnome_contig_pieces(_ptr(nodes), S, _ptr(walk_off), W, _ptr(dg.succ_ptr), _ptr(nbr), _ptr(eid), _ptr(pre), dg.num_nodes,
                                            _ptr(reads.off), reads.num_reads, _ptr(piece_len), _ptr(ws), ws.numel(), _stream(dev)),
                   "contig_pieces")
    piece_off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    torch.cumsum(piece_len, 0, out=piece_off[1:])
    plan = {"device": dev, "nodes": nodes, "walk_off": walk_off, "piece_off": piece_off, "reads": reads,
            "contig_off": piece_off[walk_off] if W else torch.zeros(1, dtype=torch.int64, device=dev)}
    return _materialise(plan, line_width)


def _as_decode_graph(graph, device=None):
    from .decode import DecodeGraph
    if isinstance(graph, DecodeGraph):
        return graph
    if isinstance(graph, dict):   # gfa.read_gfa's dict
        return DecodeGraph(graph["src"], graph["dst"], graph["num_nodes"], graph["prefix_length"], graph["read_length"], device=device)
    src, dst = graph.edges()      # a DGL graph, as evaluate.py:38 receives it
    n = int(graph.num_nodes())
    rl = graph.ndata["read_length"] if "read_length" in graph.ndata else torch.zeros(n, dtype=torch.int64)
    return DecodeGraph(src, dst, n, graph.edata["prefix_length"], rl, device=device)


def walk_to_sequence(walks, graph, reads, edges=None):
    """evaluate.py:38-48 with the same signature.  graph: a DGL-like graph (edges(), num_nodes(), edata['prefix_length']), read_gfa's
    dict or a DecodeGraph; reads: the reference's node -> sequence dict (only the even entries - the forward strands - of the reads
    the walks touch are read) or a ReadStore.  `edges` is accepted and not read: the pair -> edge-id map is a function of the edge
    list (graph_parser.py:77-80), which decode.DecodeGraph rebuilds.  -> Contigs (iterates as the reference's records)."""
    del edges
    dg = _as_decode_graph(graph)
    if not isinstance(reads, ReadStore):
        touched = sorted({int(v) >> 1 for w in walks for v in w if 0 <= int(v) < dg.num_nodes})
        seqs = [b""] * (dg.num_nodes // 2)
        for r in touched:
            s = reads[2 * r]
            seqs[r] = s.encode("ascii") if isinstance(s, str) else (bytes(s) if isinstance(s, (bytes, bytearray)) else str(s).encode("ascii"))
        reads = ReadStore.from_sequences(seqs, keep=touched, device=dg.device)
    return spell_contigs(dg, walks, reads)


def _fasta_title(rec):
    """Bio.SeqIO.FastaIO.FastaWriter's title line."""
    rid, desc = str(rec.id), str(rec.description)
    if desc and desc.split(None, 1)[0] == rid:
        return desc
    return f"{rid} {desc}" if desc else rid


def write_fasta(contigs, path, line_width=FASTA_WRAP):
    """The bytes SeqIO.write(records, path, "fasta") writes (evaluate.py:51-53): '>id description' and 60-column lines.
    Contigs: the kernel writes the bodies into the file image on the device; one device-to-host copy and one write.  Records or
    strings held on the host (str items become contig_{i+1} length={n}) are formatted on the host."""
    if line_width <= 0:
        raise ValueError("line_width must be > 0 (FastaWriter wraps)")
    if isinstance(contigs, Contigs):
        img = contigs if contigs.line_width == line_width else contigs.respell(line_width)
        with open(path, "wb") as f:
            img.fasta_bytes().tofile(f)
        return path
    with open(path, "w", newline="\n") as f:
        for i, rec in enumerate(contigs):
            if isinstance(rec, (str, bytes)):
                seq = rec.decode("latin-1") if isinstance(rec, bytes) else rec
                rec = ContigRecord(f"contig_{i + 1}", f"length={len(seq)}", seq)
            seq = str(rec.seq)
            f.write(f">{_fasta_title(rec)}\n")
            for k in range(0, len(seq), line_width):
                f.write(seq[k:k + line_width] + "\n")
    return path


def save_assembly(contigs, save_dir, idx, suffix=""):
    """evaluate.py:51-53: {save_dir}/{idx}_assembly{suffix}.fasta."""
    return write_fasta(contigs, os.path.join(save_dir, f"{idx}_assembly{suffix}.fasta"))


def _lengths(contigs):
    if isinstance(contigs, Contigs):
        return [int(x) for x in contigs.lengths_host()]
    items = list(contigs)
    return [int(c) if isinstance(c, (numbers.Integral, np.integer)) else len(c) if isinstance(c, (str, bytes)) else len(c.seq) for c in items]


def calculate_N50(contigs):   # noqa: N802 (the reference's name)
    """evaluate.py:56-72.  contigs: Contigs, records (.seq) or a list of lengths.  -1 without contigs."""
    lengths = sorted(_lengths(contigs), reverse=True)
    total, acc = sum(lengths), 0
    for n in lengths:
        acc += n
        if acc >= total / 2:
            return n
    return -1


def calculate_NG50(contigs, ref_length):   # noqa: N802
    """evaluate.py:75-91: -1 for ref_length <= 0, or when the contigs do not reach half of it."""
    if ref_length <= 0:
        return -1
    lengths = sorted(_lengths(contigs), reverse=True)
    acc = 0
    for n in lengths:
        acc += n
        if acc >= ref_length / 2:
            return n
    return -1


def quick_evaluation(contigs, ref_length=None):
    """evaluate.py:94-105 with the reference length from the caller (there: a chromosome-length table) ->
    (num_contigs, longest_contig, reconstructed, n50, ng50); reconstructed = ng50 = -1 without ref_length."""
    lengths = _lengths(contigs)
    if not lengths:
        raise ValueError("quick_evaluation: no contigs (the reference's max() of an empty list)")
    n50 = calculate_N50(lengths)
    if ref_length:
        return len(lengths), max(lengths), sum(lengths) / ref_length, n50, calculate_NG50(lengths, ref_length)
    return len(lengths), max(lengths), -1, n50, -1
