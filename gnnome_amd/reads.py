"""A FASTA / FASTQ reads file on the MI355X: the records of the wanted ids, their sequences and the positions in their titles
(graph_parser.py:121-136, :213-272, :341-366; csrc/reads_parse.hip).

    res = read_reads_device("reads.fq.gz", names, sequences=True, titles=True)
    res.last                 int64[R]: the index of the LAST record whose id is names[r], -1 without one
    res.data, res.off        uint8[total], int64[R+1]: the sequences packed as overlap.pack_reads packs them
    res.ann, res.missing     int64[R,4] strand, start, end, chromosome and int32[R] bit k = field k has no match (15: no record)

This is a second implementation of the statement the host code makes - contigs._records, _record_id, read_sequences and read_titles,
gfa._annotation and gfa._node_annotations - and nothing else: wherever it accepts a file it returns what they return.  The file's
bytes go to the device once (.gz is decompressed on the host) and textscan.tokenise finds their fields and lines, one thread per
line (FASTA) or per record (FASTQ) finds the id, title and sequence ranges, the wanted names sit in an open-addressing table that every
record looks its id up in (integer atomicMax on the record index: the last record of an id wins, like the host's dict), one thread per
matched record searches its title, and gnnome_gfa_pack copies the sequence lines - FASTQ quality bytes are never copied.  What the
device path cannot serve it declines (ReadsDeviceError names the line; _DECLINED lists the cases); parser="auto" in the callers then
runs the host code, which returns or raises as it always did.

Synchronisations per file: one for each compaction whose size the host must know (field starts, field ends and line starts of the
tokeniser, the header / sequence-line or non-blank-line lists), ONE that reports (the earliest declined line, the two byte checks and
the table), and with sequences one for the number of pack items and one for the packed size."""
import numpy as np
import torch

from . import _lib
from .contigs import reads_file_type
from .textscan import DeviceDecline, first_decline, load_within, lookup_names, pack, pack_names as _pack_names, tokenise  # noqa: F401

# What the device reader declines: codes 1-4 are left on the line by the kernels of csrc/reads_parse.hip, 5 and 6 come from
# gnnome_gfa_mark's byte checks, 7 from the name table, 8 is decided before the upload.  7 and 8 belong to no line: .line is 0.
_DECLINED = {
    1: "a sequence or quality line with more than one field",
    2: "a FASTQ record that is not in the four-line form (@title, one sequence line, +, as many quality characters)",
    3: "a number of more than 18 digits in a title",
    4: "a chr= value that mixes digits and letters",
    5: "a byte >= 0x80",
    6: "a carriage return that no line feed follows",
    7: "the name table is full",
    8: "a file above max_bytes",
}
_FIELDS = ("strand=", "start=", "end=", "chr=")


class ReadsDeviceError(DeviceDecline):
    """The device reader declines the file: .line (1-based; 0 where no line is at fault) and .reason; the host code takes any file."""
    SERVED_BY = "the device reader (parser='host' or 'auto')"


class DeviceReads:
    """read_reads_device's result (see the module docstring); data / off and ann / missing are None when not asked for."""

    def __init__(self, path, num_names):
        self.path, self.num_names = path, num_names
        self.last = self.data = self.off = self.ann = self.missing = None
        self.num_records = 0
        self._buf = self._rec = None


def record_title(res, k):
    """The title of record k of the file `res` was read from (the header line without its marker and trailing whitespace), as a str:
    one small device-to-host copy, for error messages."""
    if not 0 <= k < res.num_records:
        raise IndexError(k)
    b, e = res._rec[k, 2:4].cpu().tolist()
    return res._buf[b:e].cpu().numpy().tobytes().decode("ascii")


def pack_items(last, keep, seq_first, item_beg, item_len):
    """The pack items of the wanted reads, in read order (torch only: runs on CPU tensors as well).  last int64[R]: each read's record or
    -1; keep bool[R] or None; record k's sequence lines are items seq_first[k] : seq_first[k+1] of item_beg / item_len (int64[K+1],
    int64[S], int64[S]).  -> (src_beg, lengths, first): read r owns the returned items first[r] : first[r+1] (int64[R+1]); a read
    without a record or outside `keep` owns none."""
    R, K = int(last.numel()), int(seq_first.numel()) - 1
    have = last >= 0
    if keep is not None:
        have = have & keep
    k = last.clamp(min=0, max=max(K - 1, 0))
    count = torch.where(have, seq_first[(k + 1).clamp(max=K)] - seq_first[k], torch.zeros_like(last)) if K > 0 else torch.zeros_like(last)
    first = torch.zeros(R + 1, dtype=torch.int64, device=last.device)
    torch.cumsum(count, 0, out=first[1:])
    total = int(first[-1]) if R else 0
    owner = torch.repeat_interleave(torch.arange(R, dtype=torch.int64, device=last.device), count, output_size=total)
    idx = seq_first[k][owner] + (torch.arange(total, dtype=torch.int64, device=last.device) - first[:-1][owner])
    return item_beg[idx], item_len[idx], first


def combine_annotations(owner, sign, ann, num_owners):
    """gfa._node_annotations' rule for a segment made of several reads, for all segments at once (torch sorts and scans only: runs on CPU
    tensors as well).  Entry i belongs to segment owner[i] (int64, rising), sign[i] = +1 / -1 its A-line orientation, ann[i] = its
    title's strand, start, end, chromosome.  -> int64[num_owners, 4]: strand = +1 where the sum of strand x orientation is >= 0 else -1,
    start = min, end = max, chromosome = the most common one, ties to the first seen in entry order.  A segment without entries: 0."""
    E, S = int(owner.numel()), int(num_owners)
    out = torch.zeros(S, 4, dtype=torch.int64, device=ann.device)
    if E == 0 or S == 0:
        return out
    count = torch.bincount(owner, minlength=S)
    first = torch.zeros(S + 1, dtype=torch.int64, device=ann.device)
    torch.cumsum(count, 0, out=first[1:])
    lo, hi = first[:-1].clamp(max=E - 1), (first[1:] - 1).clamp(min=0)
    cs = torch.zeros(E + 1, dtype=torch.int64, device=ann.device)
    torch.cumsum(ann[:, 0] * sign, 0, out=cs[1:])
    total = cs[first[1:]] - cs[first[:-1]]
    out[:, 0] = torch.where(total >= 0, 1, -1)

    def by_owner_then(values):   # a permutation: by owner, within an owner by value, ties in entry order
        o1 = torch.argsort(values, stable=True)
        return o1[torch.argsort(owner[o1], stable=True)]

    out[:, 1] = ann[by_owner_then(ann[:, 1]), 1][lo]
    out[:, 2] = ann[by_owner_then(ann[:, 2]), 2][hi]
    order = by_owner_then(ann[:, 3])
    so, sc = owner[order], ann[order, 3]
    new = torch.ones(E, dtype=torch.bool, device=ann.device)
    new[1:] = (so[1:] != so[:-1]) | (sc[1:] != sc[:-1])
    run = torch.nonzero(new).squeeze(1)                       # runs of one (segment, chromosome)
    run_len = torch.cat([run[1:], run.new_tensor([E])]) - run
    run_owner, run_chr = so[run], sc[run]
    key = run_len * (E + 1) + (E - order[run])                # longer first; then the one first seen (the run's first entry is its earliest)
    o3 = torch.argsort(key, stable=True)
    best = o3[torch.argsort(run_owner[o3], stable=True)]      # by segment, the best run last
    run_last = torch.cumsum(torch.bincount(run_owner, minlength=S), 0) - 1
    out[:, 3] = run_chr[best][run_last.clamp(min=0)]
    out[count == 0] = 0
    return out


def read_reads_device(path, names, device=None, sequences=True, titles=False, max_bytes=None, keep=None, table_capacity=None):
    """-> DeviceReads for the wanted ids `names` (a list of str; a repeated name is legal) from the FASTA / FASTQ file `path` (plain or
    .gz; the type by suffix as contigs.reads_file_type).  sequences: pack the sequence of every name's last record (keep: bool numpy
    mask over the names, the others enter as zero lengths, as in ReadStore.from_packed).  titles: the four title fields of that record.
    max_bytes: files above it are declined before anything is uploaded (default: a sixth of the free device memory; a file is not
    streamed in pieces).  Raises ReadsDeviceError for what _DECLINED lists."""
    res = _read_uploaded(path, names, device, sequences, titles, max_bytes, keep, table_capacity)
    if isinstance(res, ReadsDeviceError):
        raise res       # from here: the traceback of a decline holds no frame with the reader's device tensors, so a kept error pins none
    return res


def _read_uploaded(path, names, device, sequences, titles, max_bytes, keep, table_capacity):
    """read_reads_device's work.  What is declined once the bytes are on the device is RETURNED as a ReadsDeviceError, not raised."""
    from .ops import _on, _ptr, _stream
    kind_of_file = reads_file_type(path)
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    names = list(names)
    R = len(names)
    data = load_within(path, max_bytes, device, lambda sizes: ReadsDeviceError(path, 0, f"{_DECLINED[8]} {sizes}"))
    lib = _lib.load()
    i64 = dict(dtype=torch.int64, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    tok = tokenise(data, device)
    buf, n, ls, ff, L, err, first_bad = tok.buf, tok.n, tok.ls, tok.ff, tok.L, tok.err, tok.first_bad
    res = DeviceReads(str(path), R)
    line_args = tok.line_args(with_line_starts=True)
    if kind_of_file == "fasta":
        stride = 4
        kind = torch.zeros(L, **i32)
        lrec = torch.zeros(L, 4, **i64)
        line_id = torch.arange(L, **i64)
        first_header = (torch.where(buf[ls] == 62, line_id, line_id.new_full((), L)).min() if L else line_id.new_zeros(())).reshape(1)
        with _on(device):
            _lib.check(lib.gnnome_reads_records_fasta(*line_args, _ptr(first_header), _ptr(kind), _ptr(lrec), _ptr(err), _ptr(first_bad),
                                                      _stream(device)), "reads_records_fasta")
        header = kind == 1
        rec_line = torch.nonzero(header).squeeze(1)
        s_line = torch.nonzero((kind == 2) & (torch.cumsum(header.long(), 0) > 0)).squeeze(1)   # lines above the first header: no record's
        rec = lrec[rec_line].contiguous()
        K = int(rec_line.numel())
        seq_first = torch.cat([torch.searchsorted(s_line, rec_line), s_line.new_tensor([int(s_line.numel())])])
        item_beg, item_len = lrec[s_line, 0], lrec[s_line, 1] - lrec[s_line, 0]
    else:
        stride = 6
        nonblank = torch.nonzero(ff[1:] > ff[:-1]).squeeze(1).contiguous()
        Q = int(nonblank.numel())
        K = (Q + 3) // 4
        rec = torch.zeros(K, 6, **i64)
        rec_line = nonblank[0::4].contiguous()
        if Q:
            with _on(device):
                _lib.check(lib.gnnome_reads_records_fastq(*line_args, _ptr(nonblank), Q, _ptr(rec), _ptr(err), _ptr(first_bad), _stream(device)),
                           "reads_records_fastq")
        seq_first = torch.arange(K + 1, **i64)
        item_beg, item_len = rec[:, 4], rec[:, 5] - rec[:, 4]
    res.num_records, res._buf, res._rec = K, buf, rec
    res.last, full = lookup_names(lib, tok, names, rec, stride, K, table_capacity)   # every record's id looked up among the wanted names
    if titles:
        res.ann = torch.zeros(R, 4, **i64)
        res.missing = torch.full((R,), 15, **i32)
        with _on(device):
            _lib.check(lib.gnnome_reads_annotations(_ptr(buf), n, _ptr(rec), stride, K, _ptr(rec_line), _ptr(res.last), R, _ptr(res.ann),
                                                    _ptr(res.missing), _ptr(err), L, _ptr(first_bad), _stream(device)), "reads_annotations")
    found, (table_full,) = first_decline(tok, 5, 6, extra_scalars=(full,))
    if found is not None:
        return ReadsDeviceError(path, found[0] + 1, _DECLINED.get(found[1], f"code {found[1]}"))
    if table_full:
        return ReadsDeviceError(path, 0, _DECLINED[7])
    if sequences:
        keep_dev = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep, dtype=bool)).to(device)
        src_beg, lengths, first = pack_items(res.last, keep_dev, seq_first, item_beg, item_len)
        res.data, item_off = pack(lib, buf, src_beg, lengths, device)
        res.off = item_off[first]
    return res


def read_store_arrays(path, ids, mask, device):
    """ReadStore.from_reads_file(parser="device"): (data, off) of the reads `ids` (mask: bool numpy over them, or None), or the host
    path's KeyError for the first kept read that the file does not hold."""
    res = read_reads_device(path, ids, device=device, sequences=True, keep=mask)
    absent = res.last < 0
    if mask is not None:
        absent = absent & torch.from_numpy(mask).to(absent.device)
    gone = torch.nonzero(absent)[:1].cpu().tolist()
    if gone:
        r = gone[0][0]
        raise KeyError(f"read {ids[r]!r} (node {2 * r}) is not in {path}")
    return res.data, res.off


def wanted_reads(node_to_read, num_nodes):
    """read_gfa's node_to_read -> (names, owner int64 numpy, sign int64 numpy, num_segments): one entry per read a segment is made of -
    the segment's own name, or the (read, orientation) pairs of its A lines, in A-line order."""
    values = [node_to_read[k] for k in range(0, int(num_nodes), 2)]
    entries = [e for v in values for e in (v if isinstance(v, list) else ((v, "+"),))]
    count = np.fromiter((len(v) if isinstance(v, list) else 1 for v in values), dtype=np.int64, count=len(values))
    sign = np.fromiter((1 if e[1] == "+" else -1 for e in entries), dtype=np.int64, count=len(entries))
    return [e[0] for e in entries], np.repeat(np.arange(len(values), dtype=np.int64), count), sign, len(values)


def node_annotations_device(node_to_read, num_nodes, reads_path, device=None):
    """gfa._node_annotations on the device: read_strand, read_start, read_end, read_chr int64[N] on the CPU, or the host path's
    ValueError (identical text) for the first node - or A-line read within it - that the file does not hold or whose title lacks a
    field; the title for the message is fetched from the device for that one record."""
    names, owner, sign, S = wanted_reads(node_to_read, num_nodes)
    res = read_reads_device(reads_path, names, device=device, sequences=False, titles=True)
    dev = res.last.device
    count = np.bincount(owner, minlength=S) if S else np.zeros(0, dtype=np.int64)
    empty = np.flatnonzero(count == 0)
    bad = torch.nonzero((res.last < 0) | (res.missing != 0))[:1].cpu().tolist()
    if bad and (empty.size == 0 or owner[bad[0][0]] < empty[0]):
        i = bad[0][0]
        k, miss = int(res.last[i]), int(res.missing[i])
        if k < 0:
            raise ValueError(f"read {names[i]!r} is not in {reads_path}")
        lacking = [name for bit, name in enumerate(_FIELDS) if miss >> bit & 1]
        raise ValueError(f"read {names[i]!r} in {reads_path}: the title {record_title(res, k)!r} has no {', '.join(lacking)} field")
    if empty.size:
        raise ValueError(f"unitig node {2 * int(empty[0])}: no A lines name its reads, so it has no position in {reads_path}")
    seg = combine_annotations(torch.from_numpy(owner).to(dev), torch.from_numpy(sign).to(dev), res.ann, S)
    cols = torch.repeat_interleave(seg, 2, dim=0)
    cols[1::2, 0] = -cols[1::2, 0]
    cols = cols.cpu()
    return [cols[:, j].contiguous() for j in range(4)]
