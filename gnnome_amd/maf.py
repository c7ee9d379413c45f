"""The read positions of the training labels from pbsim3's MAF files, on the host (the statement) and on the MI355X
(generate_data.py:43-60, change_description_pbsim; csrc/maf_parse.hip).

    ann, last = read_maf_annotations("sim_0001.maf", names, "chr21")          # int64[R,4] strand, start, end, chromosome; int64[R] block or -1
    cols = node_annotations(g["node_to_read"], g["num_nodes"], "sim_0001.maf", chr="chr21")   # read_strand, read_start, read_end, read_chr
    g = gfa.read_gfa("asm.gfa", training=True, maf="sim_0001.maf", maf_chr="chr21")           # the same four columns, and y

pbsim3 writes a plain FASTQ (S1_1, S1_2, ...) and a MAF with one alignment block per read.  The reference walks the MAF with Biopython's
AlignIO, takes start and size from the reference line and the strand from the read line of every block, and rewrites every read into a
FASTA whose ids get `_chr{N}` appended and whose titles carry `strand= start= end= chr=`; gfa.read_gfa(training=True) reads such titles.
This module is the other way to the same four columns: straight from the MAF, no rewritten FASTA and no Biopython.

What is read (the UCSC MAF layout as pbsim3 writes it):

    a
    s ref   1234 5000 + 248956422 ACGT-ACG...
    s S1_1     0 5011 + 5011      ACGTTACG...
    <blank line>

  * lines end at '\\n' (a '\\r' in front of it is whitespace); fields are separated by whitespace as str.split() takes it in ASCII;
  * a line without a field is blank; a line whose first field begins with '#' (`##maf version=1`) or is `track` is skipped;
  * a block is a line whose first field is `a` (anything behind it is ignored) and the `s` lines that follow it up to the next blank
    line, `a` line or end of file; skipped lines between them change nothing;
  * an `s` line has exactly 7 fields: s, name, start, size, strand, srcSize, text; start, size and srcSize are plain digits, strand is
    `+` or `-`;
  * a block holds exactly two `s` lines (the reference's `ref, read_m = align` raises otherwise), both texts have the same length, and
    each text without its `-` bytes has `size` bytes;
  * anything else - `i` / `e` / `q` lines, an `s` line outside a block, other field counts, signs or letters in a number - raises
    ValueError naming the 1-based line.  Where several lines are at fault the EARLIEST one is named (a block of fewer than two `s` lines
    is at fault on its `a` line, one of more than two on its third `s` line, unequal texts on the second `s` line);
  * per block: read id = the name of the second `s` line; start = the first line's start, as written whatever that line's strand is (as
    the reference takes it); end = start + the first line's size; strand = +1 / -1 from the second line's strand; chr = the caller's;
  * a read id that occurs in several blocks keeps its LAST block (the reference's loop overwrites the description in the same way).

`chr` is an int, or a str such as "chr21", "21", "X", "Y", "M"; X, Y and M become -1, -2, -3 as graph_parser.py:223-228 maps them.  (The
reference's own `int(chr[3:])`, generate_data.py:44, covers only the numeric "chrN" case.)  A wanted name matches a block's id when it is
equal to it or to f"{id}_chr{c}", c being what the caller passed behind "chr" - the suffix the reference appends (generate_data.py:54):
the suffix is stripped from the wanted names before the lookup, so a graph built from the reference's rewritten FASTA and one built from
the raw FASTQ both work.  `maf` may be a list of (path, chr) pairs, the reference's multi-chromosome datasets: a name with a `_chr{c}`
suffix is looked up only in the file given with that c; a name without one must be found in exactly one file (pbsim3 restarts its read
numbering per run, which is why the reference appends the suffix) - found in several, ValueError.

The device reader (parser="device") is a second implementation of this statement and nothing else.  The bytes go to the device once,
textscan.tokenise finds their fields and lines, gnnome_maf_lines reads every line's fields (one thread per line), torch scans group the `s` lines under
the nearest `a` line and check "exactly two" and "equal text lengths", gnnome_maf_text_check counts the bytes of every text that are not
`-` (one wavefront per `s` line: the only pass over the alignment texts), and the wanted names go through textscan.lookup_names
(reads_parse.hip's table, integer atomicMax: the last block of an id wins).  What it cannot serve it declines
(MafDeviceError names the line; _DECLINED lists the cases); parser="auto" then runs the host statement, which returns or raises as it
says.  Synchronisations per file: the three compactions of the tokeniser, the `s`-line and `a`-line lists, and ONE that reports."""
import os
import re

import numpy as np
import torch

from . import _lib
from .gfa import _CHR_CODES
from .reads import combine_annotations, wanted_reads
from .textscan import DeviceDecline, first_decline, load_within, lookup_names, read_bytes, tokenise

# What is at fault in a MAF, by the code left on the line: 1-5 by gnnome_maf_lines, 6-8 by the block scans, 9 by gnnome_maf_text_check.
# The host statement raises ValueError for 1, 2 and 4-9 (3 it reads, Python's ints being as long as they need); the device reader
# declines all of them, and 10 / 11 (gnnome_gfa_mark's byte checks), 12 (the name table) and 13 (decided before the upload) as well.
# 12 and 13 belong to no line: .line is 0.
_DECLINED = {
    1: "an s line without exactly 7 fields (s, name, start, size, strand, srcSize, text)",
    2: "a start, size or srcSize that is not plain digits",
    3: "a number of more than 18 digits",
    4: "a strand other than + or -",
    5: "a line that is neither blank, a comment, a track line, an a line nor an s line",
    6: "an s line outside a block (no a line above it since the last blank line)",
    7: "a block without exactly two s lines",
    8: "two texts of unequal length in one block",
    9: "a text whose bytes other than '-' are not `size` many",
    10: "a byte >= 0x80",
    11: "a carriage return that no line feed follows",
    12: "the name table is full",
    13: "a file above max_bytes",
}
_INT64_MAX = 2 ** 63 - 1
_DIGITS = re.compile(r"[0-9]+")


class MafDeviceError(DeviceDecline):
    """The device reader declines the file: .line (1-based; 0 where no line is at fault) and .reason; the host statement takes any file."""
    SERVED_BY = "the device reader (parser='host' or 'auto')"


def parse_chr(chr):
    """-> (code, spelling): the chromosome as read_chr holds it (graph_parser.py:223-228: a number, or -1 / -2 / -3 for X / Y / M) and
    what the caller wrote behind "chr", which is what the `_chr{...}` suffix of a read id carries (generate_data.py:54)."""
    if isinstance(chr, (int, np.integer)) and not isinstance(chr, bool):
        return int(chr), str(int(chr))
    if not isinstance(chr, str):
        raise ValueError(f"chr={chr!r}: expected an int or a str such as 'chr21', '21', 'X'")
    spelling = chr[3:] if chr.startswith("chr") else chr
    if spelling in _CHR_CODES:
        return _CHR_CODES[spelling], spelling
    if not _DIGITS.fullmatch(spelling):
        raise ValueError(f"chr={chr!r}: neither a number nor X, Y or M (with or without 'chr' in front)")
    return int(spelling), spelling


def _s_line(fields):
    """An s line's fields -> (code, name, start, size, strand, text); code as _DECLINED, 0 where the line is as the statement says."""
    if len(fields) != 7:
        return 1, None, 0, 0, 0, ""
    _, name, start, size, strand, src_size, text = fields
    if not all(_DIGITS.fullmatch(v) for v in (start, size, src_size)):
        return 2, None, 0, 0, 0, ""
    if strand not in ("+", "-"):
        return 4, None, 0, 0, 0, ""
    return 0, name, int(start), int(size), (1 if strand == "+" else -1), text


def read_maf_blocks(path):
    """The host statement: -> (ids, start, end, strand), one entry per alignment block in file order (list of str, three lists of int),
    or ValueError naming the earliest line at fault (see the module docstring)."""
    text = read_bytes(path).tobytes().decode("ascii", "surrogateescape")   # a byte >= 0x80 stays one character and is no whitespace
    faults = []                       # (line index, code, reason)
    blocks, current = [], None        # a block: (its a line, [(line, s-line entry)])
    orphans = []
    for ln, raw in enumerate(text.split("\n")):
        fields = raw.split()
        if not fields:
            current = None
        elif fields[0][0] == "#" or fields[0] == "track":
            continue
        elif fields[0] == "a":
            current = (ln, [])
            blocks.append(current)
        elif fields[0] == "s":
            entry = _s_line(fields)
            if entry[0]:
                faults.append((ln, entry[0], _DECLINED[entry[0]]))
            if current is None:
                faults.append((ln, 6, _DECLINED[6]))
                orphans.append((ln, entry))
            else:
                current[1].append((ln, entry))
        else:
            faults.append((ln, 5, _DECLINED[5] + f" (it begins with {fields[0][:12]!r})"))
    out = ([], [], [], [])
    for a_line, lines in blocks:
        if len(lines) < 2:
            faults.append((a_line, 7, _DECLINED[7] + f" (it has {len(lines)})"))
        faults += [(ln, 7, _DECLINED[7] + " (this is one more)") for ln, _ in lines[2:]]
        if len(lines) == 2 and not lines[0][1][0] and not lines[1][1][0]:
            (_, ref), (ln, read) = lines
            if len(ref[5]) != len(read[5]):
                faults.append((ln, 8, _DECLINED[8] + f" ({len(ref[5])} and {len(read[5])} bytes)"))
            if ref[2] + ref[3] > _INT64_MAX:
                faults.append((lines[0][0], 3, "start + size does not fit 64 bits"))
            for k, v in enumerate((read[1], ref[2], ref[2] + ref[3], read[4])):
                out[k].append(v)
    for ln, entry in [item for _, lines in blocks for item in lines] + orphans:
        if not entry[0] and len(entry[5]) - entry[5].count("-") != entry[3]:
            faults.append((ln, 9, _DECLINED[9] + f" ({len(entry[5]) - entry[5].count('-')} against size {entry[3]})"))
    if faults:
        ln, _, reason = min(faults)
        raise ValueError(f"{path}: line {ln + 1}: {reason}")
    return out


def _host_lookup(path, names):
    """-> (int64[R,3] strand, start, end; int64[R] last) on the CPU for the suffix-free names."""
    ids, start, end, strand = read_maf_blocks(path)
    index = {rid: b for b, rid in enumerate(ids)}            # the last block of an id wins
    last = np.fromiter((index.get(nm, -1) for nm in names), dtype=np.int64, count=len(names))
    cols = np.zeros((len(names), 3), dtype=np.int64)
    if ids:
        table = np.array([strand, start, end], dtype=np.int64).T.reshape(len(ids), 3)
        cols = np.where(last[:, None] >= 0, table[np.maximum(last, 0)], 0)
    return torch.from_numpy(np.ascontiguousarray(cols)), torch.from_numpy(last)


def _flag(err, first_bad, lines, mask, code, num_lines):
    """Code `code` on the lines lines[mask] that carry none yet, first_bad lowered to the smallest of them (no synchronisation)."""
    hit = torch.zeros(num_lines, dtype=torch.bool, device=err.device)
    hit[lines] = mask
    err[:num_lines] = torch.where(hit & (err[:num_lines] == 0), code, err[:num_lines])
    line_id = torch.arange(num_lines, dtype=torch.int32, device=err.device)
    first_bad.copy_(torch.minimum(first_bad, torch.where(hit, line_id, torch.iinfo(torch.int32).max).min().reshape(1)))


def assemble_blocks(kind, rec, err, first_bad):
    """The block scans (torch only: runs on CPU tensors as well).  kind int32[L] and rec int64[L,8] as gnnome_maf_lines writes them, err
    int32[>=L] and first_bad int32[1] as it leaves them (updated in place: codes 6, 7, 8).  -> (block records int64[B,8]: id begin, id
    end of the second s line, start and size of the first, strand of the second, 0, 0, 0 - all 0 for a block at fault; the s lines'
    records int64[S,8]; their lines int64[S])."""
    L = int(kind.numel())
    dev = kind.device
    i64 = dict(dtype=torch.int64, device=dev)
    if L == 0:
        return torch.zeros(0, 8, **i64), torch.zeros(0, 8, **i64), torch.zeros(0, **i64)
    line_id = torch.arange(L, **i64)
    is_a, is_s = kind == 2, kind == 3
    closer = is_a | (kind == 0)
    above = torch.cummax(torch.where(closer, line_id, line_id.new_full((), -1)), 0)[0]     # the nearest a or blank line above
    s_line = torch.nonzero(is_s).squeeze(1)
    a_line = torch.nonzero(is_a).squeeze(1)
    S, B = int(s_line.numel()), int(a_line.numel())
    srec = rec[s_line].contiguous()
    brec = torch.zeros(B, 8, **i64)
    if S == 0:
        if B:
            _flag(err, first_bad, a_line, torch.ones(B, dtype=torch.bool, device=dev), 7, L)
        return brec, srec, s_line
    up = above[s_line]
    owned = (up >= 0) & is_a[up.clamp(min=0)]
    _flag(err, first_bad, s_line, ~owned, 6, L)
    if B == 0:
        return brec, srec, s_line
    block = torch.where(owned, (torch.cumsum(is_a.long(), 0) - 1)[up.clamp(min=0)], up.new_full((), B))   # B: no block's
    count = torch.zeros(B + 1, **i64).scatter_add_(0, block, torch.ones(S, **i64))[:B]
    first = torch.cumsum(count, 0) - count                                    # among the owned s lines
    rank = torch.cumsum(owned.long(), 0) - 1 - torch.cat([first, first.new_zeros(1)])[block]
    idx = torch.arange(S, **i64)
    first_s = torch.zeros(B + 1, **i64).scatter_(0, torch.where(owned & (rank == 0), block, block.new_full((), B)), idx)[:B]
    second_s = torch.zeros(B + 1, **i64).scatter_(0, torch.where(owned & (rank == 1), block, block.new_full((), B)), idx)[:B]
    _flag(err, first_bad, a_line, count < 2, 7, L)
    _flag(err, first_bad, s_line, owned & (rank >= 2), 7, L)
    ref, read = srec[first_s], srec[second_s]
    good = (count == 2) & (ref[:, 7] == 1) & (read[:, 7] == 1)
    _flag(err, first_bad, s_line[second_s], good & ((ref[:, 6] - ref[:, 5]) != (read[:, 6] - read[:, 5])), 8, L)
    brec[:, 0:2] = read[:, 0:2]
    brec[:, 2:4] = ref[:, 2:4]
    brec[:, 4] = read[:, 4]
    brec[~good] = 0
    return brec, srec, s_line


def _device_lookup(path, names, device=None, max_bytes=None, table_capacity=None):
    """-> (int64[R,3] strand, start, end; int64[R] last) on `device` for the suffix-free names, or MafDeviceError for what _DECLINED
    lists.  max_bytes: files above it are declined before anything is uploaded (default: the share of the free device memory that
    reads.read_reads_device uses; a file is not streamed in pieces)."""
    res = _read_uploaded(path, names, device, max_bytes, table_capacity)
    if isinstance(res, MafDeviceError):
        raise res       # from here: the traceback of a decline holds no frame with the reader's device tensors, so a kept error pins none
    return res


def _read_uploaded(path, names, device, max_bytes, table_capacity):
    """_device_lookup's work.  What is declined once the bytes are on the device is RETURNED as a MafDeviceError, not raised."""
    from .ops import _on, _ptr, _stream
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    names = list(names)
    R = len(names)
    data = load_within(path, max_bytes, device, lambda sizes: MafDeviceError(path, 0, f"{_DECLINED[13]} {sizes}"))
    lib = _lib.load()
    i64 = dict(dtype=torch.int64, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    tok = tokenise(data, device)
    buf, n, L, err, first_bad = tok.buf, tok.n, tok.L, tok.err, tok.first_bad
    kind = torch.zeros(L, **i32)
    lrec = torch.zeros(L, 8, **i64)
    with _on(device):
        _lib.check(lib.gnnome_maf_lines(*tok.line_args(), _ptr(kind), _ptr(lrec), _ptr(err), _ptr(first_bad), _stream(device)), "maf_lines")
    brec, srec, s_line = assemble_blocks(kind, lrec, err, first_bad)
    s_line = s_line.contiguous()
    S, B = int(s_line.numel()), int(brec.shape[0])
    with _on(device):
        _lib.check(lib.gnnome_maf_text_check(_ptr(buf), n, _ptr(srec), _ptr(s_line), S, _ptr(err), L, _ptr(first_bad), _stream(device)),
                   "maf_text_check")
    last, full = lookup_names(lib, tok, names, brec, 8, B, table_capacity)   # every block's read id looked up among the wanted names
    found, (table_full,) = first_decline(tok, 10, 11, extra_scalars=(full,))
    if found is not None:
        return MafDeviceError(path, found[0] + 1, _DECLINED.get(found[1], f"code {found[1]}"))
    if table_full:
        return MafDeviceError(path, 0, _DECLINED[12])
    cols = torch.zeros(R, 3, **i64)
    if B and R:
        row = brec[last.clamp(min=0)]
        cols = torch.where((last >= 0)[:, None], torch.stack([row[:, 4], row[:, 2], row[:, 2] + row[:, 3]], 1), cols)
    return cols, last


def _lookup(path, names, parser, device, **device_options):
    if parser not in ("host", "device", "auto"):
        raise ValueError(f"parser={parser!r}: expected 'host', 'device' or 'auto'")
    if parser == "device" or (parser == "auto" and torch.cuda.is_available()):
        try:
            cols, last = _device_lookup(path, names, device=device, **device_options)
            return cols.cpu(), last.cpu()
        except Exception:   # noqa: BLE001 ("auto": whatever the device reader reports, the host statement answers)
            if parser == "device":
                raise
    return _host_lookup(path, names)


def _files(maf, chr):
    """maf, chr -> [(path, chromosome code, spelling)]: one path with the caller's chr, or a list of (path, chr) pairs."""
    if isinstance(maf, (str, os.PathLike)):
        if chr is None:
            raise ValueError("a MAF file needs chr: the chromosome its reads were simulated from (an int, or 'chr21', '21', 'X', ...)")
        return [(str(maf), *parse_chr(chr))]
    if chr is not None:
        raise ValueError("a list of (path, chr) pairs carries its chromosomes; chr must be None")
    files = [(str(p), *parse_chr(c)) for p, c in maf]
    if not files:
        raise ValueError("an empty list of MAF files")
    spellings = [f[2] for f in files]
    if len(set(spellings)) != len(spellings):
        raise ValueError(f"two MAF files for one chromosome: {spellings}")
    return files


def read_maf_annotations(path, names, chr=None, parser="host", device=None, **device_options):
    """-> (ann int64[R,4] strand, start, end, chromosome of every wanted name; last int64[R] its block's index in its file, -1 and a row
    of zeros where no block has the read), CPU tensors.  path: a MAF (plain or .gz) with `chr`, or a list of (path, chr) pairs with chr
    None.  parser: "host" (read_maf_blocks), "device" (csrc/maf_parse.hip; MafDeviceError where it declines) or "auto" (the device when
    there is one, the host statement whenever the device reader reports anything at all).  device_options: max_bytes, table_capacity of
    the device reader.  A name found in more than one file: ValueError (see the module docstring)."""
    files = _files(path, chr)
    names = list(names)
    R = len(names)
    ann, last = torch.zeros(R, 4, dtype=torch.int64), torch.full((R,), -1, dtype=torch.int64)
    routed = {}                                            # name index -> the one file its suffix names
    for f, (_, _, spelling) in enumerate(files):
        suffix = f"_chr{spelling}"
        for r, nm in enumerate(names):
            if nm.endswith(suffix) and r not in routed:
                routed[r] = (f, nm[:-len(suffix)])
    seen = torch.zeros(R, dtype=torch.int64)
    for f, (file_path, code, _) in enumerate(files):
        ask = [r for r in range(R) if routed.get(r, (f,))[0] == f]
        cols, found = _lookup(file_path, [routed[r][1] if r in routed else names[r] for r in ask], parser, device, **device_options)
        ask = torch.tensor(ask, dtype=torch.int64)
        hit = found >= 0
        seen[ask[hit]] += 1
        twice = torch.nonzero(seen > 1)[:1].tolist()
        if twice:
            r = twice[0][0]
            raise ValueError(f"read {names[r]!r} has a block in more than one MAF file ({', '.join(p for p, _, _ in files)}): name it with "
                             f"the _chr suffix of the file it belongs to")
        ann[ask[hit], :3] = cols[hit]
        ann[ask[hit], 3] = code
        last[ask[hit]] = found[hit]
    return ann, last


def node_annotations(node_to_read, num_nodes, maf, chr=None, parser="host", device=None):
    """gfa._node_annotations with a MAF in place of the titles: read_strand, read_start, read_end, read_chr int64[N] on the CPU.  The
    names come from reads.wanted_reads, a unitig with A lines combines its reads through reads.combine_annotations, node 2k + 1 gets the
    negated strand.  ValueError for the first read that no block has, or (the existing text) for a unitig without A lines."""
    names, owner, sign, S = wanted_reads(node_to_read, num_nodes)
    ann, last = read_maf_annotations(maf, names, chr, parser=parser, device=device)
    where = maf if isinstance(maf, (str, os.PathLike)) else ", ".join(str(p) for p, _ in maf)
    count = np.bincount(owner, minlength=S) if S else np.zeros(0, dtype=np.int64)
    empty = np.flatnonzero(count == 0)
    bad = torch.nonzero(last < 0)[:1].tolist()
    if bad and (empty.size == 0 or owner[bad[0][0]] < empty[0]):
        raise ValueError(f"read {names[bad[0][0]]!r} has no alignment block in {where}")
    if empty.size:
        raise ValueError(f"unitig node {2 * int(empty[0])}: no A lines name its reads, so it has no position in {where}")
    seg = combine_annotations(torch.from_numpy(owner), torch.from_numpy(sign), ann, S)
    cols = torch.repeat_interleave(seg, 2, dim=0)
    cols[1::2, 0] = -cols[1::2, 0]
    return [cols[:, j].contiguous() for j in range(4)]
