"""The front end the device text readers share (gfa.py, reads.py, maf.py; csrc/text_fields.h is its counterpart in the kernels): the
file's bytes to the device (load_within, tokenise), the wanted-names table (lookup_names) and the one rule for which decline a file is
reported with (first_decline).  A reader supplies its line kernel over Tokens.line_args(), a _DECLINED table of what its codes mean,
the two codes it gives the byte-level findings and a DeviceDecline subclass ("The device text readers, what they share")."""
import gzip
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib

_NONZERO_CHUNK = 1 << 30
_MEMORY_SHARE = 6    # default max_bytes = free device memory / 6: the bytes, their marks, one mask and the int64 positions of the compactions
_INT64_MAX, _INT32_MAX = torch.iinfo(torch.int64).max, torch.iinfo(torch.int32).max


class DeviceDecline(ValueError):
    """A device reader declines the file: .line (1-based; 0 where no line is at fault) and .reason.  A subclass names, in SERVED_BY, the
    reader and what serves the file instead."""
    SERVED_BY = "the device reader"

    def __init__(self, path, line, reason):
        where = f"line {line}: " if line else ""
        super().__init__(f"{path}: {where}{reason} - not served by {self.SERVED_BY}")
        self.line, self.reason = line, reason


def read_bytes(path):
    """The file's bytes as uint8 numpy; .gz is decompressed on the host."""
    if str(path).endswith(".gz"):
        with gzip.open(path, "rb") as f:
            return np.frombuffer(f.read(), dtype=np.uint8).copy()
    with open(path, "rb") as f:
        data = np.empty(os.fstat(f.fileno()).st_size, dtype=np.uint8)
        got = 0
        while got < data.size:
            k = f.readinto(memoryview(data)[got:])
            if not k:
                break
            got += k
        return data[:got]


def load_within(path, max_bytes, device, decline):
    """read_bytes(path), or raise decline("(<size> > <max_bytes>)") - the reader's own error - for a file above max_bytes (None: a
    sixth of the device's free memory): before it is read where its size is known without reading (not .gz), before the upload otherwise."""
    if max_bytes is None:
        max_bytes = torch.cuda.mem_get_info(device)[0] // _MEMORY_SHARE
    if not str(path).endswith(".gz") and os.path.getsize(path) > max_bytes:
        raise decline(f"({os.path.getsize(path)} > {max_bytes})")
    data = read_bytes(path)
    if data.size > max_bytes:
        raise decline(f"({data.size} > {max_bytes})")
    return data


def positions(marks, bit):
    """int64 positions of the bytes that carry `bit`, in rising order (nonzero in pieces: a file may exceed 2^31 bytes)."""
    n = int(marks.numel())
    parts = [torch.nonzero(marks[a:a + _NONZERO_CHUNK] & bit).squeeze(1) + a for a in range(0, n, _NONZERO_CHUNK)]
    return parts[0] if len(parts) == 1 else torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=marks.device)


class Tokens(namedtuple("Tokens", "buf n fs fe ls ff F L bad_pos first_bad err")):
    """tokenise's result, tensors on the device: field k (of F) is buf[fs[k] : fe[k] + 1], line l (of L) starts at byte ls[l] and owns
    the fields ff[l] : ff[l + 1]; bad_pos int64[2] the first byte >= 0x80 and the first '\\r' that no '\\n' follows (int64 max: none);
    err int32[max(L, 1)] zeros and first_bad int32[1] int32 max, for the line kernels to leave their codes in."""

    def line_args(self, with_line_starts=False):
        """The leading arguments of a line kernel's entry point: buf, n, fs, fe, F, ff, [ls,] L."""
        from .ops import _ptr
        return (_ptr(self.buf), self.n, _ptr(self.fs), _ptr(self.fe), self.F, _ptr(self.ff), *([_ptr(self.ls)] if with_line_starts else []), self.L)


def tokenise(data, device):
    """uint8 bytes (numpy or tensor) -> Tokens on `device`: one upload, gnnome_gfa_mark over the bytes, its marks compacted (one
    synchronisation each for the field starts, the field ends and the line starts) and freed."""
    from .ops import _on, _ptr, _stream
    lib = _lib.load()
    buf = (torch.from_numpy(data) if isinstance(data, np.ndarray) else data).to(device).contiguous()
    n = int(buf.numel())
    marks = torch.empty(n, dtype=torch.uint8, device=device)
    bad_pos = torch.full((2,), _INT64_MAX, dtype=torch.int64, device=device)
    first_bad = torch.full((1,), _INT32_MAX, dtype=torch.int32, device=device)
    with _on(device):
        _lib.check(lib.gnnome_gfa_mark(_ptr(buf), n, _ptr(marks), _ptr(bad_pos), _stream(device)), "gfa_mark")
    fs, fe, ls = positions(marks, 1), positions(marks, 2), positions(marks, 4)
    del marks
    F, L = int(fs.numel()), int(ls.numel())
    ff = torch.empty(L + 1, dtype=torch.int64, device=device)
    ff[:L] = torch.searchsorted(fs, ls)
    ff[L] = F
    return Tokens(buf, n, fs, fe, ls, ff, F, L, bad_pos, first_bad, torch.zeros(max(L, 1), dtype=torch.int32, device=device))


def pack(lib, src, src_beg, lengths, device):
    """(uint8[total], int64[R+1]): src[src_beg[r] : src_beg[r] + lengths[r]] for every r, concatenated (gnnome_gfa_pack)."""
    from .ops import _on, _ptr, _stream
    R = int(lengths.numel())
    off = torch.zeros(R + 1, dtype=torch.int64, device=device)
    torch.cumsum(lengths, 0, out=off[1:])
    total = int(off[-1]) if R else 0
    out = torch.empty(total, dtype=torch.uint8, device=device)
    src_beg = src_beg.contiguous()
    if total:
        with _on(device):
            _lib.check(lib.gnnome_gfa_pack(_ptr(src), int(src.numel()), _ptr(src_beg), _ptr(off), R, _ptr(out), total, _stream(device)),
                       "gfa_pack")
    return out, off


def texts(lib, buf, beg, end, device):
    """The fields [beg, end) as a list of str: one blob, the fields joined by '\\n', one copy to the host, one split."""
    k = int(beg.numel())
    if k == 0:
        return []
    blob, off = pack(lib, buf, beg, end - beg + 1, device)   # one byte more than the field: the whitespace behind it
    blob[off[1:] - 1] = 10
    return blob.cpu().numpy().tobytes().decode("ascii").split("\n")[:-1]


def pack_names(names):
    """list of str -> (uint8 numpy, int64[R+1] numpy): the names one after the other.  A name that is not ASCII cannot be in a file a
    device reader serves; it is encoded as UTF-8 and simply matches nothing."""
    blob = "".join(names)
    try:
        raw = blob.encode("ascii")
        lengths = np.fromiter(map(len, names), dtype=np.int64, count=len(names))
    except UnicodeEncodeError:
        enc = [s.encode("utf-8") for s in names]
        raw = b"".join(enc)
        lengths = np.fromiter(map(len, enc), dtype=np.int64, count=len(enc))
    off = np.zeros(len(names) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return np.frombuffer(raw, dtype=np.uint8).copy(), off


def lookup_names(lib, tok, names, rec, stride, num_records, table_capacity=None):
    """The wanted `names` (list of str; a repeated name is legal) into an open-addressing table of table_capacity slots (a power of two,
    default above 2 R) and every record's id - tok.buf[rec[k, 0] : rec[k, 1]], rec int64[num_records, stride] - looked up in it: the last
    record of an id wins.  -> (last int64[R]: the record of names[r] or -1; full int32[1]: nonzero when the table had no room)."""
    from .ops import _on, _ptr, _stream
    device = tok.buf.device
    R = len(names)
    name_bytes, name_off = pack_names(names)
    cap = int(table_capacity) if table_capacity is not None else max(2, 1 << (2 * R).bit_length())
    names_dev, off_dev = torch.from_numpy(name_bytes).to(device), torch.from_numpy(name_off).to(device)
    i32 = dict(dtype=torch.int32, device=device)
    table = torch.full((cap,), -1, **i32)
    match = torch.full((cap,), -1, **i32)
    slot_of = torch.full((R,), -1, **i32)
    full = torch.zeros(1, **i32)
    name_args = (_ptr(names_dev), int(names_dev.numel()), _ptr(off_dev), R, _ptr(table), cap)
    with _on(device):
        _lib.check(lib.gnnome_reads_names_insert(*name_args, _ptr(slot_of), _ptr(full), _stream(device)), "reads_names_insert")
        _lib.check(lib.gnnome_reads_match(_ptr(tok.buf), tok.n, _ptr(rec), stride, num_records, *name_args, _ptr(match), _stream(device)),
                   "reads_match")
    slot = slot_of.long()
    return (torch.where(slot >= 0, match[slot.clamp(min=0)].long(), slot) if R else slot), full


def choose_decline(byte_level, line_level, extra=()):
    """Which finding a file is declined with, from plain ints: -> (line, code), line 0-based, or None without a finding.  byte_level: the
    (line, code) pairs of the tokeniser's findings (rank 0); line_level: (line, code) of the earliest line a kernel flagged, or None
    (rank 1); extra: a reader's own (line, rank, code) candidates, rank >= 2.  The smallest (line, rank, code) wins."""
    cands = [(line, 0, code) for line, code in byte_level]
    if line_level is not None:
        cands.append((line_level[0], 1, line_level[1]))
    cands += extra
    return min(cands)[::2] if cands else None


def first_decline(tok, hi_code, cr_code, extra_scalars=(), extra_candidates=None):
    """The one synchronisation that reports: tok.first_bad, tok.bad_pos and the reader's own `extra_scalars` (one-element integer
    tensors) in ONE device-to-host copy (only a file with a finding pays for more: the line of a byte position, the flagged line's code).
    -> (choose_decline's answer, the extra scalars as ints).  hi_code / cr_code: the reader's codes for a byte >= 0x80 and a bare carriage
    return; extra_candidates(*the extra ints) -> the reader's own (line, rank, code) candidates."""
    bad_line, hi_pos, cr_pos, *extra = torch.cat([tok.first_bad.long(), tok.bad_pos, *(s.reshape(1).long() for s in extra_scalars)]).cpu().tolist()
    byte_level = [(int(torch.searchsorted(tok.ls, tok.ls.new_tensor([pos]), right=True)) - 1, code)
                  for pos, code in ((hi_pos, hi_code), (cr_pos, cr_code)) if pos != _INT64_MAX]
    line_level = (bad_line, int(tok.err[bad_line])) if bad_line != _INT32_MAX else None
    return choose_decline(byte_level, line_level, extra_candidates(*extra) if extra_candidates else ()), extra
