"""textscan.tokenise (gnnome_gfa_mark and the compaction of its marks) against its statement, written out below: every output with
torch.equal, at the sizes where k_gfa_mark's 16-byte lanes and 4096-byte tiles begin and end."""
import numpy as np
import pytest
import torch

from gnnome_amd import textscan

pytestmark = pytest.mark.gpu

INT64_MAX, INT32_MAX = torch.iinfo(torch.int64).max, torch.iinfo(torch.int32).max
WHITESPACE = frozenset([*range(0x09, 0x0e), *range(0x1c, 0x21)])


def dev():
    return torch.device("cuda", 0)


def statement(data):
    """bytes -> fs, fe, ls, ff (lists), bad_pos [first byte >= 0x80, first '\\r' that no '\\n' follows]."""
    n, padded = len(data), b"\n" + data + b"\n"                        # the byte before the file and the byte after it are '\n'
    ws = [c in WHITESPACE for c in padded]
    fs = [i for i in range(n) if not ws[i + 1] and ws[i]]              # a non-whitespace byte after whitespace
    fe = [i for i in range(n) if not ws[i + 1] and ws[i + 2]]          # a non-whitespace byte before whitespace
    ls = [i for i in range(n) if padded[i] == 10]                      # every byte whose predecessor is '\n', blank lines included
    ff = np.searchsorted(np.array(fs, dtype=np.int64), np.array(ls, dtype=np.int64)).tolist() + [len(fs)]
    hi = [i for i in range(n) if data[i] >= 0x80]
    cr = [i for i in range(n) if data[i] == 13 and padded[i + 2] != 10]
    return fs, fe, ls, ff, [hi[0] if hi else INT64_MAX, cr[0] if cr else INT64_MAX]


def check(tok, data, device_input):
    fs, fe, ls, ff, bad = statement(data)
    i64 = dict(dtype=torch.int64, device=dev())
    assert tok.n == len(data) and tok.F == len(fs) and tok.L == len(ls)
    assert torch.equal(tok.buf, device_input) and tok.buf.is_contiguous()
    for name, want in (("fs", fs), ("fe", fe), ("ls", ls), ("ff", ff), ("bad_pos", bad)):
        got = getattr(tok, name)
        assert got.dtype == torch.int64 and torch.equal(got, torch.tensor(want, **i64)), name
    assert torch.equal(tok.first_bad, torch.tensor([INT32_MAX], dtype=torch.int32, device=dev()))
    assert torch.equal(tok.err, torch.zeros(max(len(ls), 1), dtype=torch.int32, device=dev()))


PATTERN = b"S\tutg1 ACGT\tLN:i:4\n\n\nab\x1ccd \r\nx\n \t\x0b\x0c\x1d\x1e\x1f\nlonger-field-here z\n"


def patterned(n, shift=0):
    reps = (n + shift) // len(PATTERN) + 1
    return (PATTERN * reps)[shift:shift + n]


def with_byte(data, at, value):
    return data[:at] + bytes([value]) + data[at + 1:]


# name -> bytes.  Every size of 1, 15, 16, 17, 31, 32, 33 (a lane of 16 bytes: short, whole, one over; two lanes likewise) and 4095, 4096,
# 4097 (one workgroup's tile of 256 x 16 bytes and the byte on either side of it) occurs at least once.
CASES = {
    "1 a field": b"x",
    "1 a newline": b"\n",
    "1 a carriage return, the file's last byte": b"\r",
    "15 no final newline": patterned(15),
    "15 whitespace only": b" \t\n\n\r\n\x1c\x1d\x1e\x1f \x0b\x0c\n\n",
    "16 a field that ends on the lane boundary": b"a b\n" + b"c" * 12,
    "16 a carriage return ends the lane and the file": patterned(15) + b"\r",
    "17 a bare carriage return ends the first lane": b"e" * 15 + b"\rq",
    "17 a field that ends on byte 15, whitespace on 16": b"a b\n" + b"c" * 12 + b"\n",
    "17 a field across the lane boundary": b"\n\n\n" + b"d" * 14,
    "17 a carriage return on byte 15, its line feed on 16": b"e" * 15 + b"\r\n",
    "31 consecutive blank lines": b"\n\n\nab\n\n\n\n" + patterned(20, 3) + b"\n\n",
    "32 a byte >= 0x80 ends the second lane": with_byte(patterned(32), 31, 0x80),
    "32 whitespace only": b" " * 15 + b"\n" + b"\t" * 16,
    "33 one byte past two lanes": patterned(33, 7),
    "33 a bare carriage return and a high byte": with_byte(with_byte(patterned(33), 20, 0xff), 9, 13),
    "4095": patterned(4095, 5),
    "4096 a field that ends the tile": patterned(4090) + b" fffff",
    "4096 a line that starts the next tile's first byte": patterned(4095, 11) + b"\n",
    "4097 a line start on the second tile's first byte": patterned(4095) + b"\ng",
    "4097 a field across the tile boundary, its last byte >= 0x80": with_byte(patterned(4089) + b" hhhhhhh", 4096, 0xc3),
    "4097 a carriage return ends the tile, no line feed follows": patterned(4095) + b"\rk",
}


def test_the_cases_cover_the_sizes():
    assert {len(d) for d in CASES.values()} == {1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097}
    assert all(name.split()[0] == str(len(d)) for name, d in CASES.items())


@pytest.mark.parametrize("name", list(CASES))
def test_tokenise_is_its_statement(name):
    data = CASES[name]
    array = np.frombuffer(data, dtype=np.uint8).copy()
    check(textscan.tokenise(array, dev()), data, torch.from_numpy(array).to(dev()))


def test_an_unaligned_buffer_takes_the_bytewise_path():
    data = CASES["33 a bare carriage return and a high byte"]
    whole = torch.from_numpy(np.frombuffer(b"\n" + data, dtype=np.uint8).copy()).to(dev())
    sliced = whole[1:]
    assert sliced.data_ptr() % 16 == 1 and sliced.is_contiguous()
    tok = textscan.tokenise(sliced, dev())
    assert tok.buf.data_ptr() == sliced.data_ptr()      # the bytes are tokenised where they lie
    check(tok, data, sliced)
