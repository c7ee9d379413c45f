"""A seeded generator of MAF texts in pbsim3's layout (gnnome_amd/maf.py states what is read from one), with the truth the generator
itself put in: the blocks, the wanted-name lists and their rows, small GFAs that name the reads, and the FASTA generate_data.py:53-56
would write from the same blocks.  A helper, not a test file: tests/test_maf_statement.py holds the host statement to it,
tests/test_maf_device.py uses it on the GPU.

What a served file varies.  Text lengths 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097 and 5003 columns (the vector-load, wavefront and
tokeniser-tile edges), and a read text that is all '-' with size 0 (an s line has 7 fields, so the shortest text that says "size 0" is a
run of dashes); the text's first byte at every offset modulo 16 (the padding in front of it is cycled); dashes at the first byte, at the
last byte, in runs, and none at all.  Layout: `a` bare and with score=, `##maf` and `track` lines, '#' comments between blocks and inside
one, blank and whitespace-only separators, two blocks with no blank line between them, CRLF, no final newline, a last block without a
blank line.  Fields: tabs and runs of spaces, 18-digit starts, '-' on the read line, '-' on the reference line (its start is taken as
written).  Reads: repeated ids with other positions (the last wins), blocks nobody wants, wanted names with and without the _chr{N}
suffix, wanted names without a block.

bad_case(name): one file per declined or raising case, with the 1-based line at fault."""
import numpy as np

from reads_statement import _gfas

LENGTHS = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 5003)
_SHORT = (1, 15, 16, 17, 63, 64, 65)
_BASES = "ACGT"
_SEPS = (" ", "\t", "  ", " \t ", "     ")
_BLANKS = ("", "", " ", "\t", " \t ", "\x0b", "\x0c \x1c")
_CHRS = ("chr21", 7, "X", "chrY", "M", "3", "chr1", 22)
_CODES = {"X": -1, "Y": -2, "M": -3}


def chr_code(chr):
    """(code, spelling) of a `chr` argument, restated here: an int, or a str with or without 'chr' in front; X, Y, M -> -1, -2, -3."""
    spelling = str(chr)[3:] if str(chr).startswith("chr") else str(chr)
    return (_CODES[spelling] if spelling in _CODES else int(spelling)), spelling


def _bases(rng, n):
    return "".join(_BASES[c] for c in rng.integers(0, 4, size=n))


def _alignment(rng, columns, dashes):
    """Two texts of `columns` bytes each: (reference text, read text); no column is '-' in both."""
    ref, read = list(_bases(rng, columns)), list(_bases(rng, columns))
    if dashes == "all":                              # the read line says size 0
        return "".join(ref), "-" * columns
    if dashes == "first":
        ref[0] = "-"
    elif dashes == "last":
        read[-1] = "-"
    elif dashes == "runs":
        k = 0
        while k < columns:
            run = int(rng.integers(1, 20))
            who = int(rng.integers(0, 4))            # 0, 1: none; 2: the reference; 3: the read
            if who >= 2:
                (ref if who == 2 else read)[k:k + run] = "-" * len(ref[k:k + run])
            k += run
    return "".join(ref), "".join(read)


def _block(rng, rid, columns, dashes, pad, eighteen=False):
    """-> (lines of the block without its a line, (id, strand, start, end))."""
    ref, read = _alignment(rng, columns, dashes)
    ref_size, read_size = columns - ref.count("-"), columns - read.count("-")
    start = int(rng.integers(10 ** 17, 10 ** 18 - 10 ** 6)) if eighteen else int(rng.integers(0, 10 ** int(rng.integers(1, 9))))
    strand, ref_strand = "+-"[int(rng.integers(0, 2))], "+-"[int(rng.integers(0, 4)) == 0]
    sep = lambda: _SEPS[int(rng.integers(0, len(_SEPS)))]   # noqa: E731
    src = 10 ** 18 - 1 if eighteen else 248956422
    lines = [f"s{sep()}ref{sep()}{start}{sep()}{ref_size}{sep()}{ref_strand}{sep()}{src}{' ' * pad}{ref}",
             f"s{sep()}{rid}{sep()}0{sep()}{read_size}{sep()}{strand}{sep()}{read_size}{' ' * (1 + (pad * 7) % 16)}{read}"]
    return lines, (rid, 1 if strand == "+" else -1, start, start + ref_size)


def _suffixed(gfa_text, wanted, suffix):
    """The GFA with `suffix` appended to every wanted read's name (S, A and L lines), as a graph built from the rewritten FASTA has it."""
    out = []
    for line in gfa_text.splitlines():
        f = line.split("\t")
        for k in {"S": (1,), "A": (4,), "L": (1, 3)}.get(f[0], ()):
            if f[k] in wanted:
                f[k] += suffix
        out.append("\t".join(f))
    return "\n".join(out) + "\n"


def maf_case(seed, chr=None):
    """-> dict(text bytes; chr; code, spelling; blocks [(id, strand, start, end)] in file order; reads {id: (strand, start, end)} (the
    last block of an id); block_of {id: index}; names, ann, last: a wanted-name list with the rows read_maf_annotations owes for it;
    gfa_plain, gfa_utg: GFAs over bare read names; gfa_plain_chr, gfa_utg_chr: the same with the _chr{N} suffix on every read;
    fasta, fasta_bare: the FASTA of generate_data.py:53-56 (ids with the suffix) and the same with the ids left bare; text_offsets: the
    file offset of every text's first byte)."""
    rng = np.random.default_rng(5000 + seed)
    chr = _CHRS[seed % len(_CHRS)] if chr is None else chr
    code, spelling = chr_code(chr)
    eol = "\r\n" if seed % 5 == 3 else "\n"
    n_blocks = int(rng.integers(8, 20))
    long_at = int(rng.integers(0, n_blocks))
    out, blocks = [], []
    if seed % 2 == 0:
        out.append("##maf version=1 scoring=none")
    if seed % 3 == 0:
        out += ["track name=sim description=\"simulated reads\"", "# pbsim3-style output"]
    for b in range(n_blocks):
        rid = f"S{1 + seed % 3}_{b + 1}"
        roll = rng.random()
        if b and roll < 0.2:
            rid = blocks[int(rng.integers(0, b))][0]                     # a repeated id: other position
        columns = LENGTHS[7 + (seed + b) % 4] if b == long_at else _SHORT[(seed + b) % len(_SHORT)]
        dashes = ("none", "first", "last", "runs", "all")[(seed + 2 * b) % 5]
        lines, truth = _block(rng, rid, columns, dashes, pad=1 + (seed + b) % 16, eighteen=rng.random() < 0.15)
        out.append("a" if rng.random() < 0.5 else f"a score={int(rng.integers(0, 99999))}.0")
        if rng.random() < 0.1:
            lines.insert(1, "# a comment inside a block changes nothing")
        out += lines
        blocks.append(truth)
        last_one = b == n_blocks - 1
        if last_one and seed % 3 != 1:
            continue                                                      # the last block without a blank line
        if not last_one and rng.random() < 0.25:
            continue                                                      # closed by the next a line
        out.append(_BLANKS[int(rng.integers(0, len(_BLANKS)))])
        if rng.random() < 0.2:
            out.append(("", "# between blocks")[int(rng.integers(0, 2))])
    text = eol.join(out) + ("" if seed % 4 == 2 else eol)
    reads = {rid: (strand, start, end) for rid, strand, start, end in blocks}
    block_of = {rid: b for b, (rid, *_) in enumerate(blocks)}
    ids = list(reads)
    wanted = [ids[k] for k in rng.permutation(len(ids))][:max(2, len(ids) - 2)]      # the rest: blocks nobody wants
    suffix = f"_chr{spelling}"
    names = [nm + suffix if rng.random() < 0.5 else nm for nm in wanted]
    names.insert(int(rng.integers(0, len(names) + 1)), names[0])         # two nodes may name one read
    names += [f"S9_{seed}", f"S9_{seed}{suffix}", wanted[0] + "_chr", wanted[0][:-1] + "x"]   # no block has these
    bare = [nm[:-len(suffix)] if nm.endswith(suffix) else nm for nm in names]
    ann = [[*reads[nm], code] if nm in reads else [0, 0, 0, 0] for nm in bare]
    last = [block_of.get(nm, -1) for nm in bare]
    lengths = {r: 9 for r in wanted}
    plain, utg = _gfas(rng, wanted, lengths)
    fasta = lambda sfx: "".join(f">{rid}{sfx} strand={'+' if s > 0 else '-'} start={a} end={e} chr={spelling}\nACGTACGTA\n"   # noqa: E731
                                for rid, (s, a, e) in reads.items())
    offsets = []
    pos = 0
    for line in text.split("\n"):
        if line.split()[:1] == ["s"]:
            offsets.append(pos + len(line.rstrip()) - len(line.split()[6]))
        pos += len(line) + 1
    return {"text": text.encode("ascii"), "chr": chr, "code": code, "spelling": spelling, "blocks": blocks, "reads": reads,
            "block_of": block_of, "wanted": wanted, "names": names, "ann": ann, "last": last, "gfa_plain": plain, "gfa_utg": utg,
            "gfa_plain_chr": _suffixed(plain, set(wanted), suffix), "gfa_utg_chr": _suffixed(utg, set(wanted), suffix),
            "fasta": fasta(suffix), "fasta_bare": fasta(""), "text_offsets": offsets}


_GOOD = ("a score=1.0\ns ref 100 8 + 5000 ACGTACGT\ns S1_1 0 8 + 8 ACGTTCGT\n\n", "a\ns ref 300 4 + 5000 AC-GT\ns S1_3 0 5 - 5 ACTGT\n\n")
# name -> (the middle of the file, the 0-based line at fault within it, the code of maf._DECLINED, whether the host statement raises)
_BAD = {
    "one s line": ("a\ns ref 200 4 + 5000 ACGT\n\n", 0, 7, True),
    "three s lines": ("a\ns ref 200 4 + 5000 ACGT\ns S1_2 0 4 + 4 ACGT\ns S1_2b 0 4 + 4 ACGT\n\n", 3, 7, True),
    "no s line": ("a score=3\n\n", 0, 7, True),
    "6 fields": ("a\ns ref 200 4 + 5000 ACGT\ns S1_2 0 4 + ACGT\n\n", 2, 1, True),
    "8 fields": ("a\ns ref 200 4 + 5000 ACGT extra\ns S1_2 0 4 + 4 ACGT\n\n", 1, 1, True),
    "19 digits": ("a\ns ref 1234567890123456789 4 + 5000 ACGT\ns S1_2 0 4 + 4 ACGT\n\n", 1, 3, False),
    "a sign": ("a\ns ref -4 4 + 5000 ACGT\ns S1_2 0 4 + 4 ACGT\n\n", 1, 2, True),
    "a letter": ("a\ns ref 200 4 + 5000 ACGT\ns S1_2 0 4x + 4 ACGT\n\n", 2, 2, True),
    "a strand": ("a\ns ref 200 4 + 5000 ACGT\ns S1_2 0 4 * 4 ACGT\n\n", 2, 4, True),
    "an i line": ("a\ns ref 200 4 + 5000 ACGT\ns S1_2 0 4 + 4 ACGT\ni S1_2 N 0 C 0\n\n", 3, 5, True),
    "an s line outside a block": ("a\ns ref 200 4 + 5000 ACGT\ns S1_2 0 4 + 4 ACGT\n\ns S1_2 0 4 + 4 ACGT\n\n", 4, 6, True),
    "unequal texts": ("a\ns ref 200 4 + 5000 ACGT\ns S1_2 0 5 + 5 ACGTT\n\n", 2, 8, True),
    "size off by one": ("a\ns ref 200 5 + 5000 AC-GT\ns S1_2 0 5 + 5 ACTGT\n\n", 1, 9, True),
    "size off by one on a long read line": ("a\ns ref 200 4100 + 5000 " + "ACGT" * 1025 + "\ns S1_2 0 4097 + 4097 " + "-A-" + "ACGT" * 1024 + "G\n\n", 2, 9, True),
    "a byte >= 0x80": ("a\ns ref 200 4 + 5000 ACGT\ns café 0 4 + 4 ACGT\n\n", 2, 10, False),
    "a bare carriage return": ("a\ns ref 200 4 + 5000 AC\rGT\ns S1_2 0 4 + 4 ACGT\n\n", 1, 11, True),
}
BAD_CASES = tuple(_BAD)


def bad_case(name):
    """-> dict(text bytes, line: the 1-based line at fault, code: its row of maf._DECLINED, raises: whether the host statement raises
    (False: it reads the file), names, ann, last: what the host owes for `names` with chr 5 where it does not raise)."""
    middle, at, code, raises = _BAD[name]
    text = "##maf version=1\n" + _GOOD[0] + middle + _GOOD[1].rstrip("\n")
    line = 1 + _GOOD[0].count("\n") + at + 1
    names = ["S1_1", "S1_3_chr5", "S1_2"]
    second = {"19 digits": ([1, 1234567890123456789, 1234567890123456793, 5], 1), "a byte >= 0x80": ([0, 0, 0, 0], -1)}.get(name)
    ann = [[1, 100, 108, 5], [-1, 300, 304, 5], second[0] if second else None]
    last = [0, 2, second[1] if second else None]
    return {"text": text.encode("latin-1"), "line": line, "code": code, "raises": raises, "names": names, "ann": ann, "last": last}
