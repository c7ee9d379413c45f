"""A seeded generator of reads files (FASTA / FASTQ) that the device reader (gnnome_amd/reads.py) must serve, with the ids,
sequences and titles the generator itself put in, the wanted-name lists and small GFAs that name the reads.  A helper, not a test file:
tests/test_reads_statement.py holds it to contigs.read_sequences / read_titles, tests/test_reads_device.py uses it on the GPU.

What a FASTA varies: line widths from 1 to longer than a tokeniser tile, single-line records, blank and whitespace-only lines anywhere,
CRLF, blanks around a line, no final newline, lines above the first header, ' >' sequence-line decoys, '>' alone as a first field, an
empty id, lower case and IUPAC codes, repeated ids with different sequences and titles, records nobody wants.  A FASTQ: four-line
records whose quality lines start with '@' and with '+', '+id' separators, blank lines between and inside records.  Titles: the four
fields in any order, 'xstart=' / 'start=x' style decoys ahead of the real field, a second occurrence that must lose, chr= as numbers,
X, Y and M, 18-digit positions."""
import numpy as np

_BASES = "ACGT"
_IUPAC = "ACGTMRWSYKVHDBNacgtnrymk"
_WIDTHS = (1, 2, 7, 59, 60, 61, 4095, 4096, 4097, 5003)
_BLANKS = ("", "", " ", "\t", " \t ", "\x0b", "\x0c \x1c")


def _seq(rng, n, alphabet=_BASES):
    return "".join(alphabet[c] for c in rng.integers(0, len(alphabet), size=n))


def _title_fields(rng, complete=True):
    """The annotation part of a title: fields in a random order, decoys in front of some, a losing second occurrence behind."""
    start = int(rng.integers(0, 10 ** int(rng.integers(1, 10))))
    if rng.random() < 0.15:
        start = int(rng.integers(10 ** 17, 10 ** 18 - 1000))        # 18 digits
    end = start + int(rng.integers(1, 900))
    chrom = (str(int(rng.integers(1, 23))), "X", "Y", "M", "007")[int(rng.integers(0, 5))]
    fields = [f"strand={'+-'[int(rng.integers(0, 2))]}", f"start={start}", f"end={end}", f"chr={chrom}"]
    decoys = [("strand=? ", "strand= ", "xstrand=- ", "strand=x"), ("start=x ", "start= ", "xstart=7 ", "start=-4"),
              ("end=, ", "end=e5 ", "trend=12 ", "end="), ("chr=Z ", "chr= ", "chr=chr1 ", "xchr=M ")]
    parts = []
    for k in rng.permutation(4):
        if not complete and rng.random() < 0.4:
            continue
        f = fields[k]
        if rng.random() < 0.35:
            f = decoys[k][int(rng.integers(0, 4))] + " " + f
        if rng.random() < 0.25:
            f = f + " " + fields[k][:fields[k].index("=") + 1] + ("9" if k else "-")   # a second occurrence: it must lose
        parts.append(f)
    sep = (" ", ", ", "\t", "  ")[int(rng.integers(0, 4))]
    return sep.join(parts)


def _gfas(rng, wanted, lengths):
    """(plain, utg): S lines with '*' for the wanted reads in a shuffled order, chained by L lines; and the same reads named on the A
    lines of utg* segments (some reads on two segments, some segments of one read, orientation '-' on some) next to plain S lines."""
    order = [wanted[k] for k in rng.permutation(len(wanted))]
    plain = "".join(f"S\t{r}\t*\tLN:i:{lengths[r]}\n" for r in order)
    plain += "".join(f"L\t{a}\t+\t{b}\t{'+-'[int(rng.integers(0, 2))]}\t3M\n" for a, b in zip(order, order[1:]))
    utg, segs, k = "", [], 0
    while k < len(order):
        if rng.random() < 0.3:
            utg += f"S\t{order[k]}\t*\tLN:i:{lengths[order[k]]}\n"
            segs.append(order[k])
            k += 1
            continue
        take = int(rng.integers(1, 5))
        members = order[k:k + take]
        if k and rng.random() < 0.5:
            members = members + [order[int(rng.integers(0, k))]]     # a read that an earlier segment names as well
        name = f"utg{len(segs):06d}l"
        utg += f"S\t{name}\t*\tLN:i:{sum(lengths[r] for r in members)}\n"
        pos = 0
        for r in members:
            utg += f"A\t{name}\t{pos}\t{'+-'[int(rng.integers(0, 2))]}\t{r}\t0\t{lengths[r]}\tid:i:{k}\n"
            pos += lengths[r]
        segs.append(name)
        k += take
    utg += "".join(f"L\t{a}\t+\t{b}\t-\t3M\n" for a, b in zip(segs, segs[1:]))
    return plain, utg


def reads_case(seed, kind=None, records=None):
    """-> dict(kind 'fasta' | 'fastq', suffix, text bytes, sequences {id: bytes}, titles {id: title} (the last record of an id wins),
    wanted (ids a GFA may name: each has a record with a complete title and at least 8 bases), names (a wanted-name list for
    read_reads_device: `wanted` shuffled, one of them twice, the empty id when the file has one), gfa_plain, gfa_utg (str))."""
    rng = np.random.default_rng(1000 + seed)
    kind = kind or ("fasta", "fastq")[seed % 2]
    n_rec = records or int(rng.integers(6, 30))
    eol = "\r\n" if seed % 5 == 3 else "\n"
    ids = [(f"read{k}", f"m64_{seed}/{k * 7}/ccs", f"r{k}.{seed}")[k % 3] for k in range(n_rec)]
    out, sequences, titles, complete_ids = [], {}, {}, {}
    if kind == "fasta" and seed % 3 == 0:
        out += ["ACGT stray words above", "", "NNNN"]                  # above the first header: no record's
    for k in range(n_rec):
        rid = ids[k]
        roll = rng.random() if k else 0.5                                # the first record is always one a GFA may name
        if k and roll < 0.15:
            rid = ids[int(rng.integers(0, k))]                         # a repeated id: other sequence, other title
        unwanted = 0.15 <= roll < 0.3
        complete = not unwanted or rng.random() < 0.5
        words = ("", "len=5 ", "simulated read; ")[int(rng.integers(0, 3))]
        title = f"{rid} {words}{_title_fields(rng, complete)}".rstrip()
        marker = ">" if kind == "fasta" else "@"
        lead = ""
        if kind == "fasta" and roll > 0.9:
            lead = (" ", "\t ")[int(rng.integers(0, 2))]               # '>' alone is the first field: the id is the second
        if kind == "fasta" and k == n_rec // 2 and seed % 6 == 4:
            rid, title, lead, complete = "", "", "", False             # nothing behind the marker: the empty id
        header = marker + lead + title
        full_title = (lead + title).rstrip()
        trail = _BLANKS[int(rng.integers(0, len(_BLANKS)))]
        out.append(header + trail)
        if rng.random() < 0.2:
            out.append(_BLANKS[int(rng.integers(0, len(_BLANKS)))])
        if kind == "fasta":
            n = int(rng.integers(8, 400)) if rng.random() < 0.9 else int(rng.integers(4000, 9000))
            if unwanted and rng.random() < 0.3:
                n = 0
            seq = _seq(rng, n, _IUPAC if rng.random() < 0.3 else _BASES)
            width = n if rng.random() < 0.3 else _WIDTHS[int(rng.integers(0, len(_WIDTHS)))]
            if width == 1 and n > 40:
                width = 2
            lines = [seq[a:a + width] for a in range(0, n, max(width, 1))]
            if lines and rng.random() < 0.2:
                lines.insert(int(rng.integers(0, len(lines) + 1)), ">" + _seq(rng, 5))    # behind a blank: a sequence line, not a header
                lines = [(" " + ln if ln.startswith(">") else ln) for ln in lines]
            body = []
            for ln in lines:
                pad = rng.random()
                body.append((" " + ln + "  ") if pad < 0.1 else ("\t" + ln) if pad < 0.15 else ln)
                if rng.random() < 0.08:
                    body.append(_BLANKS[int(rng.integers(0, len(_BLANKS)))])
            out += body
            seq = "".join(ln.strip() for ln in lines)
        else:
            n = int(rng.integers(8, 400)) if rng.random() < 0.92 else int(rng.integers(4000, 9000))
            seq = _seq(rng, n, _IUPAC if rng.random() < 0.3 else _BASES)
            qual = "".join(chr(c) for c in rng.integers(33, 127, size=n))
            first = rng.random()
            qual = ("@" + qual[1:]) if first < 0.25 else ("+" + qual[1:]) if first < 0.5 else qual
            blank = lambda: [_BLANKS[int(rng.integers(0, len(_BLANKS)))]] if rng.random() < 0.15 else []   # noqa: E731
            out += blank() + [(" " + seq + " ") if rng.random() < 0.1 else seq] + blank()
            out += ["+" + (title.split()[0] if rng.random() < 0.4 else "")] + blank() + [qual + ("  " if rng.random() < 0.1 else "")]
        rid = full_title.split(None, 1)[0] if full_title.strip() else ""
        sequences[rid], titles[rid] = seq.encode("ascii"), full_title
        complete_ids[rid] = complete and len(seq) >= 8 and rid != ""
        if rng.random() < 0.15:
            out += ["", _BLANKS[int(rng.integers(0, len(_BLANKS)))]]
    text = eol.join(out) + ("" if seed % 4 == 2 else eol)
    wanted = [r for r, ok in complete_ids.items() if ok]
    lengths = {r: len(sequences[r]) for r in wanted}
    plain, utg = _gfas(rng, wanted, lengths)
    names = [wanted[k] for k in rng.permutation(len(wanted))]
    names.insert(int(rng.integers(0, len(names) + 1)), names[0])        # two nodes may name one read
    if "" in sequences:
        names.append("")
    suffix = {"fasta": (".fasta", ".fa", ".fna"), "fastq": (".fastq", ".fq", ".fnq")}[kind][seed % 3]
    return {"kind": kind, "suffix": suffix, "text": text.encode("ascii"), "sequences": sequences, "titles": titles, "wanted": wanted,
            "names": names, "gfa_plain": plain, "gfa_utg": utg}
