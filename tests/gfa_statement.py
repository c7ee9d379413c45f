"""Helpers of the device GFA parser's tests (not a test): a generator of adversarial GFA text from a seed, and read_gfa's line loop
(gnnome_amd/gfa.py) restated as EVENT ARRAYS - (u, v, overlap, tag) per inserted pair in file order, without the adjacency dicts -
which gfa.assemble_edges must turn into read_gfa's edges."""
import math
import re

import numpy as np
import torch

_HIFIASM_ID = re.compile(r"(.*):\d-\d*")
_TAG_TEXTS = ("1e-3", "0.30000001", "1", "0.999", ".5", "9.5E-1", "+0.25", "0.123456789012345678")


def gfa_events(path):
    """-> (u, v, overlap int64[T], tag float64[T] (NaN: the line has no SI:f: field), num_nodes): line j's (sr, dr) then (sv, dv)."""
    names, u, v, ol, tag = {}, [], [], [], []
    with open(path, "rt") as f:
        for raw in f.readlines():
            line = raw.strip().split()
            if not line:
                continue
            if line[0] == "S":
                names[line[1]] = len(names)
            elif line[0] == "L":
                tags = []
                if len(line) >= 6 and any(t.startswith("SI:f:") for t in line[6:]):
                    tags = [t for t in line[6:] if t.startswith("SI:f:")]
                    line = [t for t in line if not t.startswith("SI:f:")]
                assert len(line) in (6, 7, 8)
                id1, o1, id2, o2, cigar = line[1:6]
                if len(line) == 7:
                    id1, id2 = _HIFIASM_ID.findall(id1)[0], _HIFIASM_ID.findall(id2)[0]
                n = int(cigar[:-1])
                if n == 0:
                    continue
                a, b = names[id1], names[id2]
                if o1 == "+" and o2 == "+":
                    ev = (2 * a, 2 * b, 2 * b + 1, 2 * a + 1)
                elif o1 == "+" and o2 == "-":
                    ev = (2 * a, 2 * b + 1, 2 * b, 2 * a + 1)
                elif o1 == "-" and o2 == "+":
                    ev = (2 * a + 1, 2 * b, 2 * b + 1, 2 * a)
                else:
                    ev = (2 * a + 1, 2 * b + 1, 2 * b, 2 * a)
                t = float(tags[0][5:]) if tags else math.nan
                u += [ev[0], ev[2]]
                v += [ev[1], ev[3]]
                ol += [n, n]
                tag += [t, t]
    i64 = torch.int64
    return (torch.tensor(u, dtype=i64), torch.tensor(v, dtype=i64), torch.tensor(ol, dtype=i64), torch.tensor(tag, dtype=torch.float64),
            2 * len(names))


def adversarial_gfa(seed, tags="all", sequences=True):
    """GFA text (ASCII str) that read_gfa accepts, mixing what a tokeniser and the edge rules can get wrong: tabs and runs of blanks
    (and 0x0b, 0x0c, 0x1c-0x1f) as separators, CRLF, blank and blank-only lines, no final newline; 6-, 7- and 8-field links; hifiasm
    names that hold ':<digit>-' twice; zero overlaps; a pair inserted three times with different overlaps, from both of its events'
    orders; links whose two events are one pair (a + a -); orientation fields that are neither + nor -; utg segments with A runs, one
    cut by a blank line, and stray A lines; names that are prefixes of one another.  tags: "all" (every link carries SI:f:), "all_but_one",
    "none".  sequences=False writes '*'."""
    rng = np.random.default_rng(seed)
    seps = ["\t", "\t", "\t", " ", "  ", " \t ", "\x0b", "\x0c\t", "\x1c", "\x1d\x1e", "\x1f "]

    def join(fields):
        return "".join(f + (seps[rng.integers(len(seps))] if k + 1 < len(fields) else "") for k, f in enumerate(fields))

    def end():
        return ["\n", "\n", "\r\n", " \n", "\t\r\n"][rng.integers(5)]

    R = int(rng.integers(12, 30))
    base = ["r1", "r10", "r100", "r1a", "x", "xx", "xxx", "ab:3-x", "ab:3-", "q:1-2:3-4", "utg1", "utg10", "utg000003l", "ut", "utgx"]
    names = base[:min(R, len(base))] + [f"read{k}" for k in range(R - len(base))]
    names = [names[k] for k in rng.permutation(len(names))]
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, size=int(rng.integers(24, 70)))) for _ in names]
    lines = []
    n_links = int(rng.integers(30, 60))
    links = []
    tag_k = 0

    def link(i, j, o1, o2, n, fields):
        nonlocal tag_k
        a, b = names[i], names[j]
        if fields == 7:
            a, b = f"{a}:{rng.integers(10)}-{rng.integers(300)}", f"{b}:{rng.integers(10)}-"
        row = ["L", a, o1, b, o2, f"{n}M"] + ["L1:i:7", "L2:i:9"][:fields - 6]
        tag = f"SI:f:{_TAG_TEXTS[tag_k % len(_TAG_TEXTS)]}"
        tag_k += 1
        if fields > 6 and rng.random() < 0.5:
            row.insert(6, tag)      # the tag in front of the optional fields
            if rng.random() < 0.3:
                row.append("SI:f:0.5")   # a second one is dropped, the first decides
        else:
            row.append(tag)
        return row

    def overlap(i, j):
        return int(rng.integers(1, min(len(seqs[i]), len(seqs[j]), 24)))

    orients = ["+", "-", "+", "-", "*", "++", "p"]
    for _ in range(n_links):
        i, j = int(rng.integers(R)), int(rng.integers(R))
        links.append((i, j, orients[rng.integers(len(orients))], orients[rng.integers(len(orients))],
                      0 if rng.random() < 0.1 else overlap(i, j), int(rng.integers(6, 9))))
    i, j = int(rng.integers(R)), int(rng.integers(R - 1))
    j += j >= i
    links += [(i, j, "+", "+", overlap(i, j), 6), (j, i, "-", "-", overlap(i, j), 8), (i, j, "+", "+", overlap(i, j), 7)]   # one pair, three times
    k = int(rng.integers(R))
    links += [(k, k, "+", "-", overlap(k, k), 6), (k, k, "-", "+", overlap(k, k), 8)]                                  # a + a -
    links = [links[k] for k in rng.permutation(len(links))]
    # S lines first (with their A runs), some links in between the later S lines naming earlier segments only
    cut = int(rng.integers(R // 2, R))
    defined, pending = 0, list(links)
    for r, (name, seq) in enumerate(zip(names, seqs)):
        row = ["S", name, seq if sequences else "*", f"LN:i:{len(seq)}"] + (["rd:i:3"] if rng.random() < 0.3 else [])
        lines.append(join(row) + end())
        if rng.random() < 0.5:      # A lines: a run for utg* names (one cut by a blank line), ignored after any other name
            for a in range(int(rng.integers(1, 4))):
                if a == 1 and rng.random() < 0.4:
                    lines.append(["\n", "   \n"][rng.integers(2)])
                lines.append(join(["A", name, str(7 * a), "+-"[rng.integers(2)], f"m{r}/{a}/ccs", "0", "86", "id:i:1"][:int(rng.integers(5, 9))]) + end())
        defined = r + 1
        if r >= cut:
            rest = []
            for ln in pending:
                if ln[0] < defined and ln[1] < defined and rng.random() < 0.5:
                    lines.append(join(link(*ln)) + end())
                else:
                    rest.append(ln)
            pending = rest
        if rng.random() < 0.15:
            lines.append(["\n", " \t\n", "H\tVN:Z:1.0\n", "# S not a segment\n", "SS\tx\n", "A\tstray\t0\t+\tnobody\n"][rng.integers(6)])
    for ln in pending:
        lines.append(join(link(*ln)) + end())
    link_rows = [k for k, ln in enumerate(lines) if ln.startswith("L")]
    if tags == "none":
        lines = [re.sub(r"[\t \x0b\x0c\x1c-\x1f]+SI:f:[^\t \x0b\x0c\x1c-\x1f\r\n]*", "", ln) if ln.startswith("L") else ln for ln in lines]
    elif tags == "all_but_one":
        live = [k for k in link_rows if not re.search(r"[\t \x0b\x0c\x1c-\x1f]0M", lines[k])]
        k = live[int(rng.integers(len(live)))]
        lines[k] = re.sub(r"[\t \x0b\x0c\x1c-\x1f]+SI:f:[^\t \x0b\x0c\x1c-\x1f\r\n]*", "", lines[k])
    text = "".join(lines)
    if seed % 2:
        text = text.rstrip("\r\n \t")    # no final newline
    return text
