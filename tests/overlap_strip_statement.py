"""The strip rule of csrc/overlap_similarity.hip (k_overlap_strips) restated in plain Python - a helper, not a test module.

A query of m rows is cut into horizontal strips of `strip_rows` rows (a multiple of 32; B * 2048 in the kernel).  Every strip runs
Myers' block recurrence (32 rows per block) over all n target columns:
  * the first block of a column takes hin = +1 in strip 0 (row 0 of the NW matrix grows by one per column) and, in strip s > 0, the
    horizontal delta that the LAST row of strip s - 1 produced for that column (the carry, one value per column);
  * every strip but the last is full - all its rows belong to the query - and records its last block's hout per column as the carry;
  * D at the bottom of a strip in column 0 is the row number, so the score starts at strip_base + 32 * blocks and adds the last
    block's hout per column; only the LAST strip has padding rows, whose vertical deltas are taken off at the end.
The kernel runs the same recurrence on a skewed wavefront (lane L at column t - L): that is a schedule, not part of the rule.

bigint_edit_distance is Myers' programme on one unbounded Python integer per vector: the reference for overlaps whose full matrix
costs the Wagner-Fischer oracle too long; tests check it against that oracle on small strings first."""

M32 = 0xFFFFFFFF


def myers_block(Pv, Mv, Eq, hin):
    hneg = 1 if hin < 0 else 0
    Xv = Eq | Mv
    Eq |= hneg
    Xh = ((((Eq & Pv) + Pv) & M32) ^ Pv) | Eq
    Ph = (Mv | (~(Xh | Pv) & M32)) & M32
    Mh = Pv & Xh
    hout = (Ph >> 31) - (Mh >> 31)
    Ph = ((Ph << 1) & M32) | (1 if hin > 0 else 0)
    Mh = ((Mh << 1) & M32) | hneg
    Pv = (Mh | (~(Xv | Ph) & M32)) & M32
    Mv = Ph & Xv
    return Pv, Mv, hout


def strip_edit_distance(q, t, strip_rows):
    """Levenshtein distance of q and t (both non-empty) by strips of `strip_rows` query rows."""
    m, n = len(q), len(t)
    assert m > 0 and n > 0 and strip_rows > 0 and strip_rows % 32 == 0
    strips = (m + strip_rows - 1) // strip_rows
    carry = None                                  # hout of the previous strip's last row, per column
    for s in range(strips):
        base = s * strip_rows
        ms = min(strip_rows, m - base)            # rows of this strip: strip_rows in every strip but the last
        last = s == strips - 1
        assert last or ms == strip_rows
        blocks = (ms + 31) // 32
        peq = {}                                  # match masks of this strip's rows only
        for r in range(ms):
            masks = peq.setdefault(q[base + r], [0] * blocks)
            masks[r // 32] |= 1 << (r % 32)
        zero = [0] * blocks
        Pv, Mv = [M32] * blocks, [0] * blocks
        score = base + 32 * blocks                # D[bottom row of the strip, padding included][column 0]
        out = [0] * n
        for c in range(n):
            h = 1 if s == 0 else carry[c]
            eq = peq.get(t[c], zero)
            for b in range(blocks):
                Pv[b], Mv[b], h = myers_block(Pv[b], Mv[b], eq[b], h)
            score += h
            out[c] = h
        if not last:
            carry = out                           # a full strip: its last block's last row is a query row
            continue
        used = ms - 32 * (blocks - 1)             # rows of the last block that belong to the query (1..32)
        mask = (M32 << used) & M32
        return score - (bin(Pv[-1] & mask).count("1") - bin(Mv[-1] & mask).count("1"))


def bigint_edit_distance(q, t):
    """Levenshtein distance by Myers' bit-vector programme on Python integers of len(q) bits (global alignment: hin = +1)."""
    m = len(q)
    if m == 0 or len(t) == 0:
        return max(m, len(t))
    full = (1 << m) - 1
    top = 1 << (m - 1)
    codes = sorted(set(q))
    raw = q.encode("latin-1") if isinstance(q, str) else bytes(q)
    peq = {}
    for ch in codes:   # bit r of peq[ch] = (q[r] == ch): one bytes.translate pass over q per symbol
        byte = ord(ch) if isinstance(ch, str) else ch
        table = bytes(49 if x == byte else 48 for x in range(256))        # '1' / '0'
        peq[ch] = int(raw.translate(table)[::-1].decode("ascii"), 2)
    Pv, Mv, score = full, 0, m
    for ch in t:
        Eq = peq.get(ch, 0)
        Xv = Eq | Mv
        Xh = ((((Eq & Pv) + Pv) & full) ^ Pv) | Eq
        Ph = Mv | (~(Xh | Pv) & full)
        Mh = Pv & Xh
        if Ph & top:
            score += 1
        elif Mh & top:
            score -= 1
        Ph = ((Ph << 1) & full) | 1
        Mh = (Mh << 1) & full
        Pv = Mh | (~(Xv | Ph) & full)
        Mv = Ph & Xv
    return score
