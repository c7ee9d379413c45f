"""Overlaps beyond one wavefront's 65 536 query rows (graph_parser.py:101-117 has no such limit): the strip pass of
gnnome_overlap_edit_distance_long (csrc/overlap_similarity.hip, k_overlap_strips) behind `long_overlaps=True`, against the
Wagner-Fischer oracle - and, where the full matrix would cost that oracle too long, against the big-integer Myers programme of
tests/overlap_strip_statement.py, which tests/test_overlap_strip_statement.py checks against the oracle.  Bit-exact integers."""
import functools
import random

import pytest
import torch

from gnnome_amd import gfa
from oracle import overlap_oracle
from overlap_strip_statement import bigint_edit_distance

STRIP = 65_536   # rows of one strip at up to 19 symbols (32 blocks per lane); 32 768 above (16 blocks per lane)


def dev():
    return torch.device("cuda", 0)


def _random(rng, n, alphabet="ACGT"):
    return "".join(rng.choices(alphabet, k=n))


def _mutate(rng, s, rate, alphabet="ACGT"):
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            continue                                # deletion
        if r < 2 * rate / 3:
            out.append(rng.choice(alphabet))        # substitution
            continue
        if r < rate:
            out.append(rng.choice(alphabet))        # insertion
        out.append(ch)
    return "".join(out)


def _two_tone(rng, parts):
    """Consecutive random pieces over {A, C} and {G, T} in turn.  A short target is a subsequence of any long random ACGT query (its
    distance is just m - n, whatever the kernel does in between); against a query whose rows change alphabet at a strip boundary
    the order of the target's letters matters, and the best alignment has to cross that boundary at the right column."""
    return "".join(_random(rng, n, "AC" if k % 2 == 0 else "GT") for k, n in enumerate(parts))


def _rc(s):
    return overlap_oracle.read_seqs([s])[1]


@functools.lru_cache(maxsize=None)
def _long_pair():
    """Two reads of about 70 kb whose 66 000-base overlap differs in about 1 %: far outside the band, both sides above one strip.
    -> (reads, {(src, dst, ol): distance}) for the edge and its reverse-complement mate, by the big-integer reference."""
    rng = random.Random(21)
    shared = _random(rng, 66_000)
    a = _random(rng, 4_000) + shared
    b = _mutate(rng, shared, 0.01) + _random(rng, 4_000)
    seqs = overlap_oracle.read_seqs([a, b])
    want = {(u, v, 66_000): bigint_edit_distance(seqs[u][-66_000:], seqs[v][:66_000]) for u, v in ((0, 2), (3, 1))}
    return [a, b], want


@pytest.mark.gpu
def test_strip_edges_against_short_targets_and_the_carry_batch_edge():
    """Queries of exactly one strip, one row and one block more, exactly two strips and one row more (three strips), each against
    targets of 63, 64 and 65 columns (the batch in which lane 0 reads the carry) and one of 300 - 2 000 columns cut from the query
    across a strip boundary and mutated.  The query changes its two-letter alphabet at every strip boundary (_two_tone), so no distance
    is just m - n.  One strip is the class-32 kernel's case: the default entry must give the same."""
    from gnnome_amd import overlap
    rng = random.Random(31)
    big = _two_tone(rng, (STRIP, STRIP, 1))
    rows = (65_536, 65_537, 65_568, 131_072, 131_073)
    reads, src, dst, ol = [], [], [], []
    for m in rows:
        reads.append(big[:m])
        u = 2 * (len(reads) - 1)
        for n in (63, 64, 65, rng.randrange(300, 2001)):
            at = STRIP - n // 2 if m > STRIP else m - 2 * n      # a piece that straddles row 65 536 where there is one
            reads.append(_mutate(rng, big[at:at + 2 * n], 0.3)[:n])  # (30 %: letters the query's rows there do not have)
            assert len(reads[-1]) == n
            src.append(u), dst.append(2 * (len(reads) - 1)), ol.append(m)
    want_d, want_s = overlap_oracle.calculate_similarities(reads, src, dst, ol)
    assert all(w > m - n for w, m, n in zip(want_d, ol, (len(reads[v >> 1]) for v in dst)))
    st = {}
    d, s = overlap.edit_distances(reads, src, dst, ol, device=dev(), stats=st, long_overlaps=True)
    assert d.cpu().tolist() == want_d
    assert torch.allclose(s.cpu().double(), torch.tensor(want_s, dtype=torch.float64), atol=1e-7)
    assert st["strips"] == 16 and st["edges"] == 20      # the four one-strip overlaps went through the class-32 kernel
    one = [i for i, m in enumerate(ol) if m == STRIP]
    d0, _ = overlap.edit_distances(reads, [src[i] for i in one], [dst[i] for i in one], [ol[i] for i in one], device=dev())
    assert d0.cpu().tolist() == [want_d[i] for i in one]


@pytest.mark.gpu
def test_long_target_uses_the_carry_at_full_length():
    """66 000 x 66 000 at about 1 % divergence, forward and as the reverse-complement mate: the band gives up, two strips, the carry
    buffer is written and read for all 66 000 columns."""
    from gnnome_amd import overlap
    reads, want = _long_pair()
    src, dst, ol = (list(x) for x in zip(*want))
    st = {}
    d, s = overlap.edit_distances(reads, src, dst, ol, device=dev(), stats=st, long_overlaps=True)
    assert d.cpu().tolist() == list(want.values())
    assert all(300 < w < 1500 for w in want.values())
    assert st["banded"] == 0 and st["strips"] == 2
    assert torch.allclose(s.cpu().double(), torch.tensor([1 - w / 66_000 for w in want.values()], dtype=torch.float64), atol=1e-7)


@pytest.mark.gpu
def test_all_four_orientations_of_a_two_strip_overlap():
    """Odd endpoints read their read backwards through the complement table, in every strip's masks and in the target."""
    from gnnome_amd import overlap
    rng = random.Random(41)
    reads, src, dst, ol = [], [], [], []
    for su in (0, 1):
        spelled = _random(rng, 4_001) + _two_tone(rng, (STRIP, 464))        # what node `src` spells; its last 66 000 bases are the query
        reads.append(_rc(spelled) if su else spelled)
        u = 2 * (len(reads) - 1) + su
        for sv in (0, 1):
            target = _mutate(rng, spelled[-66_000:][STRIP - 700:STRIP + 700], 0.08)      # what node `dst` must spell, straddling the strip boundary
            reads.append(_rc(target) if sv else target)
            src.append(u), dst.append(2 * (len(reads) - 1) + sv), ol.append(66_000)
    assert sorted((u & 1, v & 1) for u, v in zip(src, dst)) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    want_d, _ = overlap_oracle.calculate_similarities(reads, src, dst, ol)
    assert all(w > 66_000 - len(reads[v >> 1]) for w, v in zip(want_d, dst))
    st = {}
    d, _ = overlap.edit_distances(reads, src, dst, ol, device=dev(), stats=st, long_overlaps=True)
    assert d.cpu().tolist() == want_d and st["strips"] == 4


@pytest.mark.gpu
def test_wide_alphabet_runs_in_class_16_strips():
    """30 symbols (IUPAC codes, both cases): 40 000 query rows have no class whose masks fit LDS - refused by default, exact in two
    strips of 32 768 rows with long_overlaps=True."""
    from gnnome_amd import overlap
    rng = random.Random(51)
    alphabet = "ACGTMRWSYKVHDBNacgtmrwsykvhdbn"
    a = _random(rng, 40_000, alphabet)
    b = _mutate(rng, a[32_768 - 750:32_768 + 750], 0.1, alphabet)[:1500]
    reads, src, dst, ol = [a, b, _rc(b)], [0, 0, 1], [2, 5, 3], [40_000, 40_000, 40_000]
    assert overlap.symbol_table(overlap.pack_reads(reads)[0])[1] == 30
    want_d, want_s = overlap_oracle.calculate_similarities(reads, src, dst, ol)
    with pytest.raises(ValueError):
        overlap.edit_distances(reads, src, dst, ol, device=dev())
    st = {}
    d, s = overlap.edit_distances(reads, src, dst, ol, device=dev(), stats=st, long_overlaps=True)
    assert d.cpu().tolist() == want_d and st["strips"] == 3 and st["banded"] == 0
    assert torch.allclose(s.cpu().double(), torch.tensor(want_s, dtype=torch.float64), atol=1e-7)


@pytest.mark.gpu
def test_mixed_list_short_overlaps_unchanged_and_three_long_ones():
    """About 200 ordinary overlaps with three long ones in between: the short ones' distances are those of a default call on the
    short ones alone, the long ones are exact, and the statistics count exactly three overlaps for the strip pass."""
    from gnnome_amd import overlap
    rng = random.Random(61)
    genome = _random(rng, 60_000)
    reads, pos = [], 0
    for _ in range(101):
        ln = rng.randrange(400, 900)
        reads.append(_mutate(rng, genome[pos:pos + ln], 0.02))
        pos += ln // 3
    src, dst, ol = [], [], []
    for r in range(100):
        for t in (1, 2):
            if r + t < len(reads):
                flip = rng.random() < 0.3       # most are true overlaps (the band settles them), the rest look unrelated
                src.append(2 * r + (rng.randrange(2) if flip else 0)), dst.append(2 * (r + t) + (rng.randrange(2) if flip else 0))
                ol.append(rng.randrange(200, min(len(reads[r]), len(reads[r + t]))))
    short = len(src)
    assert 190 <= short <= 200
    big = _two_tone(rng, (35_000, 35_000))          # (its reverse complement is two-tone in the same order)
    first_long = len(reads)
    reads += [big, _mutate(rng, big[35_000 - 600:35_000 + 600], 0.05), _random(rng, 1_100)]
    longs = [(2 * first_long, 2 * first_long + 2, 67_000), (2 * first_long + 1, 2 * first_long + 4, 69_999),
             (2 * first_long, 2 * first_long + 5, 70_000)]
    for k, (u, v, L) in enumerate(longs):           # interleaved: at 1/4, 1/2 and 3/4 of the list
        at = (k + 1) * len(src) // 4
        src.insert(at, u), dst.insert(at, v), ol.insert(at, L)
    is_long = [L > STRIP for L in ol]
    want_d, _ = overlap_oracle.calculate_similarities(reads, src, dst, ol)
    assert all(w > L - len(reads[v >> 1]) for w, v, L, lg in zip(want_d, dst, ol, is_long) if lg)
    st = {}
    d, _ = overlap.edit_distances(reads, src, dst, ol, device=dev(), stats=st, long_overlaps=True)
    assert d.cpu().tolist() == want_d
    assert st["strips"] == 3 and st["edges"] == short + 3
    keep = [i for i, lg in enumerate(is_long) if not lg]
    st0 = {}
    d0, _ = overlap.edit_distances(reads, [src[i] for i in keep], [dst[i] for i in keep], [ol[i] for i in keep], device=dev(), stats=st0)
    assert d0.cpu().tolist() == [want_d[i] for i in keep] and st0["banded"] == st["banded"] and "strips" not in st0


@pytest.mark.gpu
def test_default_still_refuses_what_it_refused():
    from gnnome_amd import overlap
    rng = random.Random(71)
    reads = [_random(rng, 66_000), _random(rng, 500)]
    with pytest.raises(ValueError):
        overlap.edit_distances(reads, [0], [2], [66_000], device=dev())
    with pytest.raises(ValueError):
        overlap.overlap_similarity(reads, [0], [2], [66_000], device=dev())
    d, _ = overlap.edit_distances(reads, [0], [2], [66_000], device=dev(), long_overlaps=True)
    assert d.cpu().tolist() == overlap_oracle.calculate_similarities(reads, [0], [2], [66_000])[0]


@pytest.mark.gpu
@pytest.mark.parametrize("parser", ("host", "device"))
def test_gfa_with_a_66_kb_overlap(tmp_path, parser):
    """Two reads of about 70 kb and one L line of 66 000: read_gfa(similarity="device") raises as it always did, and returns the
    oracle's similarities - the edge's and its reverse-complement mate's - with long_overlaps=True."""
    reads, want = _long_pair()
    path = tmp_path / "long.gfa"
    path.write_text("".join(f"S\tread{r}\t{s}\tLN:i:{len(s)}\n" for r, s in enumerate(reads)) + "L\tread0\t+\tread1\t+\t66000M\n")
    with pytest.raises(ValueError):
        gfa.read_gfa(str(path), similarity="device", parser=parser)
    g = gfa.read_gfa(str(path), similarity="device", parser=parser, long_overlaps=True)
    edges = list(zip(g["src"].tolist(), g["dst"].tolist(), g["overlap_length"].tolist()))
    assert sorted(edges) == sorted(want)
    sims = torch.tensor([1 - want[e] / e[2] for e in edges], dtype=torch.float64)
    assert g["overlap_similarity"].dtype == torch.float32
    assert torch.allclose(g["overlap_similarity"].double().cpu(), sims, atol=1e-7)
