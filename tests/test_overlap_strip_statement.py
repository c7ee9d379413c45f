"""The strip rule of the long-overlap pass (csrc/overlap_similarity.hip, k_overlap_strips), restated in Python in
tests/overlap_strip_statement.py, against the Wagner-Fischer oracle on the CPU: strips of 32, 64 and 96 rows, queries on either
side of every strip and block boundary, targets on either side of the 64-column batch the kernel reads its carry in.  This pins
the composition - the carry of the last row's horizontal deltas, the score's start per strip, the padding correction in the last
strip only - before any kernel runs.  (The kernel itself is checked against the oracle on the GPU in tests/test_overlap_long.py.)"""
import random

import pytest

from oracle import overlap_oracle
from overlap_strip_statement import bigint_edit_distance, strip_edit_distance

QUERIES = (1, 31, 32, 33, 64, 65, 191, 192, 193)
TARGETS = (1, 2, 63, 64, 65, 200)


def _near(rng, base, n, rate=0.03):
    """base cut to n symbols with a few substitutions: the alignment stays near the diagonal and crosses every strip boundary."""
    return "".join(rng.choice("ACGT") if rng.random() < rate else ch for ch in base[:n])


@pytest.mark.parametrize("strip_rows", (32, 64, 96))
def test_strip_rule_equals_the_oracle(strip_rows):
    rng = random.Random(strip_rows)
    for m in QUERIES:
        for n in TARGETS:
            base = "".join(rng.choice("ACGT") for _ in range(max(m, n)))
            pairs = [("".join(rng.choice("ACGT") for _ in range(m)), "".join(rng.choice("ACGT") for _ in range(n))),   # random
                     (base[:m], _near(rng, base, n)),                                                                   # near-identical
                     (base[:m], base[:n])]                                                                              # identical prefix
            for q, t in pairs:
                assert strip_edit_distance(q, t, strip_rows) == overlap_oracle.edit_distance(q, t), (strip_rows, m, n, q, t)


def test_one_strip_is_the_unstripped_recurrence():
    """A strip at least as tall as the query is the existing kernel's single pass: same integers as with many strips."""
    rng = random.Random(7)
    for m, n in ((193, 200), (65, 63), (500, 333)):
        q = "".join(rng.choice("ACGTN") for _ in range(m))
        t = _near(rng, q, n, 0.1)
        want = overlap_oracle.edit_distance(q, t)
        assert {strip_edit_distance(q, t, h) for h in (32, 64, 96, 512)} == {want}


def test_bigint_myers_equals_the_oracle():
    """The reference the GPU tests use where the full matrix costs the Wagner-Fischer oracle too long."""
    rng = random.Random(9)
    alphabet = "ACGTMRWSYKVHDBNacgtmrwsykvhdbn"
    for _ in range(40):
        m, n = rng.randrange(1, 400), rng.randrange(1, 400)
        q = "".join(rng.choice(alphabet) for _ in range(m))
        t = _near(rng, q + q, n, 0.2) if rng.random() < 0.5 else "".join(rng.choice(alphabet) for _ in range(n))
        assert bigint_edit_distance(q, t) == overlap_oracle.edit_distance(q, t)
    assert bigint_edit_distance("", "ACG") == 3 and bigint_edit_distance("ACGT", "") == 4
    q = "".join(rng.choice("ACGT") for _ in range(5000))
    t = _near(rng, q[40:], 4900, 0.02)
    assert bigint_edit_distance(q, t) == overlap_oracle.edit_distance(q, t)
