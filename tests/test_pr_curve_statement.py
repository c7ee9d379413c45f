"""tests/curve_statement.py against the installed scikit-learn, bit for bit, for both classes: the uncut curve against
precision_recall_curve(..., drop_intermediate=False), the AP against average_precision_score, and the cut curve (scikit-learn 0.24.2,
the reference's pin) as the tail of the uncut one from `last`."""
import numpy as np
import pytest

import curve_statement as cs

skm = pytest.importorskip("sklearn.metrics")


def _inputs():
    out = {}
    for name, (logits, labels) in {"ties_small": cs.planted_ties(257, 1), "ties": cs.planted_ties(5000, 2), "ties_few_negatives": cs.planted_ties(3000, 3, positive_rate=0.97),
                                   "distinct": cs.planted_ties(2000, 4, distinct=1), "saturated": cs.saturated(1500, 5)}.items():
        out[name] = (cs.sigmoid_f32(logits), labels)
    out["tiny_probabilities"] = cs.tiny_probabilities(2000, 6)
    return out


INPUTS = _inputs()


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("inverse", [False, True], ids=["direct", "inverse"])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_statement_is_scikit_learn(name, inverse):
    probs, labels = INPUTS[name]
    scores, positive = cs.class_view(probs, labels, inverse)
    # the reference's own calls: utils/metrics.py:54 and :60-62
    precision, recall, thresholds = skm.precision_recall_curve(labels, 1 - probs if inverse else probs, pos_label=0 if inverse else 1,
                                                               drop_intermediate=False)
    p, r, t, last = cs.statement_curve(scores, positive, cut_at_full_recall=False)
    assert thresholds.dtype == np.float32
    assert _same_bits(t, thresholds) and _same_bits(p, precision) and _same_bits(r, recall)
    ap = skm.average_precision_score(labels, 1 - probs if inverse else probs, pos_label=0 if inverse else 1)
    assert cs.statement_ap(scores, positive) == float(ap)
    # the cut of scikit-learn 0.24.2: the uncut curve without its first len(idx) - 1 - last entries
    pc, rc, tc, last_c = cs.statement_curve(scores, positive, cut_at_full_recall=True)
    drop = t.size - 1 - last
    assert last_c == last and _same_bits(pc, p[drop:]) and _same_bits(rc, r[drop:]) and _same_bits(tc, t[drop:])
    assert rc[0] == 1.0 and (drop == 0 or r[drop - 1] == 1.0) and (rc[1:] < 1.0).all()
    ap_cut = max(0.0, float(-np.sum(np.diff(rc) * pc[:-1])))
    # the dropped terms are zeros, but numpy's pairwise sum groups a shorter array differently: each order errs by at most n * 2^-53
    assert abs(ap_cut - cs.statement_ap(scores, positive)) <= t.size * 2.0 ** -52


def test_inputs_reach_the_cases_they_are_for():
    probs, labels = INPUTS["saturated"]
    assert (probs == 1.0).any() and (probs == 0.0).any()
    probs, labels = INPUTS["tiny_probabilities"]
    direct = cs.statement_counts(*cs.class_view(probs, labels, False))[0].size
    inverse = cs.statement_counts(*cs.class_view(probs, labels, True))[0].size
    assert inverse < direct / 2
    probs, labels = INPUTS["ties"]
    assert cs.statement_counts(*cs.class_view(probs, labels, False))[0].size < probs.size * 0.7


def test_scikit_learn_raises_on_nan():
    with pytest.raises(ValueError):
        skm.precision_recall_curve(np.array([1.0, 0.0]), np.array([np.nan, 0.5], dtype=np.float32))
