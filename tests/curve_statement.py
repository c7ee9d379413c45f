"""The precision-recall contract (utils/metrics.py:51-80, i.e. scikit-learn's precision_recall_curve and average_precision_score)
restated in plain numpy: the statement the device curves (gnnome_amd/metrics.py, csrc/pr_curve.hip) are checked against, itself
anchored bit for bit to the installed scikit-learn (tests/test_pr_curve_statement.py).

With `scores` float32 and `positive` bool, one per edge:
    1. sort by score, descending (the order inside a run of equal scores does not matter)
    2. idx = the last position of every run of equal scores; the last one is E-1
    3. tps[j] = positives at positions <= idx[j]; fps[j] = 1 + idx[j] - tps[j]; thresholds[j] = the score at idx[j]
    4. precision = tps / (tps + fps), recall = tps / tps[-1]: float64 divisions of exact integers
    5. scikit-learn 0.24.2 (the reference's pin) keeps j = last, last-1, ..., 0 with last the first j where tps[j] == tps[-1];
       current scikit-learn keeps every j
    6. reversed (ascending threshold), precision extended by 1.0 and recall by 0.0
    7. AP = -sum(diff(recall) * precision[:-1]), clipped below at 0: the same number with or without the cut
The inverse pair of the reference is score = 1 - p in float32 and positive = (label == 0)."""
import numpy as np


def sigmoid_f32(logits):
    """float32 sigmoid by torch's CPU kernel - the reference's own bits (utils/metrics.py:52)."""
    import torch
    return torch.sigmoid(torch.as_tensor(np.asarray(logits, dtype=np.float32))).numpy()


def class_view(probs, labels, inverse):
    """(scores float32, positive bool) of either class from float32 probabilities - utils/metrics.py:59-62."""
    probs, labels = np.asarray(probs, dtype=np.float32), np.asarray(labels)
    if inverse:
        return (np.float32(1) - probs).astype(np.float32), labels == 0
    return probs, labels == 1


def statement_counts(scores, positive):
    """steps 1-3 -> (thresholds float32[M] descending, tps int64[M], fps int64[M])."""
    scores, positive = np.asarray(scores), np.asarray(positive, dtype=bool)
    assert scores.dtype == np.float32 and scores.ndim == 1 and scores.size >= 1 and not np.isnan(scores).any()
    order = np.argsort(-scores, kind="stable")
    s, pos = scores[order], positive[order]
    idx = np.r_[np.flatnonzero(s[1:] != s[:-1]), s.size - 1].astype(np.int64)
    tps = np.cumsum(pos, dtype=np.int64)[idx]
    return s[idx], tps, 1 + idx - tps


def statement_curve(scores, positive, cut_at_full_recall=True):
    """steps 1-6 -> (precision float64[K+1], recall float64[K+1], thresholds float32[K], last)."""
    thresholds, tps, fps = statement_counts(scores, positive)
    assert tps[-1] > 0, "no edge of the positive class"
    precision = tps.astype(np.float64) / (tps + fps).astype(np.float64)
    recall = tps.astype(np.float64) / np.float64(tps[-1])
    last = int(np.searchsorted(tps, tps[-1]))
    keep = slice(last, None, -1) if cut_at_full_recall else slice(None, None, -1)
    return np.r_[precision[keep], 1.0], np.r_[recall[keep], 0.0], thresholds[keep], last


def statement_ap(scores, positive):
    """step 7 on the uncut curve."""
    precision, recall, _, _ = statement_curve(scores, positive, cut_at_full_recall=False)
    return max(0.0, float(-np.sum(np.diff(recall) * precision[:-1])))


def planted_ties(num_edges, seed, distinct=None, positive_rate=0.9):
    """random float32 logits of which about half repeat one of `distinct` planted values, and 0 / 1 labels (at least one of each
    when num_edges >= 2)."""
    rng = np.random.default_rng(seed)
    logits = rng.normal(0.0, 3.0, size=num_edges).astype(np.float32)
    pool = rng.normal(0.0, 3.0, size=distinct or max(1, num_edges // 16)).astype(np.float32)
    tie = rng.random(num_edges) < 0.5
    logits[tie] = pool[rng.integers(0, pool.size, size=int(tie.sum()))]
    labels = (rng.random(num_edges) < positive_rate).astype(np.float32)
    if num_edges >= 2:
        labels[0], labels[1] = 1.0, 0.0
    return logits, labels


def saturated(num_edges, seed):
    """logits of +-200 and +-150 (sigmoid exactly 1.0 and 0.0 in float32) among ordinary ones."""
    rng = np.random.default_rng(seed)
    logits = rng.normal(0.0, 2.0, size=num_edges).astype(np.float32)
    where = rng.random(num_edges) < 0.6
    logits[where] = rng.choice(np.array([200.0, -200.0, 150.0, -150.0], dtype=np.float32), size=int(where.sum()))
    labels = (rng.random(num_edges) < 0.5).astype(np.float32)
    labels[:2] = (1.0, 0.0)
    return logits, labels


def tiny_probabilities(num_edges, seed):
    """float32 PROBABILITIES of which most lie below 2^-25: distinct scores of the direct curve that 1 - p rounds to one score
    (1.0) of the inverse curve."""
    rng = np.random.default_rng(seed)
    probs = rng.random(num_edges).astype(np.float32)
    where = rng.random(num_edges) < 0.7
    probs[where] = (rng.random(int(where.sum())) * 2.0 ** -25).astype(np.float32)
    labels = (rng.random(num_edges) < 0.5).astype(np.float32)
    labels[:2] = (1.0, 0.0)
    assert np.unique(probs[where]).size > np.unique(np.float32(1) - probs[where]).size == 1
    return probs, labels
