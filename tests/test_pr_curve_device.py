"""The device curves (gnnome_amd/metrics.py, csrc/pr_curve.hip) against tests/curve_statement.py fed with the same float32
probabilities: thresholds, tp, fp, precision and recall bit for bit (integer counts and correctly rounded float64 divisions), the AP
within E * 2^-52 (both sides add the same terms, whose absolute values sum to at most 1; each order of summation errs by at most
E * 2^-53).  With probs_on_device=True the probabilities are the ones the kernel computed, fetched back."""
import functools

import numpy as np
import pytest
import torch

import curve_statement as cs
from gnnome_amd import metrics, pipeline
from gnnome_amd.synth import make_graph

pytestmark = pytest.mark.gpu


def _with_run(num_edges, first, last_pos, seed):
    """distinct scores except one run of equal ones at sorted positions [first, last_pos], in shuffled edge order."""
    rng = np.random.default_rng(seed)
    logits = (5.0 - 0.003 * np.arange(num_edges)).astype(np.float32)
    logits[first:last_pos + 1] = logits[first]
    labels = (rng.random(num_edges) < 0.6).astype(np.float32)
    labels[:2] = (1.0, 0.0)
    perm = rng.permutation(num_edges)
    return logits[perm], labels[perm]


def _placed_positives(num_edges, where, seed):
    """distinct scores, label 1 exactly at the sorted positions `where` (descending score), in shuffled edge order."""
    rng = np.random.default_rng(seed)
    logits = (4.0 - 0.004 * np.arange(num_edges)).astype(np.float32)
    labels = np.zeros(num_edges, dtype=np.float32)
    labels[where] = 1.0
    perm = rng.permutation(num_edges)
    return logits[perm], labels[perm]


def _logit(probs):
    with np.errstate(divide="ignore"):
        return np.log(probs.astype(np.float64) / (1.0 - probs.astype(np.float64))).astype(np.float32)


CASES = ("e1", "e2_equal", "e2_distinct", "all_equal", "all_distinct", "tile_minus_1", "tile", "tile_plus_1", "run_across_border",
         "run_over_three_tiles", "tile_squared_plus_3", "positives_lowest", "positives_top", "single_positive", "saturated",
         "inverse_merge")


@functools.lru_cache(maxsize=None)
def _case(name):
    T = metrics.pr_curve_tile_size()
    rng = np.random.default_rng(11)
    f32 = lambda *v: np.array(v, dtype=np.float32)   # noqa: E731
    if name == "e1":
        return f32(0.3), f32(1.0)
    if name == "e2_equal":
        return f32(1.5, 1.5), f32(1.0, 0.0)
    if name == "e2_distinct":
        return f32(-0.5, 2.0), f32(0.0, 1.0)
    if name == "all_equal":
        labels = (rng.random(T + 7) < 0.5).astype(np.float32)
        labels[:2] = (1.0, 0.0)
        return np.full(T + 7, 0.75, dtype=np.float32), labels
    if name == "all_distinct":
        E = 2 * T + 5
        labels = (rng.random(E) < 0.5).astype(np.float32)
        labels[:2] = (1.0, 0.0)
        return np.linspace(-8.0, 8.0, E, dtype=np.float32)[rng.permutation(E)], labels
    if name in ("tile_minus_1", "tile", "tile_plus_1"):
        return cs.planted_ties(T + {"tile_minus_1": -1, "tile": 0, "tile_plus_1": 1}[name], 12)
    if name == "run_across_border":
        return _with_run(2 * T + 9, T - 3, T + 4, 13)
    if name == "run_over_three_tiles":
        return _with_run(3 * T + 9, T - 2, 2 * T + 2, 14)
    if name == "tile_squared_plus_3":      # more tile sums than one tile of the scan over them holds
        return cs.planted_ties(min(T * T + 3, 2_000_003), 15)
    if name == "positives_lowest":
        return _placed_positives(T + 50, np.arange(T + 30, T + 50), 16)
    if name == "positives_top":            # twenty positives sharing the highest score
        logits, labels = _placed_positives(T + 50, np.arange(20), 17)
        logits[labels == 1.0] = 4.5
        return logits, labels
    if name == "single_positive":
        return _placed_positives(T + 3, np.array([T // 2]), 18)
    if name == "saturated":
        return cs.saturated(2 * T + 1, 19)
    if name == "inverse_merge":
        probs, labels = cs.tiny_probabilities(2 * T + 11, 20)
        return _logit(probs), labels
    raise KeyError(name)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("probs_on_device", [False, True], ids=["cpu_sigmoid", "device_sigmoid"])
@pytest.mark.parametrize("inverse", [False, True], ids=["direct", "inverse"])
@pytest.mark.parametrize("name", CASES)
def test_curve_counts_and_ap_are_the_statement(name, inverse, probs_on_device):
    logits, labels = _case(name)
    E = logits.size
    if E == 1 and inverse:
        labels = 1.0 - labels
    dev = torch.device("cuda", 0)
    if probs_on_device:
        probs = metrics._Curve(logits, labels, inverse, True, dev, keep_probs=True).probs.cpu().numpy()
        cpu = cs.sigmoid_f32(logits)
        assert np.abs(probs.astype(np.float64) - cpu) .max() <= 2.0 ** -22      # a sigmoid, whatever its last bits
    else:
        probs = cs.sigmoid_f32(logits)
    scores, positive = cs.class_view(probs, labels, inverse)
    want_thr, want_tp, want_fp = cs.statement_counts(scores, positive)

    thr, tp, fp, P = metrics.precision_recall_counts(logits, labels, inverse=inverse, probs_on_device=probs_on_device, device=dev)
    assert thr.is_cuda and tp.is_cuda and fp.is_cuda and P == int(positive.sum())
    assert _same_bits(thr.cpu().numpy(), want_thr) and _same_bits(tp.cpu().numpy(), want_tp) and _same_bits(fp.cpu().numpy(), want_fp)

    curve = metrics.get_precision_recall_curve_inverse if inverse else metrics.get_precision_recall_curve
    lengths = {}
    for cut in (True, False):
        wp, wr, wt, _ = cs.statement_curve(scores, positive, cut_at_full_recall=cut)
        p, r, t = curve(logits, labels, cut_at_full_recall=cut, probs_on_device=probs_on_device, device=dev)
        assert _same_bits(p, wp) and _same_bits(r, wr) and _same_bits(t, wt), (name, cut)
        lengths[cut] = t.size
    if not inverse:
        M = want_thr.size
        if name in ("all_equal", "e1", "e2_equal"):
            assert M == 1
        if name in ("all_distinct", "e2_distinct", "positives_lowest"):
            assert M == E
        if name == "positives_lowest":
            assert lengths[True] == lengths[False] == E        # the cut keeps everything
        if name == "positives_top":
            assert lengths[True] == 1 and lengths[False] == E - 19
        if name == "tile_squared_plus_3":
            T = metrics.pr_curve_tile_size()
            assert -(-E // T) > T or E == 2_000_003
    elif name == "inverse_merge":
        assert want_thr.size < cs.statement_counts(*cs.class_view(probs, labels, False))[0].size / 2

    aps = metrics.get_aps_inverse if inverse else metrics.get_aps
    got, want = aps(logits, labels, probs_on_device=probs_on_device, device=dev), cs.statement_ap(scores, positive)
    print(f"{name} inverse={inverse} device_sigmoid={probs_on_device}: E={E} M={want_thr.size} AP={got!r} |d|={abs(got - want):.3e} "
          f"bound={E * 2.0 ** -52:.3e}")
    assert isinstance(got, float) and abs(got - want) <= E * 2.0 ** -52


def _every_function(logits, labels, probs_on_device):
    dev = torch.device("cuda", 0)
    yield lambda: metrics.precision_recall_counts(logits, labels, probs_on_device=probs_on_device, device=dev)
    yield lambda: metrics.precision_recall_counts(logits, labels, inverse=True, probs_on_device=probs_on_device, device=dev)
    yield lambda: metrics.get_precision_recall_curve(logits, labels, probs_on_device=probs_on_device, device=dev)
    yield lambda: metrics.get_precision_recall_curve_inverse(logits, labels, probs_on_device=probs_on_device, device=dev)
    yield lambda: metrics.get_aps(logits, labels, probs_on_device=probs_on_device, device=dev)
    yield lambda: metrics.get_aps_inverse(logits, labels, probs_on_device=probs_on_device, device=dev)


@pytest.mark.parametrize("probs_on_device", [False, True], ids=["cpu_sigmoid", "device_sigmoid"])
def test_declined_inputs_name_the_first_edge(probs_on_device):
    T = metrics.pr_curve_tile_size()
    E = 3 * T - 5
    logits, labels = cs.planted_ties(E, 21)
    bad = logits.copy()
    bad[[2 * T + 17, T + 3]] = np.nan
    for call in _every_function(bad, labels, probs_on_device):
        with pytest.raises(ValueError, match=rf"prediction of edge {T + 3} "):
            call()
    bad = labels.copy()
    bad[T + 9], bad[2 * T + 1] = 2.0, 0.5
    for call in _every_function(logits, bad, probs_on_device):
        with pytest.raises(ValueError, match=rf"label of edge {T + 9} "):
            call()
    bad[T + 9], bad[2 * T + 1] = np.nan, 1.0
    with pytest.raises(ValueError, match=rf"label of edge {T + 9} "):
        metrics.get_aps(logits, bad, probs_on_device=probs_on_device)
    # no edge of the positive class: no edge to name, the message names the class
    calls = list(_every_function(logits, np.zeros(E, dtype=np.float32), probs_on_device))
    for k, call in enumerate(calls):
        if k % 2 == 0:
            with pytest.raises(ValueError, match=rf"none of the {E} edges has label 1"):
                call()
        else:
            call()
    calls = list(_every_function(logits, np.ones(E, dtype=np.float32), probs_on_device))
    for k, call in enumerate(calls):
        if k % 2 == 1:
            with pytest.raises(ValueError, match=rf"none of the {E} edges has label 0"):
                call()
    with pytest.raises(ValueError, match="predictions for"):
        metrics.get_aps(logits[:-1], labels)
    with pytest.raises(ValueError, match="outside"):
        metrics.get_aps(logits[:0], labels[:0])


def test_edge_report_on_a_synthetic_graph():
    g = make_graph(2000, 20000, seed=3)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(22)
    y = g["y"].numpy() if torch.is_tensor(g["y"]) else np.asarray(g["y"])
    scores = torch.from_numpy((rng.normal(0.0, 2.0, size=y.size) + 2.0 * (y - 0.5)).astype(np.float32))
    report = pipeline.edge_report(g, scores=scores, device=dev)
    TP, TN, FP, FN = metrics.calculate_tfpn(scores.to(dev), torch.as_tensor(g["y"]).to(dev))
    assert (report["TP"], report["TN"], report["FP"], report["FN"]) == (TP, TN, FP, FN) and TP + TN + FP + FN == y.size
    assert (report["acc"], report["precision"], report["recall"], report["f1"]) == metrics.calculate_metrics(TP, TN, FP, FN)
    assert (report["acc_inv"], report["precision_inv"], report["recall_inv"], report["f1_inv"]) == metrics.calculate_metrics_inverse(TP, TN, FP, FN)
    probs = cs.sigmoid_f32(scores.numpy())
    assert abs(report["aps"] - cs.statement_ap(*cs.class_view(probs, y, False))) <= y.size * 2.0 ** -52
    assert abs(report["aps_inverse"] - cs.statement_ap(*cs.class_view(probs, y, True))) <= y.size * 2.0 ** -52
    assert set(report) == {"TP", "TN", "FP", "FN", "acc", "precision", "recall", "f1", "acc_inv", "precision_inv", "recall_inv", "f1_inv",
                           "aps", "aps_inverse"}
    with pytest.raises(ValueError, match="neither a model nor scores"):
        pipeline.edge_report(g, device=dev)
    with pytest.raises(ValueError, match="no labels"):
        pipeline.edge_report({k: v for k, v in g.items() if k != "y"}, scores=scores, device=dev)
