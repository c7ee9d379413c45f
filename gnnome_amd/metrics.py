"""Confusion counts and the scores derived from them (utils/metrics.py:6-46), and the threshold-free figures - precision-recall
curves and average precision of either class (utils/metrics.py:51-80) - counted on the device.

`calculate_tfpn` replaces four `torch.sum(torch.logical_and(...)).item()` round trips (each a device sync) plus the
rounded-sigmoid temporaries by one pass and ONE 32-byte copy; the arithmetic on the four integers is the reference's.

The curves restate scikit-learn's precision_recall_curve / average_precision_score (csrc/pr_curve.hip): one elementwise pass packs
score and class into a sortable key, torch sorts the keys, an integer scan counts TP and FP at every distinct score.  One
synchronisation per curve returns the number of thresholds together with the checks; get_aps / get_aps_inverse bring one float to the
host.  Declined, each as a ValueError before anything is returned: a NaN prediction (scikit-learn raises there too), a label other than
0 or 1, and - a stated divergence - a graph without an edge of the positive class, where the reference gets NaN recall or a warning.
sample_weight and drop_intermediate are not offered.
"""
import ctypes

import torch

from . import _lib, ops
from .ops import _on, _ptr, _stream


def calculate_tfpn(edge_predictions, edge_labels):
    """(TP, TN, FP, FN) of round(sigmoid(edge_predictions)) against edge_labels - utils/metrics.py:6-12."""
    logits = edge_predictions.detach().float().reshape(-1).contiguous()
    labels = edge_labels.detach().float().reshape(-1).contiguous()
    _, _, _, counts = ops.edge_loss(logits, None, labels, 1.0, 0.0, need_grad=False, need_counts=True)
    tp, tn, fp, fn = counts.tolist()
    return tp, tn, fp, fn


def _scores(TP, TN, FP, FN):
    precision = TP / (TP + FP) if TP + FP else 0
    recall = TP / (TP + FN) if TP + FN else 0
    f1 = TP / (TP + 0.5 * (FP + FN)) if TP + 0.5 * (FP + FN) else 0
    accuracy = (TP + TN) / (TP + TN + FP + FN)
    return accuracy, precision, recall, f1


def calculate_metrics(TP, TN, FP, FN):
    """(accuracy, precision, recall, f1), zero where the reference catches ZeroDivisionError - utils/metrics.py:15-28."""
    return _scores(TP, TN, FP, FN)


def calculate_metrics_inverse(TP, TN, FP, FN):
    """the same with the negative class as the positive one - utils/metrics.py:31-46."""
    return _scores(TN, TP, FN, FP)


def _curve_inputs(preds, labels, probs_on_device, device):
    """float32 scores and labels on the device.  probs_on_device=False: the sigmoid is torch's CPU kernel - the reference's own bits
    (as DecodeGraph.set_scores) - and the probabilities are uploaded; True: the logits go up and the kernel applies the sigmoid."""
    preds, labels = torch.as_tensor(preds), torch.as_tensor(labels)
    if device is None:
        device = preds.device if preds.is_cuda else labels.device if labels.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    s = preds.detach().reshape(-1).float()
    y = labels.detach().reshape(-1).to(device, torch.float32).contiguous()
    if s.numel() != y.numel():
        raise ValueError(f"precision_recall: {s.numel()} predictions for {y.numel()} labels")
    if not 1 <= s.numel() < (1 << 31):
        raise ValueError(f"precision_recall: E={s.numel()} outside [1, 2^31)")
    s = s.to(device) if probs_on_device else torch.sigmoid(s.cpu()).to(device)
    return s.contiguous(), y, device


class _Curve:
    """The scan of one (scores, labels, class): what every public function below starts from.  After __init__ the keys are sorted, the
    tile sums are scanned and M (thresholds) and P (positives) are on the host; emit() fills the outputs it is asked for."""

    def __init__(self, preds, labels, inverse, probs_on_device, device=None, keep_probs=False):
        s, y, dev = _curve_inputs(preds, labels, probs_on_device, device)
        lib = _lib.load()
        self.lib, self.dev, self.E = lib, dev, s.numel()
        need = ctypes.c_size_t(0)
        _lib.check(lib.gnnome_pr_curve_workspace_bytes(self.E, ctypes.byref(need)), "pr_curve_workspace_bytes")
        self.ws = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
        keys = torch.empty(self.E, dtype=torch.int32, device=dev)          # the uint32 keys are below 2^31: int32 order is theirs
        self.probs = torch.empty_like(s) if keep_probs else None
        res = (ctypes.c_int64 * 4)()
        with _on(dev):
            _lib.check(lib.gnnome_pr_curve_keys(_ptr(s), _ptr(y), self.E, int(bool(probs_on_device)), int(bool(inverse)), _ptr(keys),
                                                _ptr(self.probs), _ptr(self.ws), self.ws.numel(), _stream(dev)), "pr_curve_keys")
            self.keys = torch.sort(keys, descending=True).values
            _lib.check(lib.gnnome_pr_curve_scan(_ptr(self.keys), self.E, _ptr(self.ws), self.ws.numel(), res, _stream(dev)), "pr_curve_scan")
        self.M, self.P, bad_pred, bad_label = (int(v) for v in res)
        positive = 0 if inverse else 1
        if bad_pred >= 0:
            raise ValueError(f"precision_recall: the prediction of edge {bad_pred} is NaN or not a probability in [0, 1]")
        if bad_label >= 0:
            raise ValueError(f"precision_recall: the label of edge {bad_label} is neither 0 nor 1")
        if self.P == 0:
            raise ValueError(f"precision_recall: none of the {self.E} edges has label {positive}, the positive class: recall is undefined")

    def emit(self, counts=False, curve=False):
        dev, M = self.dev, self.M
        new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)   # noqa: E731
        thresholds = new(M, torch.float32) if counts else None
        tp, fp = (new(M, torch.int64), new(M, torch.int64)) if counts else (None, None)
        precision, recall = (new(M + 1, torch.float64), new(M + 1, torch.float64)) if curve else (None, None)
        last = new(1, torch.int64) if curve else None
        with _on(dev):
            _lib.check(self.lib.gnnome_pr_curve_emit(_ptr(self.keys), self.E, M, self.P, _ptr(thresholds), _ptr(tp), _ptr(fp), _ptr(precision),
                                                     _ptr(recall), _ptr(last), _ptr(self.ws), self.ws.numel(), _stream(dev)), "pr_curve_emit")
        return thresholds, tp, fp, precision, recall, last

    def average_precision(self):
        _, _, _, precision, recall, _ = self.emit(curve=True)
        ap = torch.empty(1, dtype=torch.float64, device=self.dev)
        with _on(self.dev):
            _lib.check(self.lib.gnnome_pr_curve_ap(_ptr(precision), _ptr(recall), self.M, _ptr(ap), _ptr(self.ws), self.ws.numel(),
                                                   _stream(self.dev)), "pr_curve_ap")
        return ap


def pr_curve_tile_size():
    """Sorted positions per tile of the scan (csrc/pr_curve.hip); results do not depend on it, the tests place their edges by it."""
    tile = ctypes.c_int(0)
    _lib.check(_lib.load().gnnome_pr_curve_tile_size(ctypes.byref(tile)), "pr_curve_tile_size")
    return int(tile.value)


def precision_recall_counts(preds, labels, inverse=False, probs_on_device=False, device=None):
    """-> (thresholds float32[M], tp int64[M], fp int64[M], number of positives), tensors on the device: the distinct scores in
    DESCENDING order and, for each, the positives and negatives scored at or above it (scikit-learn's _binary_clf_curve).  Score and
    positive class: sigmoid(preds) and label 1, or with inverse=True 1 - sigmoid(preds) (float32) and label 0.  The primitive under
    the curves: e.g. the max-F1 threshold is thresholds[argmax(2 tp / (tp + fp + P))], without leaving the device."""
    c = _Curve(preds, labels, inverse, probs_on_device, device)
    thresholds, tp, fp, _, _, _ = c.emit(counts=True)
    return thresholds, tp, fp, c.P


def _curve(preds, labels, inverse, cut_at_full_recall, probs_on_device, device):
    c = _Curve(preds, labels, inverse, probs_on_device, device)
    thresholds, _, _, precision, recall, last = c.emit(counts=True, curve=True)
    thresholds = thresholds.flip(0)
    if cut_at_full_recall:   # scikit-learn 0.24.2 keeps j = last..0, which are the final last + 1 thresholds of the ascending order
        first = c.M - 1 - int(last)
        thresholds, precision, recall = thresholds[first:], precision[first:], recall[first:]
    return precision.cpu().numpy(), recall.cpu().numpy(), thresholds.cpu().numpy()


def get_precision_recall_curve(preds, labels, cut_at_full_recall=True, probs_on_device=False, device=None):
    """(precision float64[K+1], recall float64[K+1], thresholds float32[K]) as numpy arrays, thresholds ascending, the last point
    (1, 0) - utils/metrics.py:51-55.  cut_at_full_recall=True is the scikit-learn the reference pins (0.24.2: thresholds below the
    one that first reaches full recall are dropped); False is current scikit-learn, which keeps every distinct score."""
    return _curve(preds, labels, False, cut_at_full_recall, probs_on_device, device)


def get_precision_recall_curve_inverse(preds, labels, cut_at_full_recall=True, probs_on_device=False, device=None):
    """the same for score 1 - sigmoid(preds) and positive class 0 - utils/metrics.py:58-63."""
    return _curve(preds, labels, True, cut_at_full_recall, probs_on_device, device)


def get_aps(preds, labels, probs_on_device=False, device=None):
    """average_precision_score(labels, sigmoid(preds)) - utils/metrics.py:67-71; one float crosses to the host."""
    return float(_Curve(preds, labels, False, probs_on_device, device).average_precision())


def get_aps_inverse(preds, labels, probs_on_device=False, device=None):
    """average_precision_score(labels, 1 - sigmoid(preds), pos_label=0) - utils/metrics.py:75-80."""
    return float(_Curve(preds, labels, True, probs_on_device, device).average_precision())
