"""Precision-recall curves and average precision: the reference formulation on the host (utils/metrics.py:51-80: the logits are
copied to the host, torch's CPU sigmoid, then scikit-learn where it is importable, else the numpy statement of tests/curve_statement.py -
the header row says which) against the device path (gnnome_amd/metrics.py, csrc/pr_curve.hip) on the same box, three runs each, wall
time with the device drained.  The parent commit has no device path, so the host rows are the baseline.

    python tools/pr_curve_time.py [--out profiles/pr_curve_time.txt] [--sizes 1000000,10000000]

The logits and labels start on the device (where the scorer leaves them).  Labels: 3 % negatives, as on assembly graphs; logits: normal
around +-2 by class, rounded to 1/64 for one edge in four so that the curve has ties."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gnnome_amd import metrics  # noqa: E402
import curve_statement as cs  # noqa: E402

try:
    from sklearn.metrics import average_precision_score, precision_recall_curve
    HOST = "scikit-learn " + __import__("sklearn").__version__
except ImportError:
    HOST = "numpy statement (tests/curve_statement.py); scikit-learn is not importable"
    average_precision_score = precision_recall_curve = None

RUNS = 3


def host_curve(logits, labels, inverse):
    """utils/metrics.py:51-63 (current scikit-learn: no cut)"""
    p = torch.sigmoid(logits.cpu()).detach().numpy()
    y = labels.cpu().numpy()
    if inverse:
        p = 1 - p
    if precision_recall_curve is not None:
        return precision_recall_curve(y, p, pos_label=0 if inverse else 1)
    return cs.statement_curve(p, y == (0 if inverse else 1), cut_at_full_recall=False)[:3]


def host_ap(logits, labels, inverse):
    """utils/metrics.py:67-80"""
    p = torch.sigmoid(logits.cpu()).detach().numpy()
    y = labels.cpu().numpy()
    if inverse:
        p = 1 - p
    if average_precision_score is not None:
        return float(average_precision_score(y, p, pos_label=0 if inverse else 1))
    return cs.statement_ap(p, y == (0 if inverse else 1))


def timed(fn):
    out = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(round(time.perf_counter() - t0, 4))
    return out, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pr_curve_time.txt"))
    ap.add_argument("--sizes", default="1000000,10000000")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dev = torch.device("cuda", 0)
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)

    emit(device=torch.cuda.get_device_name(0), runs=RUNS, host=HOST,
         note="seconds, wall, device drained before and after each run; logits and labels start on the device; host = device-to-host copy + "
              "CPU sigmoid + the host formulation; device_default = CPU sigmoid, probabilities uploaded; device_sigmoid = probs_on_device=True")
    metrics.get_aps(torch.zeros(4, device=dev), torch.tensor([1.0, 0.0, 1.0, 0.0], device=dev))   # load the library, warm the allocator
    for E in (int(s) for s in args.sizes.split(",")):
        rng = np.random.default_rng(5)
        y = (rng.random(E) >= 0.03).astype(np.float32)
        x = (rng.normal(0.0, 1.5, size=E) + 4.0 * (y - 0.5)).astype(np.float32)
        tie = rng.random(E) < 0.25
        x[tie] = np.round(x[tie] * 64.0) / 64.0
        logits, labels = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        for name, inverse, host, device in (
                ("get_precision_recall_curve", False, host_curve, metrics.get_precision_recall_curve),
                ("get_precision_recall_curve_inverse", True, host_curve, metrics.get_precision_recall_curve_inverse),
                ("get_aps", False, host_ap, metrics.get_aps),
                ("get_aps_inverse", True, host_ap, metrics.get_aps_inverse)):
            curve = host is host_curve
            kw = {"cut_at_full_recall": False} if curve else {}
            host_s, want = timed(lambda: host(logits, labels, inverse))
            default_s, got = timed(lambda: device(logits, labels, **kw))
            sigmoid_s, got_dev = timed(lambda: device(logits, labels, probs_on_device=True, **kw))
            if curve:
                same = all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(want, got))
                emit(E=E, what=name, host_s=host_s, device_default_s=default_s, device_sigmoid_s=sigmoid_s, thresholds=int(got[2].size),
                     thresholds_device_sigmoid=int(got_dev[2].size), default_equals_host_bit_for_bit=bool(same))
            else:
                emit(E=E, what=name, host_s=host_s, device_default_s=default_s, device_sigmoid_s=sigmoid_s, host=want, device_default=got,
                     device_sigmoid=got_dev, default_minus_host=got - want, bound=E * 2.0 ** -52)


if __name__ == "__main__":
    main()
