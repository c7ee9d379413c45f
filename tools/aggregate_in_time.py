#!/usr/bin/env python
"""Launch time of gnnome_node_aggregate_in_f32 (the in-edge aggregation of GatedGCN) against gnnome_node_aggregate_f32 with an all-zero A3h
table - the only way to get this result before the kernel existed - on one device, in alternating order.

    python tools/aggregate_in_time.py [--out profiles/aggregate_in_time.txt] [--runs 3] [--launches 3000]

Shapes: the synthetic 1M-edge graph (100 000 nodes) at H = 128 and the 2.5M-edge shard (250 000 nodes) at H = 256.  Each run's figure
is the MEAN over `launches` back-to-back launches between two device events (warmed up first; 3000 launches are 0.4 - 3 s per window), with
`runs` alternating runs per kernel; the figure quoted per kernel is the MEDIAN OVER RUNS of those per-run means.  The outputs are compared
bit for bit before anything is timed.  The least bytes each kernel must move per launch are computed from the
shapes: one read of e[E,H] for the in-edge kernel, two for the symmetric one (its out-edge pass reads the rows again, whatever A3h holds)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnome_amd import ops  # noqa: E402
from gnnome_amd.synth import make_graph  # noqa: E402

SHAPES = (("synthetic 1M-edge graph", 100_000, 1_000_000, 128), ("2.5M-edge shard", 250_000, 2_500_000, 256))


def timed(fn, launches):
    for _ in range(10):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=3000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aggregate_in_time: no HIP device - this is a measurement, there is nothing to report without one")
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; {a.runs} alternating runs, each the mean of {a.launches} launches (ms per launch); quoted: the median over runs"]
    for name, n, e, H in SHAPES:
        g = make_graph(n, e, seed=1)
        views = ops.GraphViews(g["src"].to(dev), g["dst"].to(dev), n)
        gen = torch.Generator(device=dev).manual_seed(0)
        ee = torch.randn(e, H, device=dev, generator=gen)
        h = torch.randn(n, H, device=dev, generator=gen)
        P5 = torch.randn(n, 5 * H, device=dev, generator=gen)
        P5[:, 2 * H:3 * H] = 0.0                                  # the symmetric kernel's A3h: all zero
        P4 = torch.cat([P5[:, :2 * H], P5[:, 3 * H:]], 1).contiguous()   # the one-direction model's [N,4H] projection: the same A1h | A2h
        sc, sh = torch.rand(H, device=dev, generator=gen) * 0.1, torch.randn(H, device=dev, generator=gen)
        out_new, out_old = torch.empty_like(h), torch.empty_like(h)
        new = lambda: ops.node_aggregate_in(ee, P4[:, :H], P4[:, H:2 * H], views, h, 0, sc, sh, out=out_new)  # noqa: E731
        old = lambda: ops.node_aggregate(ee, P5[:, :H], P5[:, H:2 * H], P5[:, 2 * H:3 * H], views, h, 0, sc, sh, out=out_old)  # noqa: E731
        new(), old()
        torch.cuda.synchronize()
        same = torch.equal(out_new, out_old)
        lines.append(f"{name}: N={n} E={e} H={H}; outputs equal bit for bit: {same}; least bytes per launch: in-edge {e * H * 4 / 1e6:.0f} MB "
                     f"(e once), symmetric {2 * e * H * 4 / 1e6:.0f} MB (e twice)")
        t_new, t_old = [], []
        for run in range(a.runs):
            t_old.append(timed(old, a.launches))
            t_new.append(timed(new, a.launches))
            lines.append(f"  run {run}: node_aggregate (A3h = 0) {t_old[-1]:.4f} ms   node_aggregate_in {t_new[-1]:.4f} ms")
        mo, mn = sorted(t_old)[len(t_old) // 2], sorted(t_new)[len(t_new) // 2]
        lines.append(f"  median over runs: {mo:.4f} -> {mn:.4f} ms ({mo / mn:.2f}x); e stream alone at the in-edge kernel's time: {e * H * 4 / mn / 1e6:.0f} GB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
