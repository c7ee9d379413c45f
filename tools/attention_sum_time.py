#!/usr/bin/env python
"""Launch time of gnnome_node_attention_sum_f32 (the edge softmax and weighted sum of GATModel, 3 heads) against the only other way to get
the result on the device - torch's index_select + scatter_reduce(amax) + exp + two index_add_ over the same lists of g' - on one device, in
alternating order.

    python tools/attention_sum_time.py [--out profiles/attention_sum_time.txt] [--runs 3] [--launches 500] [--torch-launches 10]

Shapes: the synthetic 1M-edge graph (100 000 nodes) at H = 128 and the 2.5M-edge shard (250 000 nodes) at H = 256, each in the directed form
(in-lists + loops, E' = E) and with both lists (directed=False, E' = 2 E), scores of scale 2, with a bias.  Each run's figure is the MEAN
over back-to-back launches between two device events (warmed up first), with `runs` alternating runs per method; the figure quoted per method
is the MEDIAN OVER RUNS.  The two results are compared before anything is timed (they differ by reordered fp32 sums and the two exp's last
bits).  The gather's traffic is computed from the shapes: (E' + N) 3H 4 bytes of rows and 2 (E' + N) 16 bytes of score rows read, N 3H 4 written.

Every shape is measured by a child process of its own under a time limit (--step-timeout seconds); the parent opens no device and stops at
the first child that fails."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("synthetic 1M-edge graph", 100_000, 1_000_000, 128), ("2.5M-edge shard", 250_000, 2_500_000, 256))


def timed(fn, launches):
    import torch
    for _ in range(3):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def measure(shape, runs, launches, torch_launches):
    """One shape, both forms; prints its lines."""
    import torch
    sys.path.insert(0, ROOT)
    from gnnome_amd import ops
    from gnnome_amd.synth import make_graph
    if not torch.cuda.is_available():
        raise SystemExit("attention_sum_time: no HIP device - this is a measurement, there is nothing to report without one")
    dev = torch.device("cuda", 0)
    name, n, e, H = SHAPES[shape]
    g = make_graph(n, e, seed=1)
    src, dst = g["src"].to(dev), g["dst"].to(dev)
    views = ops.GraphViews(src, dst, n)
    gen = torch.Generator(device=dev).manual_seed(0)
    feat = torch.randn(n, 3 * H, device=dev, generator=gen)
    el, er = (2 ** 0.5) * torch.randn(n, 4, device=dev, generator=gen), (2 ** 0.5) * torch.randn(n, 4, device=dev, generator=gen)
    bias = 0.1 * torch.randn(3 * H, device=dev, generator=gen)
    feat3, el3, er3 = feat.view(n, 3, H), el[:, :3].contiguous(), er[:, :3].contiguous()
    loops = torch.arange(n, device=dev)
    print(f"{name}: N={n} E={e} H={H} heads=3 on {torch.cuda.get_device_name(dev)}")
    for both in (False, True):
        gs = torch.cat([src.long(), dst.long(), loops] if both else [src.long(), loops])
        gd = torch.cat([dst.long(), src.long(), loops] if both else [dst.long(), loops])
        gd3 = gd[:, None].expand(-1, 3)
        out_k, out_t = torch.empty_like(feat), torch.empty_like(feat)

        def kernel():
            ops.node_attention_sum(feat, views, el, er, bias=bias, both=both, out=out_k)

        def by_torch():
            s = torch.nn.functional.leaky_relu(el3.index_select(0, gs) + er3.index_select(0, gd), 0.2)
            top = torch.full((n, 3), float("-inf"), device=dev).scatter_reduce_(0, gd3, s, "amax")
            w = torch.exp(s - top.index_select(0, gd))
            den = torch.zeros(n, 3, device=dev).index_add_(0, gd, w)
            num = torch.zeros(n, 3, H, device=dev).index_add_(0, gd, w[:, :, None] * feat3.index_select(0, gs))
            torch.add((num / den[:, :, None]).view(n, 3 * H), bias, out=out_t)

        kernel(), by_torch()
        torch.cuda.synchronize()
        diff = (out_k - out_t).abs().max().item()
        e2 = gs.numel() - n
        read, written = (e2 + n) * 3 * H * 4 + 2 * (e2 + n) * 16, n * 3 * H * 4
        print(f"  {'both lists' if both else 'directed'}: E'={e2}; max |kernel - torch composition| = {diff:.2e}; gather traffic {read / 1e6:.0f} MB read, "
              f"{written / 1e6:.0f} MB written")
        t_k, t_t = [], []
        for run in range(runs):
            t_t.append(timed(by_torch, torch_launches))
            t_k.append(timed(kernel, launches))
            print(f"    run {run}: torch composition {t_t[-1]:.4f} ms   node_attention_sum {t_k[-1]:.4f} ms")
        mt, mk = sorted(t_t)[len(t_t) // 2], sorted(t_k)[len(t_k) // 2]
        print(f"    median over runs: {mt:.4f} -> {mk:.4f} ms ({mt / mk:.1f}x); the gather's traffic at the kernel's time: "
              f"{(read + written) / mk / 1e6:.0f} GB/s")
        del gs, gd, gd3
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--torch-launches", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--shape", type=int, default=None, help="(internal) measure this one shape in this process")
    a = ap.parse_args()
    if a.shape is not None:
        measure(a.shape, a.runs, a.launches, a.torch_launches)
        return
    lines = [f"{a.runs} alternating runs per method, each the mean of {a.launches} (kernel) / {a.torch_launches} (torch) launches, ms per launch; "
             "quoted: the median over runs"]
    print(lines[0], flush=True)
    for shape in range(len(SHAPES)):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--shape", str(shape), "--runs", str(a.runs),
               "--launches", str(a.launches), "--torch-launches", str(a.torch_launches)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines.append(done.stdout.rstrip())
        print(lines[-1], flush=True)
        if done.returncode != 0:   # nothing more is started on the device after a step that failed or ran out of time
            raise SystemExit(f"attention_sum_time: the step for shape {shape} ended with status {done.returncode}")
    text = "\n".join(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
