#!/usr/bin/env python
"""(a) Launch time of gnnome_node_attention_sum_bwd_f32 (both launches, with the allocation of its 64-byte-per-node scratch and the zeroing
of dP's unused score columns: what ops.node_attention_sum_bwd(dP=) does per layer) against the only other way to get the three gradients on
the device - torch autograd over the torch composition of the same statement (tools/attention_sum_time.py's: index_select,
scatter_reduce(amax), exp, two index_add_), its graph retained so that the backward alone is timed - and (b) the time of one training step
of an 8-layer GATModel (engine_gat.train_forward + BCE + backward) against the same model's eval forward, on one device.

    python tools/attention_sum_bwd_time.py [--out profiles/attention_sum_bwd_time.txt] [--runs 3] [--launches 300] [--torch-launches 5] [--steps 20]

Shapes: the synthetic 1M-edge graph (100 000 nodes) at H = 128 and the 2.5M-edge shard (250 000 nodes) at H = 256, each directed (in-lists +
loops, E' = E) and with both lists (E' = 2 E), scores of scale 2, with a bias.  Each run's figure is the MEAN over back-to-back launches
between two device events (warmed up first), the two methods ALTERNATE run by run, and the figure quoted per method is the MEDIAN OVER RUNS.
The results are compared before anything is timed (reordered fp32 sums and the two exp's last bits).  The forward in its training form is
timed beside the plain one in the same way.  The traffic is computed from the shapes: per item of g' the destination walk reads a feat row
(3H floats) and a 16-byte score row, the source walk a G row and a 64-byte row; N rows of 3H floats are written.
No hub is timed: a hub's cost stays the kernel header's estimate.

Every part is measured by a child process of its own under a time limit (--step-timeout seconds); the parent opens no device and stops at
the first child that fails.  The first line of the output names the library's build (sha256 of libgnnome_hip.so, 16 digits)."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("synthetic 1M-edge graph", 100_000, 1_000_000, 128), ("2.5M-edge shard", 250_000, 2_500_000, 256))
PARTS = ("kernel0", "kernel1", "step")


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


def _device():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("attention_sum_bwd_time: no HIP device - this is a measurement, there is nothing to report without one")
    return torch.device("cuda", 0)


def _median(v):
    return sorted(v)[len(v) // 2]


def measure_kernel(shape, runs, launches, torch_launches):
    import torch
    sys.path.insert(0, ROOT)
    from gnnome_amd import ops
    from gnnome_amd.synth import make_graph
    dev = _device()
    name, n, e, H = SHAPES[shape]
    W = 3 * H
    g = make_graph(n, e, seed=1)
    src, dst = g["src"].to(dev), g["dst"].to(dev)
    views = ops.GraphViews(src, dst, n)
    gen = torch.Generator(device=dev).manual_seed(0)
    feat, G = torch.randn(n, W, device=dev, generator=gen), torch.randn(n, W, device=dev, generator=gen)
    el, er = (2 ** 0.5) * torch.randn(n, 4, device=dev, generator=gen), (2 ** 0.5) * torch.randn(n, 4, device=dev, generator=gen)
    el[:, 3] = er[:, 3] = 0.0
    bias = 0.1 * torch.randn(W, device=dev, generator=gen)
    loops = torch.arange(n, device=dev)
    print(f"(a) {name}: N={n} E={e} H={H} heads=3 on {torch.cuda.get_device_name(dev)}")
    for both in (False, True):
        gs = torch.cat([src.long(), dst.long(), loops] if both else [src.long(), loops])
        gd = torch.cat([dst.long(), src.long(), loops] if both else [dst.long(), loops])
        gd3 = gd[:, None].expand(-1, 3)
        A, stats = ops.node_attention_sum_stats(feat, views, el, er, bias=bias, both=both)
        plain = torch.empty_like(A)
        dP = torch.empty(n, W + 64, device=dev)

        def kernel():
            ops.node_attention_sum_bwd(G, views, feat, el, er, A, stats, bias=bias, both=both, dP=dP)

        def forward_plain():
            ops.node_attention_sum(feat, views, el, er, bias=bias, both=both, out=plain)

        def forward_stats():
            ops.node_attention_sum_stats(feat, views, el, er, bias=bias, both=both, out=A, stats=stats)

        lf, ll, lr = (t.clone().requires_grad_(True) for t in (feat, el, er))
        s = torch.nn.functional.leaky_relu(ll[:, :3].index_select(0, gs) + lr[:, :3].index_select(0, gd), 0.2)
        top = torch.full((n, 3), float("-inf"), device=dev).scatter_reduce(0, gd3, s.detach(), "amax")
        w = torch.exp(s - top.index_select(0, gd))
        den = torch.zeros(n, 3, device=dev).index_add(0, gd, w)
        num = torch.zeros(n, 3, H, device=dev).index_add(0, gd, w[:, :, None] * lf.view(n, 3, H).index_select(0, gs))
        out_t = (num / den[:, :, None]).view(n, W) + bias
        got_t = []

        def by_torch():
            got_t[:] = torch.autograd.grad(out_t, (lf, ll, lr), G, retain_graph=True)

        kernel(), by_torch(), forward_plain()
        torch.cuda.synchronize()
        same_fwd = torch.equal(plain, A)
        diffs = [(dP[:, :W] - got_t[0]).abs().max().item(), (dP[:, W:W + 3] - got_t[1][:, :3]).abs().max().item(),
                 (dP[:, W + 4:W + 7] - got_t[2][:, :3]).abs().max().item()]
        items = gs.numel()
        read = items * (2 * W * 4 + 16 + 64) + 3 * n * W * 4
        written = n * W * 4 + n * (16 + 16 + 64)
        print(f"  {'both lists' if both else 'directed'}: E'={items - n}; max |kernel - torch autograd| dfeat {diffs[0]:.2e} del {diffs[1]:.2e} "
              f"der {diffs[2]:.2e}; traffic {read / 1e6:.0f} MB read, {written / 1e6:.0f} MB written (derived); training-form forward "
              f"equals the plain one bit for bit: {same_fwd}")
        if not same_fwd or not all(d < 1e-2 for d in diffs):
            raise SystemExit("attention_sum_bwd_time: the two forms differ")
        t_k, t_t, t_p, t_s = [], [], [], []
        for run in range(runs):
            t_t.append(timed(by_torch, torch_launches))
            t_k.append(timed(kernel, launches))
            t_p.append(timed(forward_plain, launches))
            t_s.append(timed(forward_stats, launches))
            print(f"    run {run}: torch autograd {t_t[-1]:.4f} ms   node_attention_sum_bwd {t_k[-1]:.4f} ms   forward {t_p[-1]:.4f} ms   "
                  f"forward with statistics {t_s[-1]:.4f} ms")
        mt, mk, mp, ms = _median(t_t), _median(t_k), _median(t_p), _median(t_s)
        print(f"    median over runs: backward {mt:.4f} -> {mk:.4f} ms ({mt / mk:.1f}x), {mk / mp:.2f} forwards; the walks' traffic at the "
              f"kernel's time: {(read + written) / mk / 1e6:.0f} GB/s; forward {mp:.4f} ms, with statistics {ms:.4f} ms")
        del s, top, w, den, num, out_t, lf, ll, lr, gs, gd, gd3
        got_t.clear()
    sys.stdout.flush()


def measure_step(runs, steps):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from gnnome_amd import engine_gat, ops
    from gnnome_amd.features import degree_features
    from gnnome_amd.models import GATModel
    from gnnome_amd.synth import make_graph
    dev = _device()
    _, n, e_cnt, H = SHAPES[0]
    g = make_graph(n, e_cnt, seed=1)
    views = ops.GraphViews(g["src"].to(dev), g["dst"].to(dev), n)
    x, e, y = degree_features(views), g["e"].to(dev), g["y"].to(dev)
    torch.manual_seed(0)
    layers, hs = 8, 64
    for directed in (True, False):
        model = GATModel(2, 2, H, 16, layers, hs, "batch", dropout=0.2, directed=directed).to(dev)
        model.range_check = False   # (the timed loops must not synchronise the host per step)
        pw = torch.tensor([1.5], device=dev)

        def step():
            model.zero_grad(set_to_none=True)
            logits = engine_gat.train_forward(model, views, x, e)
            F.binary_cross_entropy_with_logits(logits.squeeze(-1), y, pos_weight=pw).backward()

        def forward():
            with torch.no_grad():
                model(views, x, e)

        t_s, t_f = [], []
        for _ in range(runs):
            model.eval()
            t_f.append(timed(forward, steps))
            model.train()
            t_s.append(timed(step, steps))
        print(f"(b) GATModel N={n} E={e_cnt} H={H} layers={layers} hs={hs} directed={directed} dropout=0.2: eval forward "
              + ", ".join(f"{t:.3f}" for t in t_f) + f" ms (median {_median(t_f):.3f}); one training step (forward + BCE + backward, no "
              "optimizer step) " + ", ".join(f"{t:.3f}" for t in t_s) + f" ms (median {_median(t_s):.3f}): {_median(t_s) / _median(t_f):.2f} forwards")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--torch-launches", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--part", choices=PARTS, default=None, help="(internal) measure this one part in this process")
    a = ap.parse_args()
    if a.part == "step":
        return measure_step(a.runs, a.steps)
    if a.part is not None:
        return measure_kernel(int(a.part[-1]), a.runs, a.launches, a.torch_launches)
    with open(os.path.join(ROOT, "gnnome_amd", "lib", "libgnnome_hip.so"), "rb") as f:
        build = hashlib.sha256(f.read()).hexdigest()[:16]
    lines = [f"build {build}; {a.runs} alternating runs per method, each the mean of {a.launches} (kernels) / {a.torch_launches} (torch) launches / "
             f"{a.steps} steps, ms; quoted: the median over runs"]
    print(lines[0], flush=True)
    for part in PARTS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--part", part, "--runs", str(a.runs),
               "--launches", str(a.launches), "--torch-launches", str(a.torch_launches), "--steps", str(a.steps)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines.append(done.stdout.rstrip())
        print(lines[-1], flush=True)
        if done.returncode != 0:   # nothing more is started on the device after a part that failed or ran out of time
            raise SystemExit(f"attention_sum_bwd_time: the part {part} ended with status {done.returncode}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
