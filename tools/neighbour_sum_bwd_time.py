#!/usr/bin/env python
"""(a) Launch time of gnnome_node_neighbour_sum_bwd_f32 with its epilogue against the sequence it replaces - the forward kernel on the
reversed views, then the add, the multiply and the ReLU gate as separate passes over [N,H] - and (b) the time of one training step of
GCNModel and SAGEModel (engine_baselines.train_forward + BCE + backward), on one device.  tools/neighbour_sum_time.py's method:

    python tools/neighbour_sum_bwd_time.py [--out profiles/neighbour_sum_bwd_time.txt] [--runs 3] [--launches 1000] [--steps 30]

Shape: the synthetic 1M-edge graph (100 000 nodes) at H = 128, directed and with both lists, with each model's operand set - GCN: rscale,
oscale, y; SAGE: rscale, add and g the two halves of one [N,2H] table, mult, y.  Each run's figure is the MEAN over back-to-back launches
between two device events (warmed up first), the two methods ALTERNATE run by run, and the figure quoted per method is the MEDIAN OVER
RUNS.  The two results are compared bit for bit before anything is timed.  The passes the fused form saves are computed from the shapes:
each separate pass reads and writes N H 4 bytes per operand.

Every part is measured by a child process of its own under a time limit (--step-timeout seconds); the parent opens no device and stops at
the first child that fails."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, E, H = 100_000, 1_000_000, 128
PARTS = ("kernel", "gcn", "sage")


def timed(fn, launches):
    import torch
    for _ in range(5):
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
        raise SystemExit("neighbour_sum_bwd_time: no HIP device - this is a measurement, there is nothing to report without one")
    return torch.device("cuda", 0)


def measure_kernel(runs, launches):
    import torch
    sys.path.insert(0, ROOT)
    from gnnome_amd import ops
    from gnnome_amd.synth import make_graph
    dev = _device()
    g = make_graph(N, E, seed=1)
    views = ops.GraphViews(g["src"].to(dev), g["dst"].to(dev), N)
    rev = views.reversed()
    gen = torch.Generator(device=dev).manual_seed(0)
    dT = torch.randn(N, 2 * H, device=dev, generator=gen)
    dA = dT[:, H:].contiguous()
    rs, osc = 0.25 + torch.rand(N, device=dev, generator=gen), 0.25 + torch.rand(N, device=dev, generator=gen)
    mult = (torch.rand(N, H, device=dev, generator=gen) >= 0.2).float() / 0.8
    y = torch.relu(torch.randn(N, H, device=dev, generator=gen))
    out_f, s, v, out_s = (torch.empty(N, H, device=dev) for _ in range(4))
    zero = torch.zeros((), device=dev)
    print(f"(a) synthetic 1M-edge graph: N={N} E={E} H={H} on {torch.cuda.get_device_name(dev)}; one [N,H] pass = {N * H * 4 / 1e6:.0f} MB read + as much written")
    for both in (False, True):
        def gcn_fused():
            ops.node_neighbour_sum_bwd(dA, views, rscale=rs, oscale=osc, both=both, y=y, out=out_f)

        def gcn_separate():   # the parent's kernel on the reversed views, then the gate
            ops.node_neighbour_sum(dA, rev, sscale=rs, dscale=osc, both=both, out=s)
            torch.where(y > 0, s, zero, out=out_s)

        def sage_fused():
            ops.node_neighbour_sum_bwd(dT[:, H:], views, rscale=rs, both=both, add=dT[:, :H], mult=mult, y=y, out=out_f)

        def sage_separate():  # ... then the add, the multiply and the gate
            ops.node_neighbour_sum(dT[:, H:], rev, sscale=rs, both=both, out=s)
            torch.add(dT[:, :H], s, out=v)
            v.mul_(mult)
            torch.where(y > 0, v, zero, out=out_s)

        for name, fused, separate, saved in (("GCN operands (rscale, oscale, y)", gcn_fused, gcn_separate, 1),
                                             ("SAGE operands (rscale, add, mult, y)", sage_fused, sage_separate, 3)):
            fused(), separate()
            torch.cuda.synchronize()
            same = torch.equal(out_f, out_s)
            print(f"  {'both lists' if both else 'directed'}, {name}: equal bits {same}; separate form: {saved} more [N,H] write+read pass(es) (derived)")
            if not same:
                raise SystemExit("neighbour_sum_bwd_time: the two forms differ")
            t_s, t_f = [], []
            for run in range(runs):
                t_s.append(timed(separate, launches))
                t_f.append(timed(fused, launches))
                print(f"    run {run}: separate {t_s[-1]:.4f} ms   fused {t_f[-1]:.4f} ms")
            ms, mf = sorted(t_s)[len(t_s) // 2], sorted(t_f)[len(t_f) // 2]
            print(f"    median over runs: {ms:.4f} -> {mf:.4f} ms ({ms / mf:.2f}x, {(ms - mf) * 1e3:.1f} us saved)")
    sys.stdout.flush()


def measure_step(kind, runs, steps):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from gnnome_amd import engine_baselines, ops
    from gnnome_amd.features import degree_features
    from gnnome_amd.models import GCNModel, SAGEModel
    from gnnome_amd.synth import make_graph
    dev = _device()
    g = make_graph(N, E, seed=1)
    views = ops.GraphViews(g["src"].to(dev), g["dst"].to(dev), N)
    x, e, y = degree_features(views), g["e"].to(dev), g["y"].to(dev)
    torch.manual_seed(0)
    layers, hs = 8, 64
    model = (GCNModel if kind == "gcn" else SAGEModel)(2, 2, H, 16, layers, hs, "batch", dropout=0.2).to(dev).train()
    model.range_check = False   # (the timed loop must not synchronise the host per step)
    pw = torch.tensor([1.5], device=dev)

    def step():
        model.zero_grad(set_to_none=True)
        logits = engine_baselines.train_forward(model, views, x, e)
        F.binary_cross_entropy_with_logits(logits.squeeze(-1), y, pos_weight=pw).backward()

    times = [timed(step, steps) for _ in range(runs)]
    print(f"(b) one training step of {type(model).__name__}: N={N} E={E} H={H} layers={layers} hs={hs} directed=True"
          f"{' dropout=0.2' if kind == 'sage' else ''} (forward + BCE + backward, no optimizer step): "
          + ", ".join(f"{t:.3f}" for t in times) + f" ms; median {sorted(times)[len(times) // 2]:.3f} ms")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--part", choices=PARTS, default=None, help="(internal) measure this one part in this process")
    a = ap.parse_args()
    if a.part == "kernel":
        return measure_kernel(a.runs, a.launches)
    if a.part is not None:
        return measure_step(a.part, a.runs, a.steps)
    lines = [f"{a.runs} alternating runs per method, each the mean of {a.launches} launches (kernels) / {a.steps} steps, ms; quoted: the median over runs"]
    print(lines[0], flush=True)
    for part in PARTS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--part", part, "--runs", str(a.runs),
               "--launches", str(a.launches), "--steps", str(a.steps)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines.append(done.stdout.rstrip())
        print(lines[-1], flush=True)
        if done.returncode != 0:   # nothing more is started on the device after a part that failed or ran out of time
            raise SystemExit(f"neighbour_sum_bwd_time: the part {part} ended with status {done.returncode}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
