#!/usr/bin/env python
"""One training step of GatedGCNModel through its two routes - `training_step = "symmetric"` (the symmetric model's step behind an adapter
with a zero A_3) against `"in_edge"` (the one-direction step on csrc/node_aggregate_in_bwd.hip) - and the two new backward launches
alone against the entries the symmetric step uses for the same quantities, on one device, in alternating order.

    python tools/gated_step_time.py [--out profiles/gated_step_time.txt] [--runs 3] [--steps 10] [--launches 300] [--layers 8]

Shapes: the synthetic 1M-edge graph (100 000 nodes) at H = 128 and the 2.5M-edge shape (250 000 nodes) at H = 256.
  step:    forward + BCE-with-logits + backward of one model (BatchNorm, dropout 0, directed=True, the same parameters for both routes),
           each run's figure the MEAN over `steps` steps between two device events after two warm-up steps per route.
  kernels: gnnome_node_aggregate_in_bwd_f32 (two launches) against gnnome_node_aggregate_raw_f32 mode 2 (tables Tb := 0, Tf) +
           gnnome_agg_edge_bwd_f32 (zero Tb / Ub / A3h), and gnnome_node_aggregate_in_raw_f32 against mode 1 with a zero A3h; each run's
           figure the MEAN over `launches` calls.
`runs` alternating runs per route; the figure quoted is the MEDIAN OVER RUNS.  Every part is measured by a child process of its own under
a time limit (--part-timeout seconds); the parent opens no device and stops at the first part that fails."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("synthetic 1M-edge graph", 100_000, 1_000_000, 128), ("2.5M-edge shape", 250_000, 2_500_000, 256))
PARTS = ("step0", "kernels0", "step1", "kernels1")


def timed(fn, count, warm):
    import torch
    for _ in range(warm):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(count):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / count


def _device():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gated_step_time: no HIP device - this is a measurement, there is nothing to report without one")
    return torch.device("cuda", 0)


def _median(v):
    return sorted(v)[len(v) // 2]


def _alternate(routes, runs, count, warm):
    """routes: [(label, fn)] -> lines; run r times every route in turn."""
    times = {label: [] for label, _ in routes}
    lines = []
    for run in range(runs):
        for label, fn in routes:
            times[label].append(timed(fn, count, warm))
        lines.append(f"  run {run}: " + "   ".join(f"{label} {times[label][-1]:.4f} ms" for label, _ in routes))
    (la, _), (lb, _) = routes
    ma, mb = _median(times[la]), _median(times[lb])
    lines.append(f"  median over runs: {la} {ma:.4f} -> {lb} {mb:.4f} ms ({ma / mb:.2f}x)")
    return lines


def measure_step(shape, runs, steps, layers):
    import torch
    import torch.nn.functional as F
    from gnnome_amd.graph import views_for
    from gnnome_amd.models import GatedGCNModel
    from gnnome_amd.synth import make_graph
    dev = _device()
    name, n, e, H = SHAPES[shape]
    g = make_graph(n, e, seed=1)
    views = views_for((g["src"], g["dst"], n), dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(n, 2, device=dev, generator=gen)
    ef = g["e"].to(dev)
    y = (torch.rand(e, device=dev, generator=gen) < 0.5).float()
    torch.manual_seed(0)
    model = GatedGCNModel(2, 2, H, 16, layers, 64, "batch", dropout=0.0).to(dev).train()

    def step_of(route):
        def step():
            model.training_step = route
            model.zero_grad(set_to_none=True)
            loss = F.binary_cross_entropy_with_logits(model(views, x, ef).squeeze(-1), y)
            loss.backward()
            return loss
        return step

    sym, ine = step_of("symmetric"), step_of("in_edge")
    l_sym, l_in = sym().item(), ine().item()
    lines = [f"step, {name}: N={n} E={e} H={H}, {layers} layers, BatchNorm, fp32 storage, directed=True; loss symmetric {l_sym:.6f} in_edge {l_in:.6f}"]
    lines += _alternate([("symmetric", sym), ("in_edge", ine)], runs, steps, 2)
    print("\n".join(lines), flush=True)


def measure_kernels(shape, runs, launches):
    import torch
    from gnnome_amd import ops
    from gnnome_amd.synth import make_graph
    dev = _device()
    name, n, e, H = SHAPES[shape]
    g = make_graph(n, e, seed=1)
    views = ops.GraphViews(g["src"].to(dev), g["dst"].to(dev), n)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    ee, Tf, Uf, zero = rnd(e, H), rnd(n, H), rnd(n, H), torch.zeros(n, H, device=dev)
    P5 = rnd(n, 5 * H)
    P5[:, 2 * H:3 * H] = 0.0
    P4 = torch.cat([P5[:, :2 * H], P5[:, 3 * H:]], 1).contiguous()   # the one-direction model's [N,4H] projection: the same A1h | A2h
    de_new, de_old = torch.zeros(e, H, device=dev), torch.zeros(e, H, device=dev)
    dA = torch.empty(n, H, device=dev)

    def bwd_new():
        ops.node_aggregate_in_bwd(ee, Tf, Uf, P4[:, H:2 * H], views, de_new, out=dA)

    def bwd_old():
        ops.node_aggregate_raw(ee, None, zero, Tf, views, 2, n)
        ops.agg_edge_bwd(ee, Tf, Uf, zero, zero, P5[:, H:2 * H], P5[:, 2 * H:3 * H], views, de_old)

    def raw_new():
        ops.node_aggregate_in_raw(ee, P4[:, :H], P4[:, H:2 * H], views)

    def raw_old():
        ops.node_aggregate_raw(ee, P5[:, :H], P5[:, H:2 * H], P5[:, 2 * H:3 * H], views, 1, n)

    bwd_new(), bwd_old()
    torch.cuda.synchronize()
    d_de = (de_new - de_old).abs().max().item()
    d_dA = (dA - ops.node_aggregate_raw(ee, None, zero, Tf, views, 2, n)[1]).abs().max().item()
    lines = [f"kernels, {name}: N={n} E={e} H={H}; new against existing entries: max |d de| {d_de:.3e}, max |d dA2h| {d_dA:.3e}; least bytes of the "
             f"backward: e twice + de read and written = {4 * e * H * 4 / 1e6:.0f} MB"]
    lines.append(" backward: node_aggregate_raw mode 2 + agg_edge_bwd (zero tables) against node_aggregate_in_bwd")
    lines += _alternate([("mode 2 + agg_edge_bwd", bwd_old), ("node_aggregate_in_bwd", bwd_new)], runs, launches, 10)
    lines.append(" forward: node_aggregate_raw mode 1 (A3h = 0) against node_aggregate_in_raw (allocations of the outputs included in both)")
    lines += _alternate([("mode 1", raw_old), ("node_aggregate_in_raw", raw_new)], runs, launches, 10)
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--part-timeout", type=int, default=240)
    ap.add_argument("--part", choices=PARTS, default=None, help="(internal) measure this one part in this process")
    a = ap.parse_args()
    if a.part is not None:
        shape = int(a.part[-1])
        return measure_step(shape, a.runs, a.steps, a.layers) if a.part.startswith("step") else measure_kernels(shape, a.runs, a.launches)
    with open(os.path.join(ROOT, "gnnome_amd", "lib", "libgnnome_hip.so"), "rb") as f:
        build = hashlib.sha256(f.read()).hexdigest()[:16]
    lines = [f"build {build}; {a.runs} alternating runs per route, each the mean of {a.steps} steps / {a.launches} launches, ms; quoted: the median over runs"]
    print(lines[0], flush=True)
    for part in PARTS:
        cmd = ["timeout", "-k", "10", str(a.part_timeout), sys.executable, os.path.abspath(__file__), "--part", part, "--runs", str(a.runs),
               "--steps", str(a.steps), "--launches", str(a.launches), "--layers", str(a.layers)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines.append(done.stdout.rstrip())
        print(lines[-1], flush=True)
        if done.returncode != 0:   # nothing more is started on the device after a part that failed or ran out of time
            raise SystemExit(f"gated_step_time: the part {part} ended with status {done.returncode}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
