#!/usr/bin/env python
"""Does the interior / boundary split of the partitioned GCNModel / SAGEModel pay for itself?  Forward (eval) and training step of both
models on 2 and 4 ranks over RCCL, one rank per device, with the split (interior rows launched under the halo exchange, boundary rows
after it) against ONE unsplit launch after the exchange (dist.PartitionedRunner(..., split=)):

    python tools/baseline_partition_time.py [--out profiles/baseline_partition_time.txt] [--runs 5] [--iters 20]

Shape: a synthetic banded graph of about 1M edges (100 000 nodes, 10 out-edges each within a band of 2000 ids), H = 128, 8 layers,
directed=True.  Each run's figure is the MEAN over back-to-back iterations between two device events on rank 0 after a barrier (warmed
up first); the two forms ALTERNATE run by run; quoted per form: the median over runs and the spread (max - min) over runs.  The logits of
the two forms are compared bit for bit before anything is timed.  The decision rule of DESIGN 7c: the split is the default only if its
median is not above the unsplit median by more than the larger of the two spreads.

Needs as many devices as ranks: with fewer, the tool records that the case could not be run and measures nothing.  Every world size is
measured by child processes under a time limit (--step-timeout seconds); the parent opens no device and stops at the first failure."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DEG, BAND, H, LAYERS, HS = 100_000, 10, 2000, 128, 8, 64


def banded_graph(seed=1):
    import torch
    g = torch.Generator().manual_seed(seed)
    src = torch.arange(N).repeat_interleave(DEG)
    dst = (src + torch.randint(1, BAND, (N * DEG,), generator=g)) % N
    E = src.numel()
    x = torch.stack([torch.log1p(torch.bincount(dst, minlength=N).float()), torch.log1p(torch.bincount(src, minlength=N).float())], 1)
    e = torch.stack([torch.randn(E, generator=g), 0.9 + 0.1 * torch.rand(E, generator=g)], 1)
    return dict(src=src.int(), dst=dst.int(), x=x, e=e, y=(torch.rand(E, generator=g) < 0.6).float())


def rank_main(rank, world, port, runs, iters):
    import torch
    import torch.distributed as dist
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from gnnome_amd import dist as gdist
    from gnnome_amd import engine_baselines as eb
    from gnnome_amd.models import GCNModel, SAGEModel
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev = torch.device("cuda", rank)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    try:
        g = banded_graph()
        part = gdist.PartitionedGraph.from_global(g["src"], g["dst"], N, rank, world, dev)
        y, pw = g["y"].to(dev), torch.tensor([1.5], device=dev)
        if rank == 0:
            print(f"world {world}: rank 0 owns {part.n_own} of {part.n_local} local nodes, scores {part.n_score} of {int(part.edge_gid.numel())} local edges")
        for cls in (GCNModel, SAGEModel):
            torch.manual_seed(0)
            model = cls(2, 2, H, 16, LAYERS, HS, "batch", dropout=0.0).to(dev)
            model.range_check = False   # (the timed loop must not synchronise the host)
            plan = eb.plan_for(gdist.hip_ops, part, True)
            evalr = {split: gdist.PartitionedRunner(model.eval(), part, g["x"], g["e"], dev, split=split) for split in (True, False)}
            model.train()
            trainr = {split: gdist.PartitionedRunner(model, part, g["x"], g["e"], dev, split=split) for split in (True, False)}
            model.eval()

            def forward(split):
                return evalr[split].forward()

            def step(split):
                model.zero_grad(set_to_none=True)
                F.binary_cross_entropy_with_logits(trainr[split].train_forward().squeeze(-1), y, pos_weight=pw).backward()

            def timed(run, split):
                fn = lambda: run(split)  # noqa: E731
                for _ in range(3):
                    fn()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                dist.barrier()
                start.record()
                for _ in range(iters):
                    fn()
                stop.record()
                torch.cuda.synchronize()
                return start.elapsed_time(stop) / iters

            same = torch.equal(forward(True), forward(False))
            if rank == 0:
                print(f"  {cls.__name__}: interior / boundary rows of rank 0: {plan.rows_fwd[0].numel()} / {plan.rows_fwd[1].numel()} (forward), "
                      f"{plan.rows_bwd[0].numel()} / {plan.rows_bwd[1].numel()} (backward); equal logits bits {same}")
            if not same:
                raise SystemExit("baseline_partition_time: the two forms differ")
            for name, fn in (("forward", forward), ("step", step)):
                model.train(name == "step")
                t = {True: [], False: []}
                for _ in range(runs):
                    for split in (False, True):
                        t[split].append(timed(fn, split))
                if rank == 0:
                    med = {s: sorted(v)[len(v) // 2] for s, v in t.items()}
                    spread = {s: max(v) - min(v) for s, v in t.items()}
                    keep = med[True] <= med[False] + max(spread.values())
                    print(f"    {name}: unsplit median {med[False]:.3f} ms (spread {spread[False]:.3f}), split median {med[True]:.3f} ms "
                          f"(spread {spread[True]:.3f}) -> the split is {'not slower beyond the spread' if keep else 'SLOWER beyond the spread'}")
        sys.stdout.flush()
    finally:
        dist.destroy_process_group()


def measure_world(world, runs, iters):
    import socket

    import torch
    import torch.multiprocessing as mp
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < world:
        print(f"world {world}: COULD NOT BE RUN - {have} device(s) visible, one per rank needed; nothing measured")
        return
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(rank_main, args=(world, port, runs, iters), nprocs=world, join=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--world", type=int, default=None, help="(internal) measure this world size in this process tree")
    a = ap.parse_args()
    if a.world is not None:
        return measure_world(a.world, a.runs, a.iters)
    lines = [f"banded graph N={N} E={N * DEG} band={BAND}, H={H}, {LAYERS} layers, hs={HS}, directed=True; {a.runs} alternating runs per form, each "
             f"the mean of {a.iters} iterations, ms; quoted: median and spread (max - min) over runs"]
    print(lines[0], flush=True)
    for world in (2, 4):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--world", str(world), "--runs", str(a.runs),
               "--iters", str(a.iters)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines.append(done.stdout.rstrip())
        print(lines[-1], flush=True)
        if done.returncode != 0:   # nothing more is started on the devices after a world size that failed or ran out of time
            raise SystemExit(f"baseline_partition_time: world {world} ended with status {done.returncode}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
