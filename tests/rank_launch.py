"""How the partition tests start their ranks, once: `run_ranks` starts `world` fresh processes of a worker under one time limit, and
`process_group` is what every tests/dist_*_worker.py does before and after its own work."""
import contextlib
import os
import socket
import time

import torch
import torch.multiprocessing as mp


def run_ranks(worker, world, case, tmp_dir, timeout):
    """Start `world` ranks of `worker(rank, world, port, case path, out_dir)` as fresh processes and return what each saved as
    <tmp_dir>/rank<r>.pt, in rank order.  The spawn gets `timeout` seconds (the ranks start together, so one deadline serves all); the
    first rank that fails or overruns ends the others, and the caller's test fails."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.makedirs(tmp_dir, exist_ok=True)
    path = os.path.join(tmp_dir, "case.pt")
    torch.save(case, path)
    ctx = mp.spawn(worker, args=(world, port, path, str(tmp_dir)), nprocs=world, join=False)
    deadline = time.monotonic() + timeout
    try:
        while not ctx.join(timeout=max(0.0, min(1.0, deadline - time.monotonic()))):   # (raises as soon as one rank has failed)
            if time.monotonic() >= deadline:
                raise TimeoutError(f"a rank of world {world} was still running after {timeout} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join()
    return [torch.load(os.path.join(tmp_dir, f"rank{r}.pt"), weights_only=False) for r in range(world)]


@contextlib.contextmanager
def process_group(rank, world, port, case):
    """One rank's membership of the group, around its work: -> the case loaded from the path `case`.  The case chooses the transport:
    "transport": "nccl" is RCCL on device memory, one rank per GPU (the test box has one GPU => world 1), anything else gloo; with
    "force_collectives" one rank still issues every collective (gnnome_amd.dist.force_collectives)."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    g = torch.load(case, weights_only=False)
    if g.get("force_collectives"):
        os.environ["GNNOME_FORCE_COLLECTIVES"] = "1"
    if g.get("transport") == "nccl":
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        yield g
    finally:
        dist.destroy_process_group()
