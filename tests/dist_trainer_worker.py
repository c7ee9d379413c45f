"""World-size-N worker for tests/test_dist_trainer_gloo.py and tests/test_hip_trainer_partition.py: one rank of trainer.train_partitioned,
on CPU ranks over gloo with the checker backend (tests/cpu_trainer_ops.py), or on ranks that share the test box's one GPU with the HIP
kernels as compute (gloo, host-staged; world 1: RCCL with GNNOME_FORCE_COLLECTIVES=1).  A rank saves what the call returned - or the
exception it raised, as text - so the test compares the ranks; run_ranks gives the whole spawn one deadline."""
import functools
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import rank_launch  # noqa: E402


def odd_bounds(src, dst, num_nodes, world):
    """dist.split_by_incident_edges with every inner boundary moved to an odd node id: the cut falls between nodes 2r and 2r + 1 of a read."""
    from gnnome_amd import dist as gdist
    b = gdist.split_by_incident_edges(src.long(), dst.long(), num_nodes, world)
    return [0] + [min(x | 1, num_nodes - 1) for x in b[1:-1]] + [num_nodes]


def worker(rank, world, port, case, out_dir):
    with rank_launch.process_group(rank, world, port, case) as g:
        cuda = g.get("device") == "cuda"
        from gnnome_amd import models, trainer
        class GatedGCNInEdge(models.GatedGCNModel):
            training_step = "in_edge"

        def model_class(name):
            return GatedGCNInEdge if name == "GatedGCNInEdge" else getattr(models, name)
        kw = dict(g["kwargs"])
        if cuda:
            kw["device"] = torch.device("cuda", rank if g.get("transport") == "nccl" else 0)
        else:
            import cpu_trainer_ops
            kw.update(ops=cpu_trainer_ops.BACKEND, device=torch.device("cpu"))
        if g.get("odd_bounds"):
            kw["bounds"] = odd_bounds
        real_rand, calls = torch.rand, [0]
        if rank > 0:
            if g.get("peers_never_draw"):
                def no_rand(*a, **k):
                    raise AssertionError(f"rank {rank} called torch.rand: the masks are rank 0's")
                torch.rand = no_rand
            if g.get("peers_never_write"):
                def no_save(obj, f, *a, **k):   # (pickling a tensor for a collective saves into a buffer: that is no file)
                    if isinstance(f, (str, os.PathLike)):
                        raise AssertionError(f"rank {rank} called torch.save({f}): the files are rank 0's")
                    return torch.serialization.save(obj, f, *a, **k)
                torch.save = no_save
        elif g.get("empty_mask_from_draw") is not None:
            def one_read(*a, **k):   # from the given draw on, the mask keeps read 0 alone: no rank can own an in-edge
                calls[0] += 1
                t = real_rand(*a, **k)
                if calls[0] > g["empty_mask_from_draw"]:
                    t.fill_(1.0)
                    t[0] = 0.0
                return t
            torch.rand = one_read
        out = {"rank": rank, "backend": dist.get_backend(), "results": []}
        for call in g.get("calls", [{}]):     # one train_partitioned per entry (its keywords, "model": a class name); an error ends the list
            call = dict(call)
            res = {"trace": []}
            out["results"].append(res)
            try:
                res["records"] = trainer.train_partitioned(g["train_set"], g["valid_set"], trace=res["trace"],
                                                           model_class=model_class(call.pop("model", "SymGatedGCNModel")), **dict(kw, **call))
            except (ValueError, NotImplementedError) as ex:
                res["error"] = f"{type(ex).__name__}: {ex}"
                if not g.get("go_on_after_error"):
                    break
        torch.save = torch.serialization.save
        torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))


run_ranks = functools.partial(rank_launch.run_ranks, worker)
