"""World-size-N worker for the partitioned GatedGCNModel tests: one rank of an in-edge-only destination-range partition over gloo, with
the checker backend (tests/cpu_ops_gated.py) or, with device="cuda", the HIP kernels on the one GPU the ranks share (host-staged
collectives, as tests/dist_worker.py).  One run does everything a test module asks of a (graph, world) pair: the plan from the whole
edge list and from slices, the eval-mode forward, and one training step."""
import functools
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import rank_launch  # noqa: E402

PLAN_TENSORS = ("node_gid", "edge_gid", "srt_geid", "send_idx")
PLAN_VALUES = ("bounds", "n_own", "n_local", "n_score", "send_counts", "recv_counts", "score_pad", "num_edges_global", "in_edges_only")
VIEW_TENSORS = ("in_ptr", "srt_src", "srt_dst", "srt_eid", "out_ptr", "out_pos", "out_dst")


def worker(rank, world, port, case, out_dir):
    with rank_launch.process_group(rank, world, port, case) as g:
        import torch.nn.functional as F
        import gated_partition_graphs as gpg
        from gnnome_amd import dist as gdist
        from gnnome_amd.models import GatedGCNModel
        m = GatedGCNModel(2, 2, gpg.HIDDEN, 16, gpg.LAYERS, gpg.SCORE_HIDDEN, "batch", dropout=0.0)
        m.load_state_dict(g["state_dict"])
        if g.get("device") == "cuda":
            from gnnome_amd import ops as backend
            where = torch.device("cuda", 0)
            m.to(where)
        else:
            import cpu_ops_gated
            backend, where = cpu_ops_gated.BACKEND, torch.device("cpu")
        x, e, y, pw = (g[k].to(where) for k in ("x", "e", "y", "pos_weight"))
        bounds = g["bounds"][world]
        part = gdist.PartitionedGraph.from_global(g["src"], g["dst"], g["num_nodes"], rank, world, where, ops=backend, in_edges_only=True,
                                                  bounds=bounds)
        # the same plan from this rank's SLICE of the edge list (uneven slices, rank order)
        E = int(g["src"].numel())
        cuts = [0] + [min(E, (E * (r + 1)) // world + (7 if r + 1 < world else 0)) for r in range(world)]
        a, b = cuts[rank], cuts[rank + 1]
        sl = gdist.PartitionedGraph.from_slices(g["src"][a:b], g["dst"][a:b], g["num_nodes"], rank, world, where, ops=backend,
                                                in_edges_only=True, bounds=bounds)
        sliced_equal = (all(torch.equal(getattr(sl, k).cpu(), getattr(part, k).cpu()) for k in PLAN_TENSORS)
                        and all(getattr(sl, k) == getattr(part, k) for k in PLAN_VALUES)
                        and all(torch.equal(getattr(sl.views, k).cpu(), getattr(part.views, k).cpu()) for k in VIEW_TENSORS)
                        and torch.equal(sl.shuffle_edge_rows(g["e"][a:b]).cpu(), part.local_edge_rows(g["e"]).cpu()))

        m.eval()
        logits = gdist.PartitionedRunner(m, part, x, e, where, ops=backend).forward().squeeze(1)

        m.train()
        m.training_step = "in_edge"
        out = gdist.PartitionedRunner(m, part, x, e, where, ops=backend).train_forward()
        loss = F.binary_cross_entropy_with_logits(out.squeeze(-1), y, pos_weight=pw)
        loss.backward()
        if where.type == "cuda":
            torch.cuda.synchronize()
        torch.save({"logits": logits.cpu(), "train_logits": out.detach().squeeze(1).cpu(), "loss": loss.detach().cpu(),
                    "grads": {k: p.grad.cpu() for k, p in m.named_parameters()},
                    "buffers": {k: v.detach().cpu().clone() for k, v in m.named_buffers()},
                    "sliced_equal": bool(sliced_equal), "n_own": part.n_own, "n_local": part.n_local, "n_score": part.n_score,
                    "e_local": int(part.edge_gid.numel()), "send": part.send_counts, "recv": part.recv_counts,
                    "in_degree_local": (part.views.in_ptr[1:] - part.views.in_ptr[:-1]).cpu(), "srt_geid": part.srt_geid.cpu()},
                   os.path.join(out_dir, f"rank{rank}.pt"))


run_ranks = functools.partial(rank_launch.run_ranks, worker)
