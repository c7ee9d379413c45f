"""World-size-N worker for tests/test_dist_symmetry_gloo.py and tests/test_hip_symmetry_partition.py: the REVERSED pass of
SymGatedGCNModel on a destination-range partition - eval logits of run_partitioned(..., reverse=True), or one symmetry step
(train.py:159-170) through PartitionedRunner.train_forward() / train_forward(reverse=True) - on CPU ranks over gloo with the checker
backend, or on ranks that share the test box's one GPU with the HIP kernels as compute (gloo, host-staged; world 1: RCCL with
GNNOME_FORCE_COLLECTIVES=1)."""
import functools
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import rank_launch  # noqa: E402


def worker(rank, world, port, case, out_dir):
    with rank_launch.process_group(rank, world, port, case) as g:
        cuda = g.get("device") == "cuda"
        import cpu_ops
        import gnnome_amd
        from gnnome_amd import dist as gdist
        from gnnome_amd import engine
        from oracle.symgated_oracle import symmetry_loss as torch_symmetry_loss
        m = gnnome_amd.models.SymGatedGCNModel(2, 2, g["hidden"], 16, g["layers"], 64, "batch", dropout=0.0).eval()
        m.load_state_dict(g["state_dict"])
        if cuda:
            from gnnome_amd import ops as backend
            from gnnome_amd.loss import symmetry_loss
            where = torch.device("cuda", rank if g.get("transport") == "nccl" else 0)
            m.to(where)
            g = {k: (v.to(where) if k in ("x", "x_rev", "e", "y", "pos_weight") else v) for k, v in g.items()}
        else:
            backend, where, symmetry_loss = cpu_ops, torch.device("cpu"), torch_symmetry_loss
        part = gdist.PartitionedGraph.from_global(g["src"], g["dst"], g["num_nodes"], rank, world, where, ops=backend, bounds=g.get("bounds"))
        edges_before = (part.views.srt_src.data_ptr(), part.views.srt_eid.data_ptr(), part.views.out_pos.data_ptr())
        out = {"n_own": part.n_own, "n_local": part.n_local, "n_score": part.n_score, "e_local": int(part.edge_gid.numel()),
               "lo": part.lo, "srt_geid": part.srt_geid.cpu(), "node_gid": part.node_gid.cpu(), "edge_gid": part.edge_gid.cpu(),
               "backend": dist.get_backend()}
        if g.get("train"):
            m.train()
            runner = gdist.PartitionedRunner(m, part, g["x"], g["e"], where, ops=backend, x_rev_global=g["x_rev"])
            org = runner.train_forward()
            rev = runner.train_forward(reverse=True)     # (must not release or overwrite what the first pass saved)
            loss = symmetry_loss(org.squeeze(-1), rev.squeeze(-1), g["y"], g["pos_weight"], g["alpha"])
            loss.backward()
            out.update(org=org.detach().squeeze(1).cpu(), rev=rev.detach().squeeze(1).cpu(), loss=loss.detach().cpu(),
                       grads={k: p.grad.cpu() for k, p in m.named_parameters()},
                       buffers={k: b.detach().cpu().clone() for k, b in m.named_buffers()})
        else:
            prep = engine.Prepared(m, where)
            x_rev = part.local_node_rows(g["x_rev"]).contiguous()
            e_loc = part.local_edge_rows(g["e"]).contiguous()
            with torch.no_grad():
                rev = gdist.run_partitioned(backend, prep, part, x_rev, e_loc, reverse=True)
                org = gdist.run_partitioned(backend, prep, part, part.local_node_rows(g["x"]).contiguous(), e_loc)
                runner = gdist.PartitionedRunner(m, part, g["x"], g["e"], where, ops=backend, x_rev_global=g["x_rev"])
                again = runner.forward(reverse=True)
            out.update(rev=rev.cpu(), org=org.cpu(), runner_rev=again.squeeze(1).cpu())
        # one plan, one set of views: the reversed pass left the plan's orientation and its arrays where they were
        out["plan_untouched"] = (not part.views.transposed and
                                 edges_before == (part.views.srt_src.data_ptr(), part.views.srt_eid.data_ptr(), part.views.out_pos.data_ptr()))
        torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))


run_ranks = functools.partial(rank_launch.run_ranks, worker)
