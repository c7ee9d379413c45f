"""World-size-N worker for the partitioned GATModel tests: one rank of the default destination-range partition over gloo, with the checker
backend (tests/cpu_ops_gat.py) or, with device="cuda", the HIP kernels on the one GPU the ranks share (host-staged collectives, as
tests/dist_baseline_worker.py).  One run does everything a test module asks of a (graph, world) pair:
for every configuration of gat_partition_cases.CONFIGS the eval-mode forward (dropout 0) and one training step - with feat_drop masks
handed in where dropout > 0 - and the exchanges each of them started."""
import functools
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import rank_launch  # noqa: E402


def worker(rank, world, port, case, out_dir):
    with rank_launch.process_group(rank, world, port, case) as g:
        import torch.nn.functional as F
        import gat_partition_cases as gpc
        from gnnome_amd import dist as gdist
        from gnnome_amd import train
        if g.get("device") == "cuda":
            from gnnome_amd import ops as backend
            where = torch.device("cuda", 0)
        else:
            import cpu_ops_gat
            backend, where = cpu_ops_gat.BACKEND, torch.device("cpu")
        x, e, y, pw = (g[k].to(where) for k in ("x", "e", "y", "pos_weight"))
        part = gdist.PartitionedGraph.from_global(g["src"], g["dst"], g["num_nodes"], rank, world, where, ops=backend, bounds=g["bounds"][world])
        out = {"n_own": part.n_own, "n_local": part.n_local, "lo": part.lo, "hi": part.hi, "configs": {}}
        for directed, dropout in gpc.CONFIGS:
            m = gpc.model(directed, dropout).to(where)
            res = {}
            if dropout == 0.0:
                m.eval()
                with gpc.CountedExchanges() as c:
                    res["logits"] = gdist.GATPartitionedRunner(m, part, x, e, where, ops=backend).forward().squeeze(1).cpu()
                res["eval_exchanges"] = (list(c.starts), c.transposes)
            m.train()
            keep = train.dropout_mask
            if dropout > 0.0:
                train.dropout_mask = gpc.HandedMasks(gpc.known_masks(g, dropout), part.lo, part.hi)
            try:
                with gpc.CountedExchanges() as c:
                    logits = gdist.GATPartitionedRunner(m, part, x, e, where, ops=backend).train_forward()
                    res["forward_exchanges"] = (list(c.starts), c.transposes)
                    loss = F.binary_cross_entropy_with_logits(logits.squeeze(-1), y, pos_weight=pw)
                    loss.backward()
                res["backward_exchanges"] = (c.starts[len(res["forward_exchanges"][0]):], c.transposes - res["forward_exchanges"][1])
            finally:
                train.dropout_mask = keep
            if where.type == "cuda":
                torch.cuda.synchronize()
            res.update(train_logits=logits.detach().squeeze(1).cpu(), loss=loss.detach().cpu(),
                       grads={k: p.grad.cpu() for k, p in m.named_parameters()})
            out["configs"][(directed, dropout)] = res
        torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))


run_ranks = functools.partial(rank_launch.run_ranks, worker)
