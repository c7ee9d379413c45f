"""World-size-N worker for the partitioned GCNModel / SAGEModel tests: one rank of the default destination-range partition over gloo, with
the checker backend (tests/cpu_ops_baselines.py) or, with device="cuda", the HIP kernels on the one GPU the ranks share (host-staged
collectives, as tests/dist_gated_worker.py).  One run does everything a test module asks of a (graph, world) pair: for both models and
both `directed` values the eval-mode forward - with the interior / boundary split and with the unsplit launch - and one training step
(dropout 0), and once a SAGEModel step with feat_drop masks handed in."""
import functools
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import rank_launch  # noqa: E402

DROPOUT = 0.25
CONFIGS = [(kind, directed, 0.0) for kind in ("gcn", "sage") for directed in (True, False)] + [("sage", True, DROPOUT)]


def split_of(kind, directed):
    """Which launch form the training step of a configuration takes: both forms run under both models."""
    return (kind == "gcn") == directed


def worker(rank, world, port, case, out_dir):
    with rank_launch.process_group(rank, world, port, case) as g:
        import torch.nn.functional as F
        import baseline_partition_graphs as bpg
        from gnnome_amd import dist as gdist
        from gnnome_amd import engine_baselines as eb
        from gnnome_amd import train
        if g.get("device") == "cuda":
            from gnnome_amd import ops as backend
            where = torch.device("cuda", 0)
        else:
            import cpu_ops_baselines
            backend, where = cpu_ops_baselines.BACKEND, torch.device("cpu")
        x, e, y, pw = (g[k].to(where) for k in ("x", "e", "y", "pos_weight"))
        part = gdist.PartitionedGraph.from_global(g["src"], g["dst"], g["num_nodes"], rank, world, where, ops=backend, bounds=g["bounds"][world])
        out = {"n_own": part.n_own, "n_local": part.n_local, "lo": part.lo, "hi": part.hi, "node_gid": part.node_gid.cpu(), "configs": {}}
        for kind, directed, dropout in CONFIGS:
            m = bpg.model(kind, directed, dropout).to(where)
            res = {}
            if dropout == 0.0:
                m.eval()
                for split in (True, False):
                    runner = gdist.PartitionedRunner(m, part, x, e, where, ops=backend, split=split)
                    res["logits_split" if split else "logits"] = runner.forward().squeeze(1).cpu()
                plan = eb.plan_for(backend, part, directed)
                res["plan"] = {k: getattr(plan, k).cpu() for k in ("din_rsqrt", "dout_rsqrt", "din_inv")}
                res["rows_fwd"], res["rows_bwd"] = [t.cpu() for t in plan.rows_fwd], [t.cpu() for t in plan.rows_bwd]
                res["lists"] = {k: getattr(plan.lists, k).cpu() for k in ("in_ptr", "srt_src", "out_ptr", "out_dst")}
            m.train()
            keep = train.dropout_mask
            if dropout > 0.0:
                train.dropout_mask = bpg.HandedMasks(bpg.known_masks(g, dropout), part.lo, part.hi)
            try:
                logits = gdist.PartitionedRunner(m, part, x, e, where, ops=backend, split=split_of(kind, directed)).train_forward()
                loss = F.binary_cross_entropy_with_logits(logits.squeeze(-1), y, pos_weight=pw)
                loss.backward()
            finally:
                train.dropout_mask = keep
            if where.type == "cuda":
                torch.cuda.synchronize()
            res.update(train_logits=logits.detach().squeeze(1).cpu(), loss=loss.detach().cpu(),
                       grads={k: p.grad.cpu() for k, p in m.named_parameters()})
            out["configs"][(kind, directed, dropout)] = res
        torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))


run_ranks = functools.partial(rank_launch.run_ranks, worker)
