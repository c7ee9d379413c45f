"""World-size-N worker of the doubled-plan tests: one rank of GatedGCNModel(directed=False) on the in-edge-only partition of the doubled edge
list, over gloo - with the checker backend (tests/cpu_ops_gated.py) or, with device="cuda", the HIP kernels on the one GPU the ranks share
(host-staged collectives, as tests/dist_gated_worker.py).  One run does what a test module asks of a (norm, world) pair: the plan from the
whole edge list and from slices, and - unless the case says plan_only - the eval-mode forward and one in-edge training step."""
import functools
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import rank_launch  # noqa: E402

PLAN_TENSORS = ("node_gid", "edge_gid", "srt_geid", "send_idx", "enc_rows", "score_rows")
PLAN_VALUES = ("bounds", "n_own", "n_local", "n_score", "n_score_original", "send_counts", "recv_counts", "score_pad", "num_edges_global",
               "num_edges_original", "in_edges_only", "doubled")
VIEW_TENSORS = ("in_ptr", "srt_src", "srt_dst", "srt_eid", "out_ptr", "out_pos", "out_dst")


def same_plan(a, b):
    return (all(torch.equal(getattr(a, k).cpu(), getattr(b, k).cpu()) for k in PLAN_TENSORS)
            and all(getattr(a, k) == getattr(b, k) for k in PLAN_VALUES)
            and all(torch.equal(getattr(a.views, k).cpu(), getattr(b.views, k).cpu()) for k in VIEW_TENSORS)
            and all(torch.equal(getattr(a.scored.views, k).cpu(), getattr(b.scored.views, k).cpu()) for k in VIEW_TENSORS))


def plan_record(part):
    """The plan as the tests read it, in GLOBAL ids: per local sorted position the destination, the source and the original edge."""
    v = part.views
    return dict(n_own=part.n_own, n_local=part.n_local, n_score=part.n_score, n_score_original=part.n_score_original,
                e_local=int(part.edge_gid.numel()), num_edges_global=part.num_edges_global, num_edges_original=part.num_edges_original,
                doubled=part.doubled, lo=part.lo, hi=part.hi, send=part.send_counts, recv=part.recv_counts, bounds=part.bounds,
                edge_gid=part.edge_gid.cpu(), srt_geid=part.srt_geid.cpu(), enc_rows=part.enc_rows.cpu(), score_rows=part.score_rows.cpu(),
                srt_dst=part.node_gid[v.srt_dst.long()].cpu(), srt_src=part.node_gid[v.srt_src.long()].cpu(),
                srt_enc=part.enc_rows[v.srt_eid.long()].cpu(),
                in_degree_local=(v.in_ptr[1:] - v.in_ptr[:-1]).cpu())


def worker(rank, world, port, case, out_dir):
    with rank_launch.process_group(rank, world, port, case) as g:
        import torch.nn.functional as F
        import gated_doubled_graphs as gdg
        from gnnome_amd import dist as gdist
        from gnnome_amd.models import GatedGCNModel
        if g.get("device") == "cuda":
            from gnnome_amd import ops as backend
            where = torch.device("cuda", 0)
        else:
            import cpu_ops_gated
            backend, where = cpu_ops_gated.BACKEND, torch.device("cpu")
        x, e, y, pw = (g[k].to(where) for k in ("x", "e", "y", "pos_weight"))
        bounds = g["bounds"][world]
        build = functools.partial(gdist.PartitionedGraph.from_global, g["src"], g["dst"], g["num_nodes"], rank, world, where, ops=backend,
                                  in_edges_only=True, doubled=True)
        part = build(bounds=bounds)
        # the same plan from this rank's SLICE of the original edge list (uneven slices, rank order), with the given and the default bounds
        E = int(g["src"].numel())
        cuts = [0] + [min(E, (E * (r + 1)) // world + (7 if r + 1 < world else 0)) for r in range(world)]
        a, b = cuts[rank], cuts[rank + 1]
        sliced = functools.partial(gdist.PartitionedGraph.from_slices, g["src"][a:b], g["dst"][a:b], g["num_nodes"], rank, world, where,
                                   ops=backend, in_edges_only=True, doubled=True)
        sl = sliced(bounds=bounds)
        out = plan_record(part)
        out["sliced_equal"] = bool(same_plan(sl, part) and torch.equal(sl.shuffle_edge_rows(g["e"][a:b]).cpu(), part.local_edge_rows(g["e"]).cpu()))
        out["default_bounds_equal"] = bool(same_plan(sliced(), build()))
        out["slice_degrees_are_the_original_graphs"] = bool(
            torch.equal(sl.global_degrees.cpu(), torch.stack([torch.bincount(g["dst"].long(), minlength=g["num_nodes"]),
                                                              torch.bincount(g["src"].long(), minlength=g["num_nodes"])])))
        if not g.get("plan_only"):
            m = GatedGCNModel(2, 2, gdg.HIDDEN, 16, gdg.LAYERS, gdg.SCORE_HIDDEN, g["norm"], dropout=0.0, directed=False)
            m.load_state_dict(g["state_dict"])
            m.to(where).eval()
            logits = gdist.PartitionedRunner(m, part, x, e, where, ops=backend).forward().squeeze(1)
            m.train()
            m.training_step = "in_edge"
            res = gdist.PartitionedRunner(m, part, x, e, where, ops=backend).train_forward()
            loss = F.binary_cross_entropy_with_logits(res.squeeze(-1), y, pos_weight=pw)
            loss.backward()
            if where.type == "cuda":
                torch.cuda.synchronize()
            out.update(logits=logits.cpu(), train_logits=res.detach().squeeze(1).cpu(), loss=loss.detach().cpu(),
                       grads={k: p.grad.cpu() for k, p in m.named_parameters()},
                       buffers={k: v.detach().cpu().clone() for k, v in m.named_buffers()})
        torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))


def trainer_worker(rank, world, port, case, out_dir):
    """One rank of trainer.train_partitioned(overfit=True) with a GatedGCNModel subclass whose constructor sets directed=False and whose
    training step is the in-edge one: the loop builds the doubled plan itself."""
    with rank_launch.process_group(rank, world, port, case) as g:
        from gnnome_amd import models, trainer

        class GatedGCNInEdgeUndirected(models.GatedGCNModel):
            training_step = "in_edge"

            def __init__(self, *args, **kwargs):
                super().__init__(*args, **dict(kwargs, directed=False))

        kw = dict(g["kwargs"])
        if g.get("device") == "cuda":
            kw["device"] = torch.device("cuda", 0)
        else:
            import cpu_trainer_ops
            kw.update(ops=cpu_trainer_ops.BACKEND, device=torch.device("cpu"))
        trace = []
        records = trainer.train_partitioned(g["train_set"], g["train_set"], overfit=True, trace=trace, model_class=GatedGCNInEdgeUndirected, **kw)
        torch.save({"records": records, "trace": trace}, os.path.join(out_dir, f"rank{rank}.pt"))


run_ranks = functools.partial(rank_launch.run_ranks, worker)
run_trainer_ranks = functools.partial(rank_launch.run_ranks, trainer_worker)


def one_epoch_at_worlds_one_and_two(gr, tmp_path, device=None):
    """train_partitioned, one epoch, one graph, overfit=True, at world 1 and at world 2 -> per world (rank 0's result, the model file)."""
    hp = {"dim_latent": 64, "num_gnn_layers": 2, "hidden_edge_scores": 64, "num_epochs": 1, "num_nodes_per_cluster": 1000, "masking": False,
          "use_symmetry_loss": False}
    graph = {k: gr[k] for k in ("src", "dst", "num_nodes", "e", "y")}
    res = {}
    for world in (1, 2):
        d = tmp_path / f"w{world}"
        kwargs = dict(out="t", hyperparameters=hp, dropout=0.0, seed=3, models_dir=str(d / "m"), checkpoints_dir=str(d / "c"))
        outs = run_trainer_ranks(world, dict(train_set=[graph], kwargs=kwargs, **({} if device is None else {"device": device})), str(d / "ranks"),
                                 timeout=240)
        assert all(o["records"] == outs[0]["records"] for o in outs)
        res[world] = (outs[0], torch.load(d / "m" / "model_t_seed3.pt", map_location="cpu", weights_only=False))
    return res


def plain_torch_epoch(gr, initial_state, pos_weight, dtype, lr):
    """The same epoch in plain torch (tests/gated_graphs.py's restatement, directed=False, x from the ORIGINAL graph's degrees): one Adam
    step -> the parameters after it, as tests/test_dist_trainer_gloo.py::_oracle_loop does for the symmetric model."""
    import torch.nn.functional as F
    import gated_graphs as gg
    from gnnome_amd import features
    src, dst, n = gr["src"].long(), gr["dst"].long(), gr["num_nodes"]
    x = features.partition_degree_features(torch.bincount(dst, minlength=n).float(), torch.bincount(src, minlength=n).float(), torch.arange(n)).to(dtype)
    leaves = {k: (v.clone().to(dtype).requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.clone().to(dtype)
                  if v.is_floating_point() else v.clone()) for k, v in initial_state.items()}
    params = [v for v in leaves.values() if v.requires_grad]
    opt = torch.optim.Adam(params, lr=lr)
    logits = gg.gated_model(leaves, src, dst, n, x, gr["e"].to(dtype), 2, directed=False, training=True)
    loss = F.binary_cross_entropy_with_logits(logits.squeeze(-1), gr["y"].to(dtype), pos_weight=torch.tensor([pos_weight], dtype=dtype))
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.item(), {k: v.detach().double() for k, v in leaves.items() if v.requires_grad}


def rel_l2(a, b):
    num = sum(((a[k].double() - b[k].double()) ** 2).sum().item() for k in b) ** 0.5
    return num / sum((b[k].double() ** 2).sum().item() for k in b) ** 0.5
