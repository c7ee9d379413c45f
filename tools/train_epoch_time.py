"""One training epoch of gnnome_amd.trainer with the reference defaults (configs/hyperparameters.py: 1000 nodes per cluster, masking
80-100 %, symmetry loss, 64 wide, 8 layers) on a synthetic banded graph with random labels, and its parts:

  epoch wall time and steps per second (trainer.train, overfit: no validation pass)
  median step time (forward on the cluster, forward on its reverse, symmetry loss, backward, Adam; synchronised per step)
  partition time (cluster_partition of one masked graph)
  cluster-input time for all clusters of that graph: the packed kernel (features.cluster_inputs, one call) against the
  per-cluster torch path (features.partition_degree_features twice + the e / y gathers, cluster by cluster) on the same parts

    python tools/train_epoch_time.py [--nodes 500000] [--edges-per-node 10] [--repeat 5]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gnnome_amd import features, ops, trainer  # noqa: E402
from gnnome_amd.partition import cluster_partition  # noqa: E402
from gnnome_amd.synth import make_graph  # noqa: E402


def timed(fn, repeat):
    out, ts = None, []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, statistics.median(ts), ts


def per_cluster_torch(parts, in_deg, out_deg, e, y, outer_nid, outer_eid):
    out = []
    for sub in parts:
        nid, eid = outer_nid[sub.nid], outer_eid[sub.eid]
        out.append((features.partition_degree_features(in_deg, out_deg, nid), features.partition_degree_features(in_deg, out_deg, nid, True),
                    e[eid], y[eid]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=500_000)
    ap.add_argument("--edges-per-node", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30, help="steps timed one by one for the median step time")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = make_graph(a.nodes, a.nodes * a.edges_per_node, seed=1)
    hp = trainer.hyperparameters_with({"num_epochs": 1})
    res = {"nodes": a.nodes, "edges": a.nodes * a.edges_per_node, "num_nodes_per_cluster": hp["num_nodes_per_cluster"]}

    # the parts: one masked graph, its clusters, the inputs both ways
    trainer.set_seed(1)
    gr = trainer._Graph("synthetic", g, dev)
    masked = features.mask_graph_strandwise(gr.views, 0.9, dev)
    _, k = trainer.plan(masked.num_nodes(), hp["num_nodes_per_cluster"])
    parts, t_part, _ = timed(lambda: list(cluster_partition(masked, k, extra_cached_hops=1, device=dev).values()), 2)
    res.update(clusters=len(parts), partition_ms=t_part * 1e3)
    packed, t_packed, _ = timed(lambda: features.cluster_inputs(parts, gr.in_deg, gr.out_deg, gr.e, gr.y, masked.nid, masked.eid), a.repeat)
    ref, t_torch, _ = timed(lambda: per_cluster_torch(parts, gr.in_deg, gr.out_deg, gr.e, gr.y, masked.nid, masked.eid), a.repeat)
    same = all(torch.equal(p.e, r[2]) and torch.equal(p.y, r[3]) and torch.allclose(p.x, r[0], rtol=1e-5, atol=1e-6, equal_nan=True)
               for p, r in zip(packed, ref))
    res.update(inputs_packed_ms=t_packed * 1e3, inputs_per_cluster_torch_ms=t_torch * 1e3, inputs_speedup=t_torch / t_packed,
               inputs_agree=bool(same))

    # the median step, synchronised step by step
    model = trainer.SymGatedGCNModel(2, 2, hp["dim_latent"], hp["hidden_ne_features"], hp["num_gnn_layers"], hp["hidden_edge_scores"],
                                     hp["normalization"], dropout=hp["dropout"]).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=hp["lr"])
    pw = torch.tensor([2.0], device=dev)
    log = torch.zeros((len(parts), 5), dtype=torch.float64, device=dev)
    step_ts = []
    for i, (sub, ci) in enumerate(list(zip(parts, packed))[:a.steps]):
        if sub.eid.numel() == 0:
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        org = model(sub.views, ci.x, ci.e).squeeze(-1)
        rev = model(sub.views.reversed(), ci.x_rev, ci.e).squeeze(-1)
        trainer._step(model, opt, org, rev, ci.y, pw, hp["alpha"], log[i], ops.edge_loss)
        torch.cuda.synchronize()
        step_ts.append(time.perf_counter() - t0)
    res["median_step_ms"] = statistics.median(step_ts[2:] or step_ts) * 1e3

    # one whole epoch through the loop (first epoch includes the library's one-time set-up; run it twice, report the second)
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            recs = trainer.train([g], None, out=f"t{rep}", hyperparameters={"num_epochs": 1}, overfit=True, seed=1,
                                 models_dir=os.path.join(tmp, "m"), checkpoints_dir=os.path.join(tmp, "c"), device=dev)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        res.update(epoch_s=recs[0]["seconds"], train_call_s=wall, steps=recs[0]["train/steps"],
                   steps_per_s=recs[0]["train/steps"] / recs[0]["seconds"], skipped_clusters=recs[0]["train/skipped_clusters"],
                   train_loss=recs[0]["train/loss"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
