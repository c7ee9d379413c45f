"""The training loop: train.py:188-450 of the reference on this package, from a dataset of labelled graphs to a trained model.

    records = trainer.train(train_set, valid_set, out="run", seed=1)        # -> one record per epoch
    python -m gnnome_amd.trainer --train DIR --valid DIR --name run [--overfit] [--resume] [--dropout P] [--seed S] [--gpu I]
    records = trainer.train_partitioned(train_set, valid_set, out="run", seed=1)   # every rank of a process group: graphs larger than one GPU
    python -m gnnome_amd.trainer --train DIR --valid DIR --name run --gpus N [--transport nccl|gloo]

Per epoch, as the reference: shuffle the training graphs; if `masking`, keep a random fraction of the reads
(features.mask_graph_strandwise); train on the whole graph if `num_nodes_per_cluster >= N`, otherwise on the
`N // num_nodes_per_cluster + 1` clusters of partition.cluster_partition, shuffled; each step runs the symmetry loss (or BCE),
zero_grad / backward / step.  Then validation under torch.no_grad() and model.eval() (masked as well), the model saved at a new
minimum of the validation loss (of the training loss under `overfit`), ReduceLROnPlateau stepped, a checkpoint written.

Where the inputs come from (train.py:125-186, utils/data_utils.py:31-41): degrees are the FULL graph's stored degrees, e is the full
graph's z-scored edge features computed once per graph at load, labels are y[eid] composed through the mask.  All clusters of a graph
get their inputs from ONE call of gnnome_cluster_inputs_f32 (features.cluster_inputs); the whole-graph mode is the same call with one
cluster.  Loss and the confusion counts come out of one pass of the edge-loss kernel and stay on the device in a [steps, 5] log that
is copied to the host once per epoch: the loop itself adds no host synchronisation per step.

Deliberate deviations from the reference:
  * clusters without edges are skipped and counted in the epoch record (the reference divides by zero there);
  * the first overfit epoch saves the model (the reference's min([]) raises at that point);
  * the checkpoint also holds the scheduler state and the random state (and the order of the training graphs), and resume restores
    them, so a resumed run reproduces the run that was not interrupted;
  * the epoch records are returned and appended as JSON lines next to the checkpoint, in place of wandb.
"""
import argparse
import functools
import json
import os
import random
import re
import sys
import time
import types
from datetime import datetime

import numpy as np
import torch
from torch.optim.lr_scheduler import ReduceLROnPlateau

from . import features, metrics, ops
from .models import SymGatedGCNModel
from .partition import cluster_partition

# configs/hyperparameters.py, the keys the loop reads
DEFAULT_HYPERPARAMETERS = {
    "seed": 1,
    "dim_latent": 64,
    "num_gnn_layers": 8,
    "node_features": 2,
    "edge_features": 2,
    "hidden_ne_features": 16,
    "hidden_edge_scores": 64,
    "normalization": "batch",
    "dropout": 0.2,
    "num_epochs": 5,
    "lr": 1e-4,
    "use_symmetry_loss": True,
    "alpha": 0.1,
    "num_nodes_per_cluster": 1000,
    "k_extra_hops": 1,
    "patience": 2,
    "decay": 0.95,
    "masking": True,
    "mask_frac_low": 80,
    "mask_frac_high": 100,
    "nb_pos_enc": 0,            # add_positional_encoding (utils/data_utils.py:53-54): 0 = off, as the reference ships it
    "type_pos_enc": "none",     # 'RW' | 'PR'; anything else sets no pe
}

CHECKPOINT_KEYS = ("epoch", "model_state_dict", "optim_state_dict", "loss_train", "loss_valid", "scheduler_state_dict", "rng_state")
METRIC_KEYS = ("loss", "fp_rate", "fn_rate", "acc", "precision", "recall", "f1", "acc_inv", "precision_inv", "recall_inv", "f1_inv")


def hyperparameters_with(overrides=None):
    """configs/hyperparameters.py's values, updated by `overrides` (the reference's key names; an unknown key raises)."""
    hp = dict(DEFAULT_HYPERPARAMETERS)
    for k, v in (overrides or {}).items():
        if k not in hp:
            raise KeyError(f"unknown hyperparameter {k!r}")
        hp[k] = v
    return hp


def set_seed(seed):
    """utils/utils.py:10-30: Python, numpy, torch and the device generators."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def plan(num_nodes, num_nodes_per_cluster):
    """train.py:316-320: -> (whole graph?, num_clusters).  The whole graph if num_nodes_per_cluster >= N, otherwise N // npc + 1 clusters."""
    if num_nodes_per_cluster >= num_nodes:
        return True, 1
    return False, num_nodes // num_nodes_per_cluster + 1


def pos_weight_of(graphs):
    """train.py:239: 1 / mean over the training graphs of #(round(y) == 1) / #(round(y) == 0).  `graphs`: (name, y) pairs."""
    ratios = []
    for name, y in graphs:
        r = torch.round(torch.as_tensor(y).float())
        pos, neg = int((r == 1).sum()), int((r == 0).sum())
        if neg == 0:
            raise ValueError(f"graph {name}: no negative edges (round(y) == 0), the positive-class weight is undefined")
        ratios.append(pos / neg)
    if not ratios:
        raise ValueError("no training graphs")
    mean = sum(ratios) / len(ratios)
    if mean == 0:
        raise ValueError("no positive edges in the training graphs, the positive-class weight is undefined")
    return 1.0 / mean


def compute_fp_fn_rates(TP, TN, FP, FN):
    """train.py:23-27."""
    fp_rate = FP / (FP + TN) if (FP + TN) != 0 else 0.0
    fn_rate = FN / (FN + TP) if (FN + TP) != 0 else 0.0
    return fp_rate, fn_rate


def compute_metrics(TP, TN, FP, FN, loss):
    """train.py:30-54 from the four counts (the reference counts them from the logits first)."""
    acc, precision, recall, f1 = metrics.calculate_metrics(TP, TN, FP, FN)
    acc_inv, precision_inv, recall_inv, f1_inv = metrics.calculate_metrics_inverse(TP, TN, FP, FN)
    fp_rate, fn_rate = compute_fp_fn_rates(TP, TN, FP, FN)
    return {"loss": loss, "fp_rate": fp_rate, "fn_rate": fn_rate, "acc": acc, "precision": precision, "recall": recall, "f1": f1,
            "acc_inv": acc_inv, "precision_inv": precision_inv, "recall_inv": recall_inv, "f1_inv": f1_inv}


def average_epoch_metrics(step_metrics):
    """train.py:57-59 over a list of compute_metrics dicts -> {key: mean} (plain floats)."""
    if not step_metrics:
        return {}
    return {k: float(np.mean([m[k] for m in step_metrics])) for k in step_metrics[0]}


def metrics_from_log(log):
    """[steps, 5] rows (loss, TP, TN, FP, FN) on the host -> the per-step compute_metrics dicts."""
    rows = log.tolist() if hasattr(log, "tolist") else log
    return [compute_metrics(int(tp), int(tn), int(fp), int(fn), float(loss)) for loss, tp, tn, fp, fn in rows]


# ---- datasets --------------------------------------------------------------------------------------------------------------

def _dataset_files(path):
    found = []
    for name in os.listdir(path):
        m = re.fullmatch(r"(\d+)\.(pt|dgl)", name)
        if m:
            found.append((int(m.group(1)), m.group(2), os.path.join(path, name)))
    return sorted(found)


def load_dataset(ds, hyperparameters=None, device=None):
    """A list of graph dicts (as gfa.read_gfa / dgl_io return them, each with y) -> [(name, dict)]; or a directory of <idx>.pt files
    (torch.save of such a dict; trainer.process writes them), sorted by idx, and of <idx>.dgl files when DGL can be imported.
    hyperparameters: with nb_pos_enc > 0 every graph goes through positional.add_positional_encoding on `device`, as the reference's
    dataset class does with every loaded graph (graph_dataset.py:50-52).  At nb_pos_enc = 0, the default, that call would only store the
    degrees (data_utils.py:50-57), which _Graph counts at load anyway: the graphs are returned exactly as they were read."""
    named = _read_dataset(ds)
    hp = hyperparameters_with(hyperparameters)
    if hp["nb_pos_enc"] > 0:
        from .positional import add_positional_encoding
        for _, g in named:
            add_positional_encoding(g, hp["nb_pos_enc"], hp["type_pos_enc"], device=device)
    return named


def _read_dataset(ds):
    if isinstance(ds, (str, os.PathLike)):
        out = []
        try:
            import dgl  # noqa: F401
            have_dgl = True
        except ImportError:
            have_dgl = False
        for idx, kind, path in _dataset_files(ds):
            if kind == "pt":
                out.append((path, torch.load(path, map_location="cpu", weights_only=False)))
            elif have_dgl:
                from .dgl_io import load_dgl_file
                out.append((path, load_dgl_file(path)))
        if not out:
            raise ValueError(f"{ds}: no <idx>.pt graphs" + ("" if have_dgl else " (.dgl files need DGL, which is not installed)"))
        return out
    return [(f"graph {i}", g) for i, g in enumerate(ds)]


def hip_backend():
    """The namespace the loops reach the device through - the package's own kernels: `kernels` (what dist.PartitionedRunner takes as
    ops=), GraphViews, cluster_inputs (features.cluster_inputs), edge_loss (ops.edge_loss), stored_degrees, edge_features.
    train_partitioned(ops=...) takes another one (the CPU tests: a torch restatement)."""
    return types.SimpleNamespace(kernels=ops, GraphViews=ops.GraphViews, cluster_inputs=features.cluster_inputs, edge_loss=ops.edge_loss,
                                 stored_degrees=features.stored_degrees, edge_features=features.edge_features)


class _Graph:
    """One dataset graph on the device, prepared once at load: the full graph's views, stored degrees, z-scored e and labels (and the
    edge list itself, in edge-id order: train_partitioned masks and plans from it)."""

    def __init__(self, name, g, device, be=None):
        be = be or hip_backend()
        y = g.get("y") if isinstance(g, dict) else None
        if y is None:
            raise ValueError(f"graph {name}: no labels (y); build training graphs with gfa.read_gfa(..., training=True) or trainer.process")
        self.name = name
        self.num_nodes = int(g["num_nodes"])
        src = torch.as_tensor(g["src"]).to(device=device, dtype=torch.int32).contiguous()
        dst = torch.as_tensor(g["dst"]).to(device=device, dtype=torch.int32).contiguous()
        self.src, self.dst = src, dst
        self.views = be.GraphViews(src, dst, self.num_nodes)
        self.num_edges = int(src.numel())
        self.y = torch.as_tensor(y).to(device=device, dtype=torch.float32).contiguous()
        if self.y.numel() != self.num_edges:
            raise ValueError(f"graph {name}: {self.y.numel()} labels for {self.num_edges} edges")
        if g.get("e") is not None:
            self.e = torch.as_tensor(g["e"]).to(device=device, dtype=torch.float32).contiguous()
        else:
            if g.get("overlap_length") is None or g.get("overlap_similarity") is None:
                raise ValueError(f"graph {name}: needs overlap_length and overlap_similarity (or e) for the edge features")
            self.e = be.edge_features(torch.as_tensor(g["overlap_length"]).to(device).float(),
                                      torch.as_tensor(g["overlap_similarity"]).to(device).float())
        if g.get("in_deg") is not None and g.get("out_deg") is not None:
            self.in_deg = torch.as_tensor(g["in_deg"]).to(device=device, dtype=torch.float32).contiguous()
            self.out_deg = torch.as_tensor(g["out_deg"]).to(device=device, dtype=torch.float32).contiguous()
        else:
            self.in_deg, self.out_deg = (t.contiguous() for t in be.stored_degrees(self.views))


def process(gfa, reads, out_path, device=None, maf=None, maf_chr=None, maf_parser="host", coverage=False):
    """One training graph file: gfa.read_gfa(gfa, reads_path=reads, training=True) with the labels computed on the device and the
    stored degrees (graph_parser.py: ndata in_deg / out_deg) added, written with torch.save to `out_path` (<dir>/<idx>.pt).  maf, maf_chr,
    maf_parser: the simulator's MAF file as the source of the read positions (read_gfa's keywords; `reads` may then be None).
    coverage=True also stores labels.reference_coverage(g) under "coverage": what of the reference the reads cover, per chromosome."""
    from .gfa import read_gfa
    g = read_gfa(gfa, reads_path=reads, training=True, labels="device", maf=maf, maf_chr=maf_chr, maf_parser=maf_parser)
    device = device or torch.device("cuda", torch.cuda.current_device())
    views = ops.GraphViews(g["src"].to(device=device, dtype=torch.int32), g["dst"].to(device=device, dtype=torch.int32), g["num_nodes"])
    g["in_deg"], g["out_deg"] = (t.cpu() for t in features.stored_degrees(views))
    if coverage:
        from .labels import reference_coverage
        g["coverage"] = reference_coverage(g, device=device)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    torch.save(g, out_path)
    return g


# ---- the step --------------------------------------------------------------------------------------------------------------

class _LossAndCounts(torch.autograd.Function):
    """loss.symmetry_loss / loss.bce_loss that also leaves (loss, TP, TN, FP, FN) of the org logits in a row of the device log:
    one edge-loss kernel gives all of them (ops.edge_loss(..., need_counts=True); `edge_loss`: the backend's entry)."""

    @staticmethod
    def forward(ctx, org, rev, labels, pos_weight, alpha, row, edge_loss):
        need = org.requires_grad or (rev is not None and rev.requires_grad)
        loss, d_org, d_rev, tfpn = edge_loss(org.detach().float().contiguous(), None if rev is None else rev.detach().float().contiguous(),
                                                labels, pos_weight, alpha, need_grad=need, need_counts=True)
        row[0].copy_(loss[0])
        row[1:5].copy_(tfpn)
        ctx.save_for_backward(d_org, d_rev)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        d_org, d_rev = ctx.saved_tensors
        return (None if d_org is None else g * d_org), (None if d_rev is None else g * d_rev), None, None, None, None, None


def _graph_steps(gr, hp, device, training, trace, phase, epoch):
    """Mask, plan, partition and build the inputs of one graph -> the list of (views, ClusterInputs, record) steps, and the
    number of clusters skipped for having no edges."""
    fraction, outer_nid, outer_eid, work = None, None, None, gr.views
    if hp["masking"]:
        fraction = random.randint(hp["mask_frac_low"], hp["mask_frac_high"]) / 100
        work = features.mask_graph_strandwise(gr.views, fraction, device)   # torch.rand on the device, as train.py:92
        outer_nid, outer_eid = work.nid, work.eid
    n = work.num_nodes if isinstance(work, ops.GraphViews) else work.num_nodes()
    whole, num_clusters = plan(n, hp["num_nodes_per_cluster"])
    if whole:
        views = work if isinstance(work, ops.GraphViews) else work.views
        parts = [types.SimpleNamespace(nid=torch.arange(n, device=device), eid=torch.arange(views.num_edges, device=device),
                                       views=views, src=None, dst=None)]
    else:
        parts = list(cluster_partition(work, num_clusters, extra_cached_hops=hp["k_extra_hops"], device=device).values())
    inputs = features.cluster_inputs(parts, gr.in_deg, gr.out_deg, gr.e, gr.y, outer_nid=outer_nid, outer_eid=outer_eid,
                                     need_rev=hp["use_symmetry_loss"])
    steps = list(zip(parts, inputs))
    if training and not whole:
        random.shuffle(steps)                                                  # train.py:336
    kept = [s for s in steps if s[0].eid.numel() > 0]
    if trace is not None:
        for sub, _ in kept:
            nid, eid = sub.nid, sub.eid
            if outer_nid is not None:
                nid, eid = outer_nid[nid], outer_eid[eid]
            v = sub.views
            src = sub.src if sub.src is not None else _edge_src_dst(v)[0]
            dst = sub.dst if sub.dst is not None else _edge_src_dst(v)[1]
            trace.append({"phase": phase, "epoch": epoch, "graph": gr.name, "fraction": fraction, "whole": whole,
                          "nid": nid.cpu(), "eid": eid.cpu(), "src": src.cpu(), "dst": dst.cpu(), "num_nodes": int(sub.nid.numel())})
    return [(sub.views, ci) for sub, ci in kept], len(steps) - len(kept)


def _edge_src_dst(views):
    src = torch.empty(views.num_edges, dtype=torch.int32, device=views.device)
    dst = torch.empty_like(src)
    src[views.srt_eid.long()], dst[views.srt_eid.long()] = views.srt_src, views.srt_dst
    return src, dst


def _model_step(model, views, x, e):
    """`model(views, x, e)` - except for GCNModel / SAGEModel / GATModel in train mode, whose call refuses train mode and whose training
    step is the explicit entry engine_baselines.train_forward (GATModel: engine_gat.train_forward)."""
    if model.training and getattr(model, "kind", None) in ("gcn", "sage"):
        from . import engine_baselines
        return engine_baselines.train_forward(model, views, x, e)
    if model.training and getattr(model, "kind", None) == "gat":
        from . import engine_gat
        return engine_gat.train_forward(model, views, x, e)
    return model(views, x, e)


def _step(model, optimizer, org, rev, y, pos_weight, alpha, row, edge_loss, rec=None, grads=False):
    """One step from its logits on: loss and counts into `row` of the device log, then - `optimizer` not None - zero_grad / backward /
    step.  rec: the step's trace entry (gets the org logits, and with `grads` the gradients before the optimizer step).  Nothing here
    waits for the device unless a trace is kept."""
    loss = _LossAndCounts.apply(org, rev, y, pos_weight, alpha, row, edge_loss)
    if rec is not None:
        rec["logits"] = org.detach().cpu()
    if optimizer is not None:
        optimizer.zero_grad()
        loss.backward()
        if grads:
            rec["grads"] = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
        optimizer.step()


def _wants_grads(trace, training):
    """The first training step of a traced run records its gradients."""
    return trace is not None and training and not any(t.get("grads") is not None for t in trace)


def _finish_phase(logs, trace, n_trace0, phase):
    """The device logs of a phase -> (mean metrics, steps): the one copy to the host of the phase, and its rows into the trace."""
    log = torch.cat(logs).cpu() if logs else torch.zeros((0, 5), dtype=torch.float64)
    if trace is not None:
        for rec, row in zip(trace[n_trace0:], log.tolist()):
            rec.update(loss=row[0], tp=int(row[1]), tn=int(row[2]), fp=int(row[3]), fn=int(row[4]))
    step_metrics = metrics_from_log(log)
    if not step_metrics:
        raise ValueError(f"{phase}: no step with edges in this epoch")
    return average_epoch_metrics(step_metrics), len(step_metrics)


def _run_epoch_phase(run, graphs, training, epoch):
    """One pass over `graphs` on one device, whole graphs or clusters -> (mean metrics, steps, skipped clusters, 0.0: no plan time)."""
    hp, model, trace, phase = run.hp, run.model, run.trace, "train" if training else "valid"
    logs, skipped, first_grads = [], 0, _wants_grads(trace, training)
    n_trace0, n_done = len(trace) if trace is not None else 0, 0
    for gr in graphs:
        if training:
            model.train()
        steps, skip = _graph_steps(gr, hp, run.device, training, trace, phase, epoch)
        skipped += skip
        log = torch.zeros((len(steps), 5), dtype=torch.float64, device=run.device)
        for i, (views, ci) in enumerate(steps):
            org = _model_step(model, views, ci.x, ci.e).squeeze(-1)
            rev = _model_step(model, views.reversed(), ci.x_rev, ci.e).squeeze(-1) if hp["use_symmetry_loss"] else None
            _step(model, run.optimizer if training else None, org, rev, ci.y, run.pos_weight, run.alpha, log[i], ops.edge_loss,
                  rec=None if trace is None else trace[n_trace0 + n_done + i], grads=first_grads and n_done + i == 0)
        logs.append(log)
        n_done += len(steps)
    return (*_finish_phase(logs, trace, n_trace0, phase), skipped, 0.0)


def _rng_state(train_order):
    return {"python": random.getstate(), "numpy": np.random.get_state(), "torch": torch.get_rng_state(),
            "cuda": torch.cuda.get_rng_state_all() if torch.cuda.is_available() else [], "train_order": list(train_order)}


def _set_rng_state(st):
    random.setstate(st["python"])
    np.random.set_state(st["numpy"])
    torch.set_rng_state(st["torch"].cpu())
    if st.get("cuda"):
        torch.cuda.set_rng_state_all([t.cpu() for t in st["cuda"]])


# ---- the loop: train and train_partitioned are _set_up, _resume, their own restore of the random state, and _run_epochs -------------
# What differs between them is a phase function (_run_epoch_phase, _run_partitioned_phase) and a description of the ranks (_OneProcess,
# _RankGroup): who draws the order, who writes, whose random states the checkpoint holds, how the ranks agree on the times.

def _set_up(train_set, valid_set, out, hyperparameters, overfit, dropout, seed, device, models_dir, checkpoints_dir, trace, model_class,
            be=None):
    """Everything up to the first epoch that needs no other rank -> the run: hyperparameters, device, seed, datasets, pos_weight, model,
    optimizer, scheduler.  be: another backend than hip_backend(), which admits a CPU device.  The generators are seeded, then the model
    draws its parameters; nothing else draws."""
    hp = hyperparameters_with(hyperparameters)
    seed = hp["seed"] if seed is None else seed
    dropout = hp["dropout"] if dropout is None else dropout
    if device is not None:
        device = torch.device(device)
    else:
        device = torch.device("cuda", torch.cuda.current_device()) if be is None else torch.device("cpu")
    if be is None and device.type != "cuda":
        raise ValueError("the training step runs on the MI355X: device must be a HIP device")
    if device.type == "cuda":
        torch.cuda.set_device(device)
    be = be or hip_backend()
    set_seed(seed)
    if out is None:
        out = datetime.now().strftime("%Y-%b-%d-%H-%M-%S")
    ds_train = [_Graph(n, g, device, be) for n, g in load_dataset(train_set, hp, device)]
    ds_valid = ds_train if overfit else [_Graph(n, g, device, be) for n, g in load_dataset(valid_set, hp, device)]
    pos_weight = torch.tensor([pos_weight_of([(g.name, g.y) for g in ds_train])], device=device)
    model = model_class(hp["node_features"], hp["edge_features"], hp["dim_latent"], hp["hidden_ne_features"], hp["num_gnn_layers"],
                        hp["hidden_edge_scores"], hp["normalization"], dropout=dropout).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=hp["lr"])
    scheduler = ReduceLROnPlateau(optimizer, mode="min", factor=hp["decay"], patience=hp["patience"])
    if trace is not None:
        trace.append({"initial_state": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, "pos_weight": float(pos_weight)})
    return types.SimpleNamespace(hp=hp, seed=seed, out=out, overfit=overfit, device=device, be=be, ds_train=ds_train, ds_valid=ds_valid,
                                 pos_weight=pos_weight, alpha=float(hp["alpha"]) if hp["use_symmetry_loss"] else 0.0, model=model,
                                 optimizer=optimizer, scheduler=scheduler, trace=trace, models_dir=models_dir, checkpoints_dir=checkpoints_dir)


def _run_paths(out, seed, models_dir, checkpoints_dir, resumed=None):
    """(model file, checkpoint file) of the run `out` with `seed`; resumed=num_epochs: the files a resumed run writes."""
    out = f"{out}_seed{seed}" + ("" if resumed is None else f"_resumed-{resumed}")
    return os.path.join(models_dir, f"model_{out}.pt"), os.path.join(checkpoints_dir, f"ckpt_{out}.pt")


def _load_checkpoint(ckpt, model, optimizer, scheduler, loss_train, loss_valid):
    """Model, optimizer, scheduler and the best losses out of a checkpoint -> the epoch to start from (the random state is the caller's)."""
    model.load_state_dict(ckpt["model_state_dict"])
    optimizer.load_state_dict(ckpt["optim_state_dict"])
    loss_train.append(ckpt["loss_train"])
    loss_valid.append(ckpt["loss_valid"])
    if "scheduler_state_dict" in ckpt:
        scheduler.load_state_dict(ckpt["scheduler_state_dict"])
    return ckpt["epoch"] + 1


def _resume(run, resume):
    """The files the run writes, the epoch it starts from and the losses so far, onto `run` -> the checkpoint it resumes from (None: a
    fresh run), whose random state the caller restores."""
    run.model_path, run.ckpt_path = _run_paths(run.out, run.seed, run.models_dir, run.checkpoints_dir)
    run.start_epoch, run.loss_train, run.loss_valid = 0, [], []
    if not resume:
        return None
    ckpt = torch.load(run.ckpt_path, map_location="cpu", weights_only=False)   # load_state_dict moves to the device
    run.model_path, run.ckpt_path = _run_paths(run.out, run.seed, run.models_dir, run.checkpoints_dir, resumed=run.hp["num_epochs"])
    run.start_epoch = _load_checkpoint(ckpt, run.model, run.optimizer, run.scheduler, run.loss_train, run.loss_valid)
    return ckpt


class _OneProcess:
    """The ranks of `train`: one, which draws and writes and has nobody to agree with."""
    writes = True
    timed_fields = ("seconds",)

    def shuffled(self, order):
        random.shuffle(order)                                                          # train.py:294 shuffles the list in place
        return order

    def record_fields(self):
        return {}

    def checkpoint_rng(self, order):
        return {"rng_state": _rng_state(order)}

    def agreed(self, times):
        return times


def _run_epochs(run, ranks, phase, order):
    """The epochs from run.start_epoch on -> the records.  phase(run, graphs, training, epoch) -> (mean metrics, steps, skipped clusters,
    plan seconds); ranks: _OneProcess or _RankGroup; order: the order of the training graphs the last epoch left."""
    hp, model, optimizer, scheduler, loss_train, loss_valid = run.hp, run.model, run.optimizer, run.scheduler, run.loss_train, run.loss_valid
    log_path = os.path.splitext(run.ckpt_path)[0] + ".jsonl"
    if ranks.writes:
        os.makedirs(run.models_dir, exist_ok=True)
        os.makedirs(run.checkpoints_dir, exist_ok=True)
    records = []
    for epoch in range(run.start_epoch, hp["num_epochs"]):
        t0 = time.perf_counter()
        order = ranks.shuffled(order)
        train_mean, n_steps, n_skip, train_plan = phase(run, [run.ds_train[i] for i in order], True, epoch)
        loss_train.append(train_mean["loss"])
        lr = optimizer.param_groups[0]["lr"]
        rec = {"epoch": epoch, **{f"train/{k}": v for k, v in train_mean.items()}, "train/steps": n_steps, "train/skipped_clusters": n_skip}
        valid_plan = 0.0
        if not run.overfit:
            model.eval()
            with torch.no_grad():
                valid_mean, v_steps, v_skip, valid_plan = phase(run, run.ds_valid, False, epoch)
            loss_valid.append(valid_mean["loss"])
            rec.update({f"valid/{k}": v for k, v in valid_mean.items()})
            rec.update({"valid/steps": v_steps, "valid/skipped_clusters": v_skip})
        watched = loss_train if run.overfit else loss_valid
        saved = len(watched) == 1 or watched[-1] < min(watched[:-1])                   # the first epoch saves (the reference's min([]) raises)
        scheduler.step(watched[-1])
        best = (min(loss_train), 0.0 if run.overfit else min(loss_valid))
        if saved:
            rec["saved"] = True
        rec["lr"] = lr
        rec.update(ranks.record_fields())
        times = [time.perf_counter() - t0, train_plan, valid_plan]
        rng = ranks.checkpoint_rng(order)                                              # (every rank: among ranks it is a collective)
        if ranks.writes:
            if saved:
                torch.save(model.state_dict(), run.model_path)
            # after scheduler.step: the checkpoint's scheduler state is the one the next epoch starts from
            torch.save({"epoch": epoch, "model_state_dict": model.state_dict(), "optim_state_dict": optimizer.state_dict(),
                        "loss_train": best[0], "loss_valid": best[1], "scheduler_state_dict": scheduler.state_dict(), **rng}, run.ckpt_path)
        # the times are the writer's, and leave it after its writes: the barrier a later read (resume) depends on
        rec.update(zip(ranks.timed_fields, ranks.agreed(times)))
        if ranks.writes:
            with open(log_path, "a") as f:
                f.write(json.dumps(rec) + "\n")
        records.append(rec)
    ranks.agreed([0.0])                                                                # (the last .jsonl line is written)
    return records


def train(train_set, valid_set, out=None, hyperparameters=None, overfit=False, dropout=None, seed=None, resume=False, device=None,
          models_dir="models", checkpoints_dir="checkpoints", trace=None, model_class=SymGatedGCNModel):
    """train.py:188-450 (see the module docstring) -> the list of epoch records.  `hyperparameters`: overrides of
    configs/hyperparameters.py by the reference's key names.  `trace` (for tests): a list that receives the initial state dict and
    one dict per step (graph, mask fraction, the step's full-graph node and edge ids, its edges, its org logits, loss and counts; the
    first training step's gradients) - it copies to the host per step.  `model_class`: the model to train, SymGatedGCNModel, GatedGCNModel, GCNModel or
    SAGEModel (same constructor arguments).  A GatedGCNModel subclass that sets `training_step = "in_edge"` (and, if it wants the doubled
    graph, passes directed=False to the base constructor) trains through `_model_step` like any other model: its own call selects the
    one-direction step (engine_gated.train_forward_in_edge)."""
    run = _set_up(train_set, valid_set, out, hyperparameters, overfit, dropout, seed, device, models_dir, checkpoints_dir, trace, model_class)
    ckpt = _resume(run, resume)
    order = list(range(len(run.ds_train)))
    if ckpt is not None and "rng_state" in ckpt:
        _set_rng_state(ckpt["rng_state"])
        order = list(ckpt["rng_state"]["train_order"])
    return _run_epochs(run, _OneProcess(), _run_epoch_phase, order)


# ---- the loop on destination-range partitions --------------------------------------------------------------------------------

def _ranks_that_would_be_empty(src, dst, num_nodes, world, bounds, in_edges_only):
    """(bounds, owned nodes per rank, owned in-edges per rank) of the plan PartitionedGraph.from_global would build, from the edge list
    alone - no process group, the same on every rank (dist.partition_census's arithmetic)."""
    from . import dist as gdist
    src, dst = src.long(), dst.long()
    bounds = gdist.split_by_incident_edges(src, dst, num_nodes, world) if bounds is None else gdist._checked_bounds(bounds, num_nodes, world)
    bt = torch.tensor(bounds[1:-1], device=dst.device, dtype=torch.long)
    owned_in = torch.bincount(torch.bucketize(dst, bt, right=True), minlength=world).tolist()
    return bounds, [b - a for a, b in zip(bounds[:-1], bounds[1:])], owned_in


def _partition_bounds(ctx, gr, src, dst, num_nodes, epoch, phase):
    """The range boundaries of one (masked) graph's plan, or the collective refusal: decided from the edge list every rank holds, before the
    first collective of the plan, so every rank raises the same ValueError and none is left waiting for a peer."""
    bounds = None if ctx.bounds is None else ctx.bounds(src, dst, num_nodes, ctx.world)
    if ctx.doubled:   # the plan is cut over the doubled edge list: a rank's in-edges are the edges INCIDENT to its nodes, counted there
        from . import engine_gated
        plan_src, plan_dst = engine_gated.doubled_edge_list(src, dst)
    else:
        plan_src, plan_dst = src, dst
    bounds, nodes, in_edges = _ranks_that_would_be_empty(plan_src, plan_dst, num_nodes, ctx.world, bounds, ctx.in_edges_only)
    for r in range(ctx.world):
        if nodes[r] == 0 or in_edges[r] == 0:
            when = "before epoch 0" if epoch is None else f"{phase} phase of epoch {epoch}"
            raise ValueError(f"graph {gr.name}, {when}: rank {r} of world size {ctx.world} would own {nodes[r]} nodes and {in_edges[r]} "
                             f"in-edges of the {num_nodes} nodes and {int(src.numel())} edges left (bounds {bounds}): the graph is too "
                             "small for this world size")
    return bounds


def _partition_plan(ctx, src, dst, num_nodes, bounds):
    from . import dist as gdist
    return gdist.PartitionedGraph.from_global(src, dst, num_nodes, ctx.rank, ctx.world, ctx.device, ops=ctx.be.kernels, group=ctx.group,
                                              in_edges_only=ctx.in_edges_only, bounds=bounds, doubled=ctx.doubled)


def _partition_runner(ctx, model, part, ci):
    from . import dist as gdist
    if getattr(model, "kind", None) == "gat":
        return gdist.GATPartitionedRunner(model, part, ci.x, ci.e, ctx.device, ops=ctx.be.kernels, group=ctx.group)
    return gdist.PartitionedRunner(model, part, ci.x, ci.e, ctx.device, ops=ctx.be.kernels, group=ctx.group, x_rev_global=ci.x_rev)


def _synchronize(device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def _drawn_mask(ctx, gr, hp):
    """(fraction, keep bool[N // 2]) of one graph: rank 0 draws both exactly as _graph_steps does - random.randint, then torch.rand on the
    device - and broadcasts them in one message; no other rank draws."""
    from . import dist as gdist
    half = gr.num_nodes // 2
    if gr.num_nodes % 2:
        raise ValueError("nodes come in (read, reverse complement) pairs: N must be even")
    msg = torch.empty(1 + half, dtype=torch.uint8, device=ctx.device)
    if ctx.rank == 0:
        percent = random.randint(hp["mask_frac_low"], hp["mask_frac_high"])
        msg[0] = percent
        msg[1:] = torch.rand(half, device=ctx.device) < percent / 100               # train.py:92
    if not ctx.alone:
        gdist.broadcast_from(msg, 0, ctx.group)
    return int(msg[0]) / 100, msg[1:].bool()


def _run_partitioned_phase(ctx, run, graphs, training, epoch):
    """_run_epoch_phase in the whole-graph regime, every graph as one step on its destination-range partition -> (mean metrics, steps,
    0 skipped clusters, seconds spent on plans and runners)."""
    hp, model, trace, phase = run.hp, run.model, run.trace, "train" if training else "valid"
    device, be, sym = ctx.device, ctx.be, bool(hp["use_symmetry_loss"])
    first_grads = _wants_grads(trace, training)
    n_trace0 = len(trace) if trace is not None else 0
    log = torch.zeros((len(graphs), 5), dtype=torch.float64, device=device)
    plan_seconds = 0.0
    for i, gr in enumerate(graphs):
        if training:
            model.train()
        fraction, nid, eid, src, dst, n = None, None, None, gr.src, gr.dst, gr.num_nodes
        if hp["masking"]:
            fraction, keep = _drawn_mask(ctx, gr, hp)
            src, dst, nid, eid = features.induced_edge_list(gr.src, gr.dst, keep.repeat_interleave(2))
            n = int(nid.numel())
        _synchronize(device)
        t0 = time.perf_counter()
        bounds = _partition_bounds(ctx, gr, src, dst, n, epoch, phase)
        plan_seconds += time.perf_counter() - t0
        whole = types.SimpleNamespace(nid=torch.arange(n, device=device), eid=torch.arange(int(src.numel()), device=device))
        ci = be.cluster_inputs([whole], gr.in_deg, gr.out_deg, gr.e, gr.y, outer_nid=nid, outer_eid=eid, need_rev=sym)[0]
        _synchronize(device)
        t0 = time.perf_counter()
        part = _partition_plan(ctx, src, dst, n, bounds)
        runner = _partition_runner(ctx, model, part, ci)
        _synchronize(device)
        plan_seconds += time.perf_counter() - t0
        if trace is not None:
            trace.append({"phase": phase, "epoch": epoch, "graph": gr.name, "fraction": fraction, "whole": True,
                          "nid": (whole.nid if nid is None else nid).cpu(), "eid": (whole.eid if eid is None else eid).cpu(),
                          "src": src.cpu(), "dst": dst.cpu(), "num_nodes": n, "rank": ctx.rank, "n_own": part.n_own, "n_score": part.n_score})
        forward = runner.train_forward if training else runner.forward
        org = forward().squeeze(-1)
        rev = forward(reverse=True).squeeze(-1) if sym else None
        _step(model, run.optimizer if training else None, org, rev, ci.y, run.pos_weight, run.alpha, log[i], be.edge_loss,
              rec=None if trace is None else trace[-1], grads=first_grads and i == 0)
    return (*_finish_phase([log], trace, n_trace0, phase), 0, plan_seconds)


class _RankGroup:
    """The ranks of `train_partitioned`: rank 0 draws and writes, the checkpoint holds every rank's random state, the times are rank 0's."""
    timed_fields = ("seconds", "train/plan_seconds", "valid/plan_seconds")

    def __init__(self, ctx, reseeded):
        self.ctx, self.writes, self.reseeded = ctx, ctx.rank == 0, reseeded

    def _from_rank_0(self, t):
        from . import dist as gdist
        if not self.ctx.alone:
            gdist.broadcast_from(t, 0, self.ctx.group)
        return t.tolist()

    def shuffled(self, order):
        drawn = torch.zeros(len(order), dtype=torch.int64, device=self.ctx.device)
        if self.writes:
            random.shuffle(order)                                                      # train.py:294
            drawn.copy_(torch.tensor(order, dtype=torch.int64))
        return self._from_rank_0(drawn)

    def record_fields(self):
        """`world`, and in the first record after a resume at another world size "rng": "reseeded"."""
        fields, self.reseeded = {"world": self.ctx.world, **({"rng": "reseeded"} if self.reseeded else {})}, False
        return fields

    def checkpoint_rng(self, order):
        import torch.distributed as tdist
        states = [_rng_state(order)]
        if not self.ctx.alone:
            states = [None] * self.ctx.world
            tdist.all_gather_object(states, _rng_state(order), group=self.ctx.group)
        return {"rng_state": states[0], "world": self.ctx.world, "rng_states": states}

    def agreed(self, times):
        return self._from_rank_0(torch.tensor(times, dtype=torch.float64, device=self.ctx.device))


def train_partitioned(train_set, valid_set, out=None, hyperparameters=None, overfit=False, dropout=None, seed=None, resume=False, device=None,
                      models_dir="models", checkpoints_dir="checkpoints", trace=None, model_class=SymGatedGCNModel, group=None, ops=None,
                      bounds=None):
    """`train` with every graph on its destination-range partition (gnnome_amd.dist): every rank of an initialised torch.distributed
    group calls it with the same arguments, every rank returns the same list of epoch records.  The whole-graph regime only
    (num_nodes_per_cluster >= N for every graph of the datasets); clusters stay on `train`.

    group: the process group (None: the default one).  ops: the backend namespace (hip_backend() by default; with another one a CPU device
    is accepted).  bounds: a function (src, dst, num_nodes, world) -> range boundaries [0, ..., N] for the plan of each (masked) graph,
    in place of dist.split_by_incident_edges.

    A GatedGCNModel subclass whose constructor sets directed=False (with training_step = "in_edge") trains on the doubled plan of each graph
    (PartitionedGraph.from_global(..., in_edges_only=True, doubled=True), full_graph.py:47-51); `bounds` still receives the original edges.

    Rank 0 draws every random decision of the loop - the shuffle of the training graphs, the mask fraction, the keep mask - in the order
    `train` draws them and broadcasts it, so one seed gives the graph order and the masks of the single-device loop.  The logits and the
    gradients (summed over ranks) are the same bits on every rank, so the optimizers, the schedulers and the records stay in step.  Only
    rank 0 writes files; the checkpoint also holds `world` and `rng_states`, the random state of every rank (each rank's own generators
    draw its dropout rows), and resumes at the same world size bit for bit; at another world size rank 0's state is restored, the others
    reseed from seed + rank and the first record says "rng": "reseeded".  A refusal is decided on every rank from data all of them hold,
    before the collectives of the graph concerned ("Training loop on partitions")."""
    import torch.distributed as tdist
    from . import dist as gdist
    from .models import GatedGCNModel
    if not tdist.is_initialized():
        raise RuntimeError("train_partitioned: every rank of an initialised torch.distributed process group calls it")
    rank, world = tdist.get_rank(group), tdist.get_world_size(group)
    run = _set_up(train_set, valid_set, out, hyperparameters, overfit, dropout, seed, device, models_dir, checkpoints_dir, trace, model_class,
                  be=ops)
    hp, model, device, be = run.hp, run.model, run.device, run.be
    if hp["use_symmetry_loss"] and not issubclass(model_class, SymGatedGCNModel):
        raise ValueError(f"use_symmetry_loss=True needs the reversed pass, which only SymGatedGCNModel has on a partition; "
                         f"{model_class.__name__} trains with use_symmetry_loss=False")
    for gr in run.ds_train + ([] if overfit else run.ds_valid):
        if hp["num_nodes_per_cluster"] < gr.num_nodes:
            raise ValueError(f"num_nodes_per_cluster={hp['num_nodes_per_cluster']} is smaller than the {gr.num_nodes} nodes of graph {gr.name}: "
                             "that is the cluster regime, which trainer.train serves; train_partitioned trains on whole graphs")
    ctx = types.SimpleNamespace(be=be, group=group, rank=rank, world=world, device=device, bounds=bounds, alone=gdist._alone(world),
                                in_edges_only=isinstance(model, GatedGCNModel),
                                doubled=isinstance(model, GatedGCNModel) and not model.directed)   # full_graph.py:47-51: the doubled plan
    # the runners' own refusals (a model they do not serve, a training step they do not run) surface here, on every rank, before epoch 0
    model.train()
    first = run.ds_train[0]
    part = _partition_plan(ctx, first.src, first.dst, first.num_nodes,
                           _partition_bounds(ctx, first, first.src, first.dst, first.num_nodes, None, "train"))
    whole = types.SimpleNamespace(nid=torch.arange(first.num_nodes, device=device), eid=torch.arange(first.num_edges, device=device))
    ci = be.cluster_inputs([whole], first.in_deg, first.out_deg, first.e, first.y, need_rev=bool(hp["use_symmetry_loss"]))[0]
    _partition_runner(ctx, model, part, ci).check_train_step()
    del part, ci, whole

    if rank > 0:
        set_seed(run.seed + rank)    # the model above is the same on every rank; from here on a rank's generators draw its own dropout rows
    ckpt = _resume(run, resume)
    order = list(range(len(run.ds_train)))
    reseeded = False
    if ckpt is not None:
        states = ckpt.get("rng_states") if "world" in ckpt else ([ckpt["rng_state"]] if "rng_state" in ckpt else None)   # no `world`: train's
        if states is not None:
            order = list(states[0]["train_order"])
            reseeded = len(states) != world
            if not reseeded or rank == 0:
                _set_rng_state(states[rank])
    records = _run_epochs(run, _RankGroup(ctx, reseeded), functools.partial(_run_partitioned_phase, ctx), order)
    if trace is not None:
        trace.append({"final_state": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}})
    return records


def main(argv=None):
    """train.py:498-509."""
    p = argparse.ArgumentParser(description="Train a SymGatedGCN model on a dataset of labelled graphs")
    p.add_argument("--train", type=str, required=True, help="directory of <idx>.pt training graphs (trainer.process)")
    p.add_argument("--valid", type=str, required=True, help="directory of <idx>.pt validation graphs")
    p.add_argument("--asm", type=str, default=None, help="assembler used (accepted for the reference's command line; not read)")
    p.add_argument("--name", type=str, default=None, help="name for the model")
    p.add_argument("--overfit", action="store_true", help="overfit on the training data")
    p.add_argument("--resume", action="store_true", help="resume from the checkpoint of the run with this name and seed")
    p.add_argument("--dropout", type=float, default=None, help="dropout rate for the model")
    p.add_argument("--seed", type=int, default=None, help="random seed")
    p.add_argument("--gpu", type=int, default=None, help="index of the GPU to train on")
    p.add_argument("--models-dir", type=str, default="models")
    p.add_argument("--checkpoints-dir", type=str, default="checkpoints")
    p.add_argument("--gpus", type=int, default=None, help="train on destination-range partitions over this many ranks (train_partitioned)")
    p.add_argument("--transport", choices=("nccl", "gloo"), default="nccl",
                   help="nccl: one rank per GPU over RCCL; gloo: host-staged collectives, the ranks share one GPU (plumbing mode)")
    a = p.parse_args(argv)
    if a.gpus is not None and not 1 <= a.gpus <= MAX_RANKS:
        p.error(f"--gpus {a.gpus}: between 1 and {MAX_RANKS} ranks")
    if "WORLD_SIZE" in os.environ and a.gpus is not None:        # under torch.distributed.run: join the group that was set up
        return _rank_main(int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), None, a, int(os.environ.get("LOCAL_RANK", os.environ["RANK"])))
    if a.gpus is not None and a.gpus > 1:
        return _launch_ranks(a)
    device = torch.device("cuda", a.gpu if a.gpu is not None else torch.cuda.current_device())
    for rec in train(a.train, a.valid, out=a.name, overfit=a.overfit, dropout=a.dropout, seed=a.seed, resume=a.resume, device=device,
                     models_dir=a.models_dir, checkpoints_dir=a.checkpoints_dir):
        print(json.dumps(rec))
    return 0


MAX_RANKS = 16


def _rank_main(rank, world, port, a, local_rank=None):
    """One rank of `--gpus N`: set the device, join the group, train_partitioned; rank 0 prints the records."""
    import torch.distributed as tdist
    if port is not None:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    local_rank = rank if local_rank is None else local_rank
    # gloo: host-staged collectives between ranks that share one device (--gpu, default 0); nccl: rank r on GPU r
    device = torch.device("cuda", (a.gpu if a.gpu is not None else 0) if a.transport == "gloo" else local_rank)
    torch.cuda.set_device(device)
    if a.transport == "nccl":
        tdist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    else:
        tdist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        records = train_partitioned(a.train, a.valid, out=a.name, overfit=a.overfit, dropout=a.dropout, seed=a.seed, resume=a.resume,
                                    device=device, models_dir=a.models_dir, checkpoints_dir=a.checkpoints_dir)
        if rank == 0:
            for rec in records:
                print(json.dumps(rec), flush=True)
    finally:
        tdist.destroy_process_group()
    return 0


def _launch_ranks(a):
    """`--gpus N` without a launcher: N fresh processes (spawn), started before this one touches the GPU; it only waits.  -> the first
    non-zero exit status; when one rank fails the others are terminated (they would wait for it in a collective)."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_main, args=(r, a.gpus, port, a)) for r in range(a.gpus)]
    for pr in procs:
        pr.start()
    status = 0
    try:
        while status == 0 and any(pr.exitcode is None for pr in procs):
            for pr in procs:
                pr.join(timeout=0.2)
                if pr.exitcode not in (None, 0):
                    status = pr.exitcode
                    break
    finally:
        for pr in procs:
            if pr.exitcode is None:
                pr.terminate()
        for pr in procs:
            pr.join()
    return status if status != 0 else next((pr.exitcode for pr in procs if pr.exitcode), 0)


if __name__ == "__main__":
    sys.exit(main())
