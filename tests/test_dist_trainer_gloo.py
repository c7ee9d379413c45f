"""trainer.train_partitioned on CPU ranks over gloo with the checker backend (tests/cpu_trainer_ops.py): the loop against a plain torch loop
on the oracle model, the masks rank 0 draws, the refusals every rank raises alike, the files only rank 0 writes, resume, and the two
baselines that train with BCE.  The step's bars are tests/test_dist_symmetry_gloo.py's; every spawn has a deadline."""
import json
import os

import pytest
import torch
import torch.nn.functional as F
from torch.optim.lr_scheduler import ReduceLROnPlateau

import cpu_trainer_ops
import trainer_partition_cases as tpc
from dist_trainer_worker import run_ranks
from gnnome_amd import engine_baselines, engine_gat, features, models, trainer
from oracle.symgated_oracle import OracleModel, symmetry_loss
from test_train_host import check_grads

TIMEOUT = 120
UNMASKED = dict(tpc.HP, masking=False)
MASKED = dict(tpc.HP, masking=True)


@pytest.fixture(scope="module")
def sets():
    return tpc.datasets()


def _case(sets, tmp_path, **kw):
    kwargs = dict(out="t", hyperparameters=UNMASKED, dropout=0.0, seed=3, models_dir=str(tmp_path / "m"), checkpoints_dir=str(tmp_path / "c"))
    kwargs.update(kw.pop("kwargs", {}))
    return dict(train_set=sets[0], valid_set=sets[1], kwargs=kwargs, **kw)


def _degrees(g):
    n = int(g["num_nodes"])
    return torch.bincount(g["dst"].long(), minlength=n).float(), torch.bincount(g["src"].long(), minlength=n).float()


def _same_tensors(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def _same_trace(a, b):
    """Two ranks' traces, bit for bit, but for what names the rank."""
    if len(a) != len(b):
        return False
    for s, t in zip(a, b):
        for k in set(s) | set(t):
            if k in ("rank", "n_own", "n_score"):
                continue
            u, v = s.get(k), t.get(k)
            same = _same_tensors(u, v) if isinstance(u, dict) else torch.equal(u, v) if torch.is_tensor(u) else u == v
            if not same:
                return False
    return True


def _oracle_loop(sets, trace, hp, dtype):
    """train.py:188-450 in the whole-graph regime without masks, in plain torch: the oracle model, Adam, ReduceLROnPlateau, the graph order
    of the traced run -> (loss and gradients of step 1, final parameters)."""
    hp = trainer.hyperparameters_with(hp)
    train_set, valid_set = sets
    by_name = {f"graph {i}": g for i, g in enumerate(train_set)}
    om = OracleModel(2, 2, hp["dim_latent"], 16, hp["num_gnn_layers"], hp["hidden_edge_scores"], "batch", dropout=0.0)
    om.load_state_dict(trace[0]["initial_state"])
    om = om.to(dtype)
    opt = torch.optim.Adam(om.parameters(), lr=hp["lr"])
    sched = ReduceLROnPlateau(opt, mode="min", factor=hp["decay"], patience=hp["patience"])
    pw = torch.tensor([trace[0]["pos_weight"]], dtype=dtype)
    first = None

    def losses(g):
        ind, outd = _degrees(g)
        nid = torch.arange(g["num_nodes"])
        x = features.partition_degree_features(ind, outd, nid).to(dtype)
        xr = features.partition_degree_features(ind, outd, nid, reverse=True).to(dtype)
        src, dst, e, y = g["src"].long(), g["dst"].long(), g["e"].to(dtype), g["y"].to(dtype)
        org = om((src, dst, g["num_nodes"]), x, e).squeeze(-1)
        rev = om((dst, src, g["num_nodes"]), xr, e).squeeze(-1)
        return symmetry_loss(org, rev, y, pw, hp["alpha"])

    for epoch in range(hp["num_epochs"]):
        om.train()
        for s in (t for t in trace[1:-1] if t["phase"] == "train" and t["epoch"] == epoch):
            loss = losses(by_name[s["graph"]])
            opt.zero_grad()
            loss.backward()
            if first is None:
                first = (loss.item(), {k: p.grad.detach().float().clone() for k, p in om.named_parameters()})
            opt.step()
        om.eval()
        with torch.no_grad():
            sched.step(sum(losses(g).item() for g in valid_set) / len(valid_set))
    return first, {k: p.detach().double() for k, p in om.named_parameters()}


def _rel_l2(a, b):
    num = sum(((a[k].double() - b[k].double()) ** 2).sum().item() for k in b) ** 0.5
    return num / sum((b[k].double() ** 2).sum().item() for k in b) ** 0.5


@pytest.mark.parametrize("world", [2, 3])
def test_two_epochs_against_the_oracle_loop(sets, tmp_path, world):
    """Step 1 with the bars of the symmetry step (loss 1e-5, every gradient rtol 1e-3); the end of the run in relative L2 of the parameters
    against 10 times the oracle loop's own fp32-to-fp64 difference.  Measured (world 2 / world 3): 2.3e-5 / 1.9e-5 to the oracle's fp32
    loop, whose difference to its fp64 self is 1.4e-5 - the bar is 1.4e-4."""
    outs = run_ranks(world, _case(sets, tmp_path, odd_bounds=(world == 3)), str(tmp_path), TIMEOUT)
    res = [o["results"][0] for o in outs]
    assert all("error" not in r for r in res)
    steps = [t for t in res[0]["trace"][1:-1] if t["phase"] == "train"]
    assert len(steps) == 4 and len({s["graph"] for s in steps}) == 2 and all(s["fraction"] is None for s in steps)
    if world == 3:   # the explicit boundaries cut reads in two
        plans = [r["trace"][1] for r in res]
        assert plans[0]["n_own"] % 2 == 1 and sum(p["n_own"] for p in plans) == plans[0]["num_nodes"]
    assert sum(r["trace"][1]["n_score"] for r in res) == steps[0]["src"].numel()
    (loss1, grads1), end32 = _oracle_loop(sets, res[0]["trace"], UNMASKED, torch.float32)
    _, end64 = _oracle_loop(sets, res[0]["trace"], UNMASKED, torch.float64)
    assert abs(steps[0]["loss"] - loss1) < 1e-5
    check_grads(steps[0]["grads"], grads1, rtol=1e-3)
    final = torch.load(tmp_path / "c" / "ckpt_t_seed3.pt", weights_only=False)["model_state_dict"]
    noise = _rel_l2(end32, end64)
    got = _rel_l2({k: final[k] for k in end32}, end32)
    print(f"world {world}: parameters after 2 epochs, relative L2 to the oracle loop {got:.3e}; the oracle's fp32 to fp64 {noise:.3e}, "
          f"bar {10 * noise:.3e}")
    assert got < 10 * noise
    for r in res[1:]:   # records, traces (the first step's gradients among them) and the final state dicts: the same bits on every rank
        assert r["records"] == res[0]["records"] and _same_trace(r["trace"], res[0]["trace"])
        assert _same_tensors(r["trace"][-1]["final_state"], res[0]["trace"][-1]["final_state"])
    assert _same_tensors(res[0]["trace"][-1]["final_state"], final)
    assert [rec["world"] for rec in res[0]["records"]] == [world, world]
    assert all(rec["train/plan_seconds"] > 0 and rec["valid/plan_seconds"] > 0 for rec in res[0]["records"])


def test_masks_are_rank_zeros_and_whole_reads(sets, tmp_path):
    hp = trainer.hyperparameters_with(MASKED)
    outs = run_ranks(2, _case(sets, tmp_path, kwargs=dict(hyperparameters=MASKED), peers_never_draw=True, odd_bounds=True), str(tmp_path), TIMEOUT)
    res = [o["results"][0] for o in outs]
    assert all("error" not in r for r in res), [r.get("error") for r in res]
    assert _same_trace(res[0]["trace"], res[1]["trace"]) and res[0]["records"] == res[1]["records"]
    steps = res[0]["trace"][1:-1]
    assert len(steps) == 6
    for s in steps:
        assert hp["mask_frac_low"] / 100 <= s["fraction"] <= hp["mask_frac_high"] / 100
        kept = torch.zeros(2 * (int(s["nid"].max()) // 2 + 1), dtype=torch.bool)
        kept[s["nid"]] = True
        assert torch.equal(kept[0::2], kept[1::2])                       # 2r is there if and only if 2r + 1 is
        assert s["num_nodes"] == s["nid"].numel() and s["eid"].numel() == s["src"].numel()
    by = {(s["phase"], s["epoch"], s["graph"]): s for s in steps}
    for (phase, epoch, graph), s in by.items():
        if epoch == 0:
            assert not torch.equal(s["nid"], by[(phase, 1, graph)]["nid"])   # two epochs, two masks
    assert any(s["num_nodes"] < g["num_nodes"] for s in steps for g in sets[0][:1])


def test_a_rank_without_nodes_or_in_edges_is_refused_on_every_rank(sets, tmp_path):
    tiny = tpc.tiny_graph()
    case = dict(train_set=[tiny], valid_set=[tiny], kwargs=dict(out="t", hyperparameters=UNMASKED, dropout=0.0, seed=1,
                                                                 models_dir=str(tmp_path / "m"), checkpoints_dir=str(tmp_path / "c")))
    outs = run_ranks(3, case, str(tmp_path / "tiny"), TIMEOUT)
    texts = [o["results"][0].get("error") for o in outs]
    assert texts[0] is not None and texts[0].startswith("ValueError") and texts == [texts[0]] * 3
    assert "graph 0" in texts[0] and "world size 3" in texts[0] and "before epoch 0" in texts[0]
    assert not os.path.exists(tmp_path / "m") and not os.path.exists(tmp_path / "c")
    # epoch 1: from rank 0's fourth draw on (three graphs per epoch) the mask keeps one read, which no plan can serve
    outs = run_ranks(2, _case(sets, tmp_path, kwargs=dict(hyperparameters=MASKED), empty_mask_from_draw=3), str(tmp_path / "mask"), TIMEOUT)
    texts = [o["results"][0].get("error") for o in outs]
    assert texts[0] is not None and texts[0].startswith("ValueError") and texts == [texts[0]] * 2
    assert "world size 2" in texts[0] and "epoch 1" in texts[0] and "graph " in texts[0]
    assert len([json.loads(x) for x in open(tmp_path / "c" / "ckpt_t_seed3.jsonl")]) == 1     # epoch 0 had finished


def test_up_front_refusals_come_before_epoch_zero_and_write_nothing(sets, tmp_path):
    calls = [dict(hyperparameters=dict(UNMASKED, num_nodes_per_cluster=100)),
             dict(model="GCNModel"),
             dict(model="GatedGCNModel", hyperparameters=dict(UNMASKED, use_symmetry_loss=False))]
    outs = run_ranks(2, _case(sets, tmp_path, calls=calls, go_on_after_error=True), str(tmp_path), TIMEOUT)
    for o in outs:
        errs = [r.get("error") for r in o["results"]]
        assert len(errs) == 3 and errs == [r.get("error") for r in outs[0]["results"]]
        assert errs[0].startswith("ValueError") and "num_nodes_per_cluster" in errs[0] and "graph 0" in errs[0]
        assert errs[1].startswith("ValueError") and "use_symmetry_loss" in errs[1]
        assert errs[2].startswith("NotImplementedError") and "in_edge" in errs[2]
        assert all(len(r["trace"]) <= 1 for r in o["results"])           # (the initial state at most: no step ran)
    assert not os.path.exists(tmp_path / "m") and not os.path.exists(tmp_path / "c")


def test_files_are_rank_zeros_and_resume_is_bit_identical(sets, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    dirs = lambda d: dict(models_dir=str(d / "m"), checkpoints_dir=str(d / "c"))  # noqa: E731
    one = dict(MASKED, num_epochs=1)
    calls = [dict(hyperparameters=MASKED, **dirs(a)), dict(hyperparameters=one, **dirs(b)), dict(hyperparameters=MASKED, resume=True, **dirs(b))]
    outs = run_ranks(2, _case(sets, tmp_path, kwargs=dict(dropout=0.2, seed=5), calls=calls, peers_never_write=True), str(tmp_path), TIMEOUT)
    full, first, second = outs[0]["results"]
    assert all("error" not in r for o in outs for r in o["results"])
    assert sorted(os.listdir(a / "m")) == ["model_t_seed5.pt"] and sorted(os.listdir(a / "c")) == ["ckpt_t_seed5.jsonl", "ckpt_t_seed5.pt"]
    assert len(open(a / "c" / "ckpt_t_seed5.jsonl").readlines()) == 2
    want = torch.load(a / "c" / "ckpt_t_seed5.pt", weights_only=False)
    assert set(want) == set(trainer.CHECKPOINT_KEYS) | {"world", "rng_states"} and want["world"] == 2 and len(want["rng_states"]) == 2
    assert [r["epoch"] for r in first["records"]] == [0] and [r["epoch"] for r in second["records"]] == [1]
    timed = ("seconds", "train/plan_seconds", "valid/plan_seconds")
    strip = lambda r: {k: v for k, v in r.items() if k not in timed}  # noqa: E731
    assert [strip(r) for r in first["records"] + second["records"]] == [strip(r) for r in full["records"]]
    got = torch.load(b / "c" / "ckpt_t_seed5_resumed-2.pt", weights_only=False)
    assert _same_tensors(got["model_state_dict"], want["model_state_dict"])
    assert "rng" not in second["records"][0]
    # the world-2 checkpoint of epoch 0 resumed by three ranks
    outs = run_ranks(3, _case(sets, tmp_path, kwargs=dict(dropout=0.2, seed=5, hyperparameters=MASKED, resume=True, **dirs(b))),
                     str(tmp_path / "w3"), TIMEOUT)
    recs = [o["results"][0].get("records") for o in outs]
    assert recs[0] is not None and recs[0] == recs[1] == recs[2]
    assert [r["epoch"] for r in recs[0]] == [1] and recs[0][0]["rng"] == "reseeded" and recs[0][0]["world"] == 3


def test_gcn_and_gat_train_one_epoch_with_bce(sets, tmp_path):
    """The first step's loss against the single-rank step sequences of engine_baselines / engine_gat on the checker backend (the statement
    tests/test_dist_baseline_gloo.py and tests/test_dist_gat_gloo.py hold the partitioned step to), with their bar: 1e-5."""
    hp = dict(UNMASKED, num_epochs=1, use_symmetry_loss=False)
    calls = [dict(model="GCNModel", hyperparameters=hp), dict(model="GATModel", hyperparameters=hp, out="gat")]
    outs = run_ranks(2, _case(sets, tmp_path, calls=calls), str(tmp_path), TIMEOUT)
    full = trainer.hyperparameters_with(hp)
    for i, (name, eng) in enumerate((("GCNModel", engine_baselines), ("GATModel", engine_gat))):
        a, b = outs[0]["results"][i], outs[1]["results"][i]
        assert "error" not in a and "error" not in b, (a.get("error"), b.get("error"))
        assert a["records"] == b["records"] and _same_trace(a["trace"], b["trace"])
        step = a["trace"][1]
        g = sets[0][int(step["graph"].split()[1])]
        m = getattr(models, name)(2, 2, full["dim_latent"], 16, full["num_gnn_layers"], full["hidden_edge_scores"], "batch", dropout=0.0)
        m.load_state_dict(a["trace"][0]["initial_state"])
        m.train()
        ci = cpu_trainer_ops.cluster_inputs([step_ns(g)], *_degrees(g), g["e"], g["y"], need_rev=False)[0]
        views = cpu_trainer_ops.KERNELS.GraphViews(g["src"], g["dst"], g["num_nodes"])
        logits, _ = eng._step_forward(cpu_trainer_ops.KERNELS, m, views, ci.x, ci.e, [None] * full["num_gnn_layers"])
        want = F.binary_cross_entropy_with_logits(logits.squeeze(-1), ci.y, pos_weight=torch.tensor([a["trace"][0]["pos_weight"]]))
        print(f"{name}: first-step loss {step['loss']:.7f}, single-rank statement {want.item():.7f}")
        assert torch.isfinite(want) and abs(step["loss"] - want.item()) < 1e-5
        assert all(torch.isfinite(torch.tensor(r["train/loss"])) for r in a["records"])


def step_ns(g):
    import types
    return types.SimpleNamespace(nid=torch.arange(g["num_nodes"]), eid=torch.arange(g["src"].numel()))
