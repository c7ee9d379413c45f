"""gnnome_amd.trainer end to end on the MI355X (train.py:188-450): the loop's steps replayed on the CPU with the oracle model and
torch.optim.Adam, resume, the checkpoint against the reference's load_checkpoint, learning, and a dataset directory written by
trainer.process, through the command line."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from gnnome_amd import features, gfa, trainer
from gnnome_amd.models import SymGatedGCNModel
from gnnome_amd.synth import make_graph
from oracle.symgated_oracle import OracleModel
from oracle.symgated_oracle import edge_features as oracle_edge_features

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SMALL = {"num_nodes_per_cluster": 25}   # the reference lr (1e-4)


def _g14(name):
    g = gfa.read_gfa(os.path.join(GOLDEN, f"g14_{name}.gfa"), reads_path=os.path.join(GOLDEN, f"g14_{name}.fasta"), training=True,
                     labels="device")
    sim = g["overlap_similarity"] if g["overlap_similarity"] is not None else torch.ones(g["src"].numel())
    g["e"] = oracle_edge_features(g["overlap_length"].float(), sim.float())
    return g


@pytest.fixture(scope="module")
def datasets():
    syn = make_graph(400, 3200, seed=5)
    syn["y"][:4] = torch.tensor([1.0, 0.0, 1.0, 0.0])
    return [_g14("single"), syn], [_g14("multi")]


def _degrees(g):
    n = int(g["num_nodes"])
    src, dst = torch.as_tensor(g["src"]).long(), torch.as_tensor(g["dst"]).long()
    return torch.bincount(dst, minlength=n).float(), torch.bincount(src, minlength=n).float()


def _symmetry_loss(org, rev, labels, pos_weight, alpha):
    """train.py:103-109."""
    a = F.binary_cross_entropy_with_logits(org, labels, pos_weight=pos_weight, reduction="none")
    b = F.binary_cross_entropy_with_logits(rev, labels, pos_weight=pos_weight, reduction="none")
    return (a + b + alpha * torch.abs(org - rev)).mean()


def _compute_metrics(logits, labels, loss):
    """train.py:30-54 with utils/metrics.py:6-46, on the host."""
    pred = torch.round(torch.sigmoid(logits))
    TP = int(((pred == 1) & (labels == 1)).sum())
    TN = int(((pred == 0) & (labels == 0)).sum())
    FP = int(((pred == 1) & (labels == 0)).sum())
    FN = int(((pred == 0) & (labels == 1)).sum())
    return TP, TN, FP, FN


def _check_grads(got, want, rtol):
    """tests/test_hip_training.py's bar: every gradient tensor within rtol of its own scale, with the absolute floor of the
    BatchNorm-fed biases."""
    floor = 1e-6 * max(w.abs().max().item() for w in want.values())
    for k, w in want.items():
        err = (got[k] - w).abs().max().item()
        assert err <= rtol * w.abs().max().item() + floor, f"{k}: max abs err {err:.2e} vs max |grad| {w.abs().max().item():.2e}"


def test_two_epochs_replay_on_the_oracle(datasets, tmp_path):
    train_set, valid_set = datasets
    hp = dict(SMALL, num_epochs=2)
    trace = []
    records = trainer.train(train_set, valid_set, out="replay", hyperparameters=hp, dropout=0.0, seed=3,
                            models_dir=str(tmp_path / "m"), checkpoints_dir=str(tmp_path / "c"), trace=trace)
    assert len(records) == 2 and all(r["train/steps"] > 0 and r["valid/steps"] > 0 for r in records)
    head, steps = trace[0], [t for t in trace[1:] if t["phase"] == "train"]
    assert len(steps) == sum(r["train/steps"] for r in records)
    assert any(not s["whole"] for s in steps) and len({s["graph"] for s in steps}) == 2
    assert all(s["fraction"] is not None and 0.8 <= s["fraction"] <= 1.0 for s in steps)

    fulls = {}
    for name, g in trainer.load_dataset(train_set):
        fulls[name] = (*_degrees(g), torch.as_tensor(g["e"]).float(), torch.as_tensor(g["y"]).float())
    hp_all = trainer.hyperparameters_with(hp)
    om = OracleModel(2, 2, hp_all["dim_latent"], 16, hp_all["num_gnn_layers"], 64, "batch", dropout=0.0)
    om.load_state_dict(head["initial_state"])
    om.train()
    opt = torch.optim.Adam(om.parameters(), lr=hp_all["lr"])
    pw = torch.tensor([head["pos_weight"]])
    for i, s in enumerate(steps):
        in_deg, out_deg, e, y = fulls[s["graph"]]
        x = features.partition_degree_features(in_deg, out_deg, s["nid"])
        xr = features.partition_degree_features(in_deg, out_deg, s["nid"], reverse=True)
        es, ys, n = e[s["eid"]], y[s["eid"]], s["num_nodes"]
        src, dst = s["src"].long(), s["dst"].long()
        org = om((src, dst, n), x, es).squeeze(-1)
        rev = om((dst, src, n), xr, es).squeeze(-1)
        loss = _symmetry_loss(org, rev, ys, pw, hp_all["alpha"])
        opt.zero_grad()
        loss.backward()
        if i == 0:
            _check_grads(s["grads"], {k: p.grad for k, p in om.named_parameters()}, rtol=3e-2)
        opt.step()
        assert abs(s["loss"] - loss.item()) <= 1e-4 * abs(loss.item()), (i, s["loss"], loss.item())
        near = int((org.detach().abs() < 1e-2).sum())
        for got, want in zip((s["tp"], s["tn"], s["fp"], s["fn"]), _compute_metrics(org.detach(), ys, None)):
            assert abs(got - want) <= near + 1, (i, got, want)

    ckpt = torch.load(tmp_path / "c" / "ckpt_replay_seed3.pt", map_location="cpu", weights_only=False)
    bound = hp_all["lr"] * len(steps)
    for k, p in om.named_parameters():
        d = (ckpt["model_state_dict"][k].cpu() - p.detach()).abs()
        assert d.max().item() <= 2 * bound and d.mean().item() <= 0.05 * bound, (k, d.max().item(), d.mean().item())


def test_resume_is_bit_identical_to_the_uninterrupted_run(datasets, tmp_path):
    train_set, valid_set = datasets
    kw = dict(out="r", dropout=0.2, seed=5)
    a = tmp_path / "a"
    trainer.train(train_set, valid_set, hyperparameters=dict(SMALL, num_epochs=2), models_dir=str(a / "m"), checkpoints_dir=str(a / "c"), **kw)
    b = tmp_path / "b"
    first = trainer.train(train_set, valid_set, hyperparameters=dict(SMALL, num_epochs=1), models_dir=str(b / "m"), checkpoints_dir=str(b / "c"),
                          **kw)
    second = trainer.train(train_set, valid_set, hyperparameters=dict(SMALL, num_epochs=2), models_dir=str(b / "m"),
                           checkpoints_dir=str(b / "c"), resume=True, **kw)
    assert [r["epoch"] for r in first] == [0] and [r["epoch"] for r in second] == [1]
    want = torch.load(a / "c" / "ckpt_r_seed5.pt", map_location="cpu", weights_only=False)
    got = torch.load(b / "c" / "ckpt_r_seed5_resumed-2.pt", map_location="cpu", weights_only=False)
    assert os.path.isfile(b / "m" / "model_r_seed5.pt")
    for k, v in want["model_state_dict"].items():
        assert torch.equal(got["model_state_dict"][k], v), k
    lines = [json.loads(x) for x in open(a / "c" / "ckpt_r_seed5.jsonl")]
    assert [r["epoch"] for r in lines] == [0, 1] and lines[1]["train/loss"] == second[0]["train/loss"]


def test_checkpoint_loads_with_the_reference_load_checkpoint(datasets, tmp_path):
    train_set, valid_set = datasets
    trainer.train(train_set, valid_set, out="ck", hyperparameters=dict(SMALL, num_epochs=1), seed=1, models_dir=str(tmp_path / "m"),
                  checkpoints_dir=str(tmp_path / "c"))
    path = tmp_path / "c" / "ckpt_ck_seed1.pt"

    def load_checkpoint(ckpt_path, model, optimizer):   # train.py:72-81, the path made an argument
        checkpoint = torch.load(ckpt_path, weights_only=False)
        epoch = checkpoint['epoch']
        model.load_state_dict(checkpoint['model_state_dict'])
        optimizer.load_state_dict(checkpoint['optim_state_dict'])
        loss_train = checkpoint['loss_train']
        loss_valid = checkpoint['loss_valid']
        return epoch, model, optimizer, loss_train, loss_valid

    model = SymGatedGCNModel(2, 2, 64, 16, 8, 64, "batch", dropout=0.2).cuda()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-4)
    epoch, model, optimizer, lt, lv = load_checkpoint(path, model, optimizer)
    assert epoch == 0 and lt > 0 and lv > 0
    assert set(torch.load(path, weights_only=False)) == set(trainer.CHECKPOINT_KEYS)
    assert os.path.isfile(tmp_path / "m" / "model_ck_seed1.pt")


def test_training_loss_falls_in_overfit_mode(datasets, tmp_path):
    train_set, _ = datasets
    hp = {"num_epochs": 10, "masking": False, "num_nodes_per_cluster": 10_000, "lr": 1e-3}   # one whole-graph step per graph and epoch
    records = trainer.train(train_set[:1], None, out="of", hyperparameters=hp, overfit=True, dropout=0.0, seed=2,
                            models_dir=str(tmp_path / "m"), checkpoints_dir=str(tmp_path / "c"))
    losses = [r["train/loss"] for r in records]
    assert len(losses) == 10 and all(r["train/steps"] == 1 for r in records)
    assert losses[-1] < losses[0], losses
    assert records[0].get("saved") and "valid/loss" not in records[0]


def test_dataset_directory_from_process_and_the_command_line(tmp_path):
    d = tmp_path / "ds"
    g0 = trainer.process(os.path.join(GOLDEN, "g14_single.gfa"), os.path.join(GOLDEN, "g14_single.fasta"), str(d / "0.pt"))
    trainer.process(os.path.join(GOLDEN, "g14_multi.gfa"), os.path.join(GOLDEN, "g14_multi.fasta"), str(d / "1.pt"))
    loaded = trainer.load_dataset(str(d))
    assert [os.path.basename(n) for n, _ in loaded] == ["0.pt", "1.pt"]
    assert torch.equal(loaded[0][1]["y"], g0["y"]) and loaded[0][1]["in_deg"].numel() == g0["num_nodes"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "gnnome_amd.trainer", "--train", str(d), "--valid", str(d), "--name", "t", "--seed", "4"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert [x["epoch"] for x in lines] == [0, 1, 2, 3, 4]
    assert os.path.isfile(tmp_path / "models" / "model_t_seed4.pt") and os.path.isfile(tmp_path / "checkpoints" / "ckpt_t_seed4.pt")
