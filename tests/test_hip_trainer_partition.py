"""GPU tests of trainer.train_partitioned with the HIP kernels as compute (the host twin is tests/test_dist_trainer_gloo.py).  The test box
has ONE MI355X: world 2 is two processes sharing the device over gloo with host staging, world 1 runs over RCCL with
GNNOME_FORCE_COLLECTIVES=1, as in tests/test_hip_symmetry_partition.py, whose step bars these are.  Never run on two devices."""
import json
import os
import subprocess
import sys

import pytest
import torch

import trainer_partition_cases as tpc
from conftest import ROOT
from dist_trainer_worker import run_ranks
from gnnome_amd import trainer

pytestmark = pytest.mark.gpu

TIMEOUT = 240
# tests/test_dist_trainer_gloo.py::test_two_epochs_against_the_oracle_loop measures the oracle loop in fp32 against itself in fp64 over its 4
# training steps: 1.4e-5 in relative L2 of the parameters.  Per step that is 3.6e-6; a later step's loss is held
# to 10 times that, times the training steps taken so far, relative to the loss.
ORACLE_DRIFT_PER_STEP = 1.4e-5 / 4
TIMED = ("seconds", "train/plan_seconds", "valid/plan_seconds", "world")


def _kwargs(tmp_path, name, hp, **kw):
    return dict(out="t", hyperparameters=hp, dropout=0.0, seed=3, models_dir=str(tmp_path / name / "m"),
                checkpoints_dir=str(tmp_path / name / "c"), **kw)


def test_world_two_against_the_single_device_loop(tmp_path):
    """Masking on: the masks are trainer.train's, step 1 within the step's bars (loss 1e-5, probabilities 1e-4), the later losses within
    the oracle's own fp32 drift, the counts within the number of edges whose single-device probability is that close to 0.5."""
    train_set, valid_set = tpc.datasets()
    hp = dict(tpc.HP, masking=True)
    one = []
    trainer.train(train_set, valid_set, trace=one, **_kwargs(tmp_path, "one", hp))
    outs = run_ranks(2, dict(train_set=train_set, valid_set=valid_set, kwargs=_kwargs(tmp_path, "two", hp), device="cuda"),
                     str(tmp_path / "ranks"), TIMEOUT)
    res = [o["results"][0] for o in outs]
    assert all("error" not in r for r in res), [r.get("error") for r in res]
    assert res[0]["records"] == res[1]["records"]
    want, got = one[1:], res[0]["trace"][1:-1]
    assert len(want) == len(got) == 6
    done = 0
    for k, (w, g) in enumerate(zip(want, got)):
        assert (w["phase"], w["epoch"], w["graph"], w["fraction"]) == (g["phase"], g["epoch"], g["graph"], g["fraction"])
        assert torch.equal(w["nid"], g["nid"]) and torch.equal(w["eid"], g["eid"])           # rank 0 drew in train's order
        done += w["phase"] == "train"
        E = int(w["eid"].numel())
        prob = (torch.sigmoid(g["logits"]) - torch.sigmoid(w["logits"])).abs().max().item()
        bar = 1e-5 if k == 0 else 10 * ORACLE_DRIFT_PER_STEP * done * abs(w["loss"])
        near = int(((torch.sigmoid(w["logits"]) - 0.5).abs() < 1e-4).sum())
        print(f"step {k} ({w['phase']}, epoch {w['epoch']}): loss {g['loss']:.7f} vs {w['loss']:.7f}, difference {abs(g['loss'] - w['loss']):.3e}, "
              f"bar {bar:.3e}; probability difference {prob:.3e}; {near} of {E} edges within 1e-4 of 0.5")
        assert abs(g["loss"] - w["loss"]) <= bar
        if k == 0:
            assert prob < 1e-4
        assert g["tp"] + g["tn"] + g["fp"] + g["fn"] == E
        assert near < 0.01 * E
        for c in ("tp", "tn", "fp", "fn"):
            assert abs(g[c] - w[c]) <= near, (k, c, g[c], w[c])
    assert all(t["n_own"] > 0 and t["n_score"] > 0 for x in res for t in x["trace"][1:-1])
    share = [(r["train/plan_seconds"] + r["valid/plan_seconds"]) / r["seconds"] for r in res[0]["records"]]
    print(f"plan_seconds share of an epoch, masking on, world 2 on one device over gloo: {share}")


def test_world_one_over_rccl_equals_the_single_device_loop_bit_for_bit(tmp_path):
    """Masking off, dropout 0: records and final state dict of one rank that issues every collective over RCCL against trainer.train.
    One rank's rows are the whole graph's, so the step keeps the single-rank BatchNorm kernels and sends their moments and backward sums
    through the collectives (train._can_fuse_bn, PartitionShard.sync_moments): a one-rank collective is the identity."""
    train_set, valid_set = tpc.datasets()
    hp = dict(tpc.HP, masking=False)
    records = trainer.train(train_set, valid_set, **_kwargs(tmp_path, "one", hp))
    outs = run_ranks(1, dict(train_set=train_set, valid_set=valid_set, kwargs=_kwargs(tmp_path, "rccl", hp), device="cuda", transport="nccl",
                             force_collectives=True), str(tmp_path / "ranks"), TIMEOUT)
    res = outs[0]["results"][0]
    assert "error" not in res and outs[0]["backend"] == "nccl"
    strip = lambda r: {k: v for k, v in r.items() if k not in TIMED}  # noqa: E731
    want = torch.load(tmp_path / "one" / "c" / "ckpt_t_seed3.pt", map_location="cpu", weights_only=False)["model_state_dict"]
    got = torch.load(tmp_path / "rccl" / "c" / "ckpt_t_seed3.pt", map_location="cpu", weights_only=False)["model_state_dict"]
    for a, b in zip(res["records"], records):
        off = {k: (a[k], b[k]) for k in strip(b) if a.get(k) != b[k]}
        print(f"epoch {b['epoch']}: {len(off)} record fields differ; losses (forced collectives, single device): "
              f"{ {k: v for k, v in off.items() if k.endswith('loss')} }")
    fl = [k for k in want if want[k].is_floating_point()]
    num = sum(((got[k].double() - want[k].double()) ** 2).sum().item() for k in fl) ** 0.5
    print(f"final state dict: {sum(not torch.equal(got[k], want[k]) for k in want)} of {len(want)} tensors differ, relative L2 "
          f"{num / sum((want[k].double() ** 2).sum().item() for k in fl) ** 0.5:.3e}")
    assert [strip(r) for r in res["records"]] == [strip(r) for r in records]
    assert all(r["world"] == 1 for r in res["records"])
    assert set(want) == set(got)
    for k, v in want.items():
        assert torch.equal(got[k], v), k


def _cli(tmp_path, data, name):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "gnnome_amd.trainer", "--train", str(data), "--valid", str(data), "--name", name, "--seed", "4",
                           "--gpus", "2", "--transport", "gloo"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=TIMEOUT)


def test_command_line_with_two_ranks(tmp_path):
    train_set, _ = tpc.datasets()
    d = tmp_path / "ds"
    os.makedirs(d)
    for i, g in enumerate(train_set):
        torch.save(g, d / f"{i}.pt")
    r = _cli(tmp_path, d, "t")
    assert r.returncode == 0, r.stderr[-3000:]
    epochs = trainer.DEFAULT_HYPERPARAMETERS["num_epochs"]
    assert sorted(os.listdir(tmp_path / "models")) == ["model_t_seed4.pt"]
    lines = [json.loads(x) for x in open(tmp_path / "checkpoints" / "ckpt_t_seed4.jsonl")]
    assert [x["epoch"] for x in lines] == list(range(epochs)) and all(x["world"] == 2 for x in lines)
    assert [json.loads(x)["epoch"] for x in r.stdout.splitlines() if x.startswith("{")] == list(range(epochs))
    small = tmp_path / "small"
    os.makedirs(small)
    torch.save(tpc.two_node_graph(), small / "0.pt")
    r = _cli(tmp_path, small, "s")
    assert r.returncode != 0
    assert "ValueError" in r.stderr and "world size 2" in r.stderr and "too small for this world size" in r.stderr
    assert not os.path.exists(tmp_path / "models" / "model_s_seed4.pt")
