"""The pure parts of gnnome_amd.trainer (train.py:188-450): the whole-graph-or-clusters rule, the positive-class weight, the metric
formulas and their epoch average, the checkpoint keys, hyperparameter defaults and the dataset errors.  No GPU."""
import os

import pytest
import torch

from gnnome_amd import trainer


def test_whole_graph_or_clusters_rule():
    assert trainer.plan(1000, 1000) == (True, 1)
    assert trainer.plan(999, 1000) == (True, 1)
    assert trainer.plan(1001, 1000) == (False, 2)
    assert trainer.plan(5000, 1000) == (False, 6)      # N // npc + 1, as train.py:317
    assert trainer.plan(5999, 1000) == (False, 6)
    assert trainer.plan(40, 7) == (False, 6)


def test_pos_weight_is_one_over_the_mean_ratio():
    y1 = torch.tensor([1.0, 0.0, 0.0, 0.0])           # 1 / 3
    y2 = torch.tensor([0.6, 0.4, 1.0, 0.0])           # round: 1, 0, 1, 0 -> 2 / 2
    assert trainer.pos_weight_of([("a", y1), ("b", y2)]) == pytest.approx(1 / ((1 / 3 + 1) / 2))


def test_pos_weight_without_negatives_names_the_graph():
    with pytest.raises(ValueError, match="graph b"):
        trainer.pos_weight_of([("a", torch.tensor([1.0, 0.0])), ("b", torch.tensor([1.0, 0.9]))])
    with pytest.raises(ValueError, match="no positive"):
        trainer.pos_weight_of([("a", torch.tensor([0.0, 0.0]))])


def test_metric_formulas_on_hand_made_counts():
    m = trainer.compute_metrics(6, 10, 2, 4, 0.5)
    assert m["loss"] == 0.5
    assert m["fp_rate"] == pytest.approx(2 / 12) and m["fn_rate"] == pytest.approx(4 / 10)
    assert m["acc"] == pytest.approx(16 / 22)
    assert m["precision"] == pytest.approx(6 / 8) and m["recall"] == pytest.approx(6 / 10) and m["f1"] == pytest.approx(6 / (6 + 3))
    assert m["acc_inv"] == pytest.approx(16 / 22)
    assert m["precision_inv"] == pytest.approx(10 / 14) and m["recall_inv"] == pytest.approx(10 / 12)
    assert m["f1_inv"] == pytest.approx(10 / (10 + 3))
    assert tuple(m) == trainer.METRIC_KEYS


def test_metric_formulas_at_zero_division():
    m = trainer.compute_metrics(0, 5, 0, 0, 1.0)        # no positives predicted or present
    assert m["precision"] == 0 and m["recall"] == 0 and m["f1"] == 0 and m["fn_rate"] == 0.0 and m["fp_rate"] == 0.0
    assert m["acc"] == 1.0 and m["precision_inv"] == 1.0
    m = trainer.compute_metrics(3, 0, 0, 0, 1.0)        # no negatives
    assert m["fp_rate"] == 0.0 and m["precision_inv"] == 0 and m["recall_inv"] == 0 and m["f1_inv"] == 0


def test_epoch_average_and_the_log_rows():
    log = torch.tensor([[0.5, 6, 10, 2, 4], [1.5, 0, 5, 0, 0]], dtype=torch.float64)
    steps = trainer.metrics_from_log(log)
    assert steps[0] == trainer.compute_metrics(6, 10, 2, 4, 0.5) and steps[1] == trainer.compute_metrics(0, 5, 0, 0, 1.5)
    avg = trainer.average_epoch_metrics(steps)
    assert avg["loss"] == pytest.approx(1.0)
    assert avg["precision"] == pytest.approx((6 / 8 + 0) / 2)
    assert all(isinstance(v, float) for v in avg.values())
    assert trainer.average_epoch_metrics([]) == {}


def test_checkpoint_keys_hold_the_reference_five():
    assert set(trainer.CHECKPOINT_KEYS) == {"epoch", "model_state_dict", "optim_state_dict", "loss_train", "loss_valid",
                                            "scheduler_state_dict", "rng_state"}


def test_hyperparameter_defaults_and_overrides():
    hp = trainer.hyperparameters_with({"lr": 1e-3})
    assert hp["lr"] == 1e-3 and hp["num_nodes_per_cluster"] == 1000 and hp["alpha"] == 0.1 and hp["mask_frac_low"] == 80
    assert hp["use_symmetry_loss"] is True and hp["masking"] is True and hp["num_epochs"] == 5 and hp["decay"] == 0.95
    with pytest.raises(KeyError):
        trainer.hyperparameters_with({"learning_rate": 1})


def test_graph_without_labels_names_it():
    g = {"src": torch.tensor([0, 1]), "dst": torch.tensor([1, 0]), "num_nodes": 2, "y": None}
    with pytest.raises(ValueError, match="graph g7"):
        trainer._Graph("g7", g, torch.device("cpu"))
    del g["y"]
    with pytest.raises(ValueError, match="graph g8"):
        trainer._Graph("g8", g, torch.device("cpu"))


def test_dataset_directory_is_read_in_index_order(tmp_path):
    for idx in (10, 2, 1):
        torch.save({"num_nodes": idx}, os.path.join(tmp_path, f"{idx}.pt"))
    (tmp_path / "notes.txt").write_text("not a graph")
    got = trainer.load_dataset(str(tmp_path))
    assert [g["num_nodes"] for _, g in got] == [1, 2, 10]
    assert got[0][0].endswith("1.pt")
    assert [n for n, _ in trainer.load_dataset([{"a": 1}, {"b": 2}])] == ["graph 0", "graph 1"]
    os.makedirs(tmp_path / "empty")
    with pytest.raises(ValueError, match="no <idx>.pt graphs"):
        trainer.load_dataset(str(tmp_path / "empty"))
