"""The training step of GATModel (engine_gat.train_forward) against torch autograd over the plain-torch train-mode restatement on the CPU
(tests/gat_training_cases.py), at the project's bars for a training step (tests/test_baseline_training.py: probabilities 1e-4, loss 1e-5,
gradients test_hip_training._check_grads rtol 1e-3, every parameter with a gradient that is not identically zero), and one epoch of
trainer.train."""
import os

import pytest
import torch
import torch.nn.functional as F

from gnnome_amd import engine_baselines, engine_gat, ops, train, trainer
from gnnome_amd.models import GATModel

import baseline_graphs as bg
import gat_training_cases as cases
from baseline_training_cases import MaskFeed, seeded_masks
from test_hip_training import _check_grads          # the symmetric step's own gradient check

pytestmark = pytest.mark.gpu

PW = 1.5
DROPOUT = 0.25


def dev():
    return torch.device("cuda", 0)


def _bce(logits, y):
    return F.binary_cross_entropy_with_logits(logits.squeeze(-1), y, pos_weight=torch.tensor([PW], device=y.device))


def _case(hidden, hs, nl, n, e_cnt, directed, seed):
    src, dst, x, e = bg.model_graph(n, e_cnt, seed=seed)
    y = (torch.rand(e_cnt, generator=torch.Generator().manual_seed(seed + 1)) < 0.6).float()
    m = GATModel(2, 2, hidden, 16, nl, hs, "batch", dropout=DROPOUT, directed=directed)
    sd = bg.random_state_dict(m, seed=seed + 2)
    m.load_state_dict(sd)
    return m, sd, src, dst, x, e, y


def _autograd(sd, graphs, n, x, e, nl, directed, masks, loss_of):
    """torch autograd over the restatement -> (logits per graph, loss, {name: grad})."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    logits = [cases.gat_model_train(leaves, s, d, n, x, e, nl, directed=directed, masks=masks[i * nl:(i + 1) * nl])
              for i, (s, d) in enumerate(graphs)]
    loss = loss_of(*logits)
    loss.backward()
    return [t.detach() for t in logits], loss.item(), {k: leaves[k].grad for k in leaves}


def _compare(m, got_logits, got_loss, want_logits, want_loss, want, what):
    got = {k: p.grad for k, p in m.named_parameters()}
    for gl, wl in zip(got_logits, want_logits):
        assert gl.is_cuda and gl.shape == wl.shape
        diff = bg.prob_diff(gl, wl)
        print(f"{what}: max |dp| = {diff:.2e}")
        assert diff < 1e-4
    print(f"{what}: loss {got_loss:.6f} against {want_loss:.6f}")
    assert abs(got_loss - want_loss) < 1e-5
    assert set(got) == set(want)
    assert any(k.endswith("attn_l") for k in got) and any(k.endswith("fc.weight") for k in got) and any(".linears." in k for k in got)
    assert all(v is not None for v in got.values()), "a parameter is missing its gradient"
    assert all(v.abs().max().item() > 0 for k, v in got.items()), "a gradient is identically zero"
    _check_grads(got, want, rtol=1e-3)


def _one_step(hidden, hs, nl, n, e_cnt, directed, seed, monkeypatch):
    m, sd, src, dst, x, e, y = _case(hidden, hs, nl, n, e_cnt, directed, seed)
    masks = seeded_masks(n, hidden, DROPOUT, nl, seed=seed + 3)
    want_logits, want_loss, want = _autograd(sd, [(src, dst)], n, x, e, nl, directed, masks, lambda t: _bce(t, y))
    feed = MaskFeed(masks)
    monkeypatch.setattr(train, "dropout_mask", feed)
    m.to(dev()).train()
    logits = engine_gat.train_forward(m, (src, dst, n), x.to(dev()), e.to(dev()))
    assert logits.requires_grad and feed.calls == nl
    loss = _bce(logits, y.to(dev()))
    loss.backward()
    _compare(m, [logits], loss.item(), want_logits, want_loss, want, f"gat H={hidden} hs={hs} directed={directed}")
    return m


@pytest.mark.parametrize("directed", (True, False))
def test_one_bce_step_matches_torch_autograd(directed, monkeypatch):
    """H = 64, three layers: two ReLU gates are crossed, every layer's input loses a quarter of its elements through substituted masks."""
    m = _one_step(64, 64, 3, 60, 300, directed, 21, monkeypatch)
    # the model's own call keeps refusing train mode, as does engine_baselines' entry; an optimizer step leaves a model that scores
    src, dst, x, e = bg.model_graph(60, 300, seed=21)
    with pytest.raises(NotImplementedError, match="eval mode"):
        m((src, dst, 60), x.to(dev()), e.to(dev()))
    with pytest.raises(NotImplementedError, match="engine_gat.train_forward"):
        engine_baselines.train_forward(m, (src, dst, 60), x.to(dev()), e.to(dev()))
    torch.optim.Adam(m.parameters(), lr=1e-4).step()
    assert torch.isfinite(m.eval()((src, dst, 60), x.to(dev()), e.to(dev()))).all()


@pytest.mark.parametrize("hidden,hs,directed", ((128, 32, True), (128, 32, False), (256, 128, False), (256, 128, True)))
def test_one_bce_step_at_the_wider_widths(hidden, hs, directed, monkeypatch):
    _one_step(hidden, hs, 2, 40, 200, directed, hidden + hs, monkeypatch)


@pytest.mark.parametrize("directed", (True, False))
def test_the_same_step_as_bf16x6(directed, monkeypatch):
    with ops.bf16x6_arithmetic():
        _one_step(64, 64, 3, 60, 300, directed, 23, monkeypatch)


def test_two_steps_from_the_same_state_leave_equal_gradient_bits(monkeypatch):
    nl, n = 3, 60
    m, sd, src, dst, x, e, y = _case(64, 64, nl, n, 300, False, 5)
    masks = seeded_masks(n, 64, DROPOUT, nl, seed=6)
    m.to(dev()).train()
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    runs = []
    for _ in range(2):
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        monkeypatch.setattr(train, "dropout_mask", MaskFeed(masks))
        logits = engine_gat.train_forward(m, views, x.to(dev()), e.to(dev()))
        _bce(logits, y.to(dev())).backward()
        runs.append((logits.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


@pytest.mark.parametrize("directed", (True, False))
def test_reversed_views_and_the_symmetry_loss_sum(directed, monkeypatch):
    nl, n, hidden = 2, 60, 64
    m, sd, src, dst, x, e, y = _case(hidden, 64, nl, n, 300, directed, 31)
    x_rev = x.flip(1).contiguous()   # (trainer hands the reversed call other node features: in- and out-degree exchanged)
    m.to(dev()).train()
    views = ops.GraphViews(src.to(dev()), dst.to(dev()), n)
    xd, xrd, ed, yd = x.to(dev()), x_rev.to(dev()), e.to(dev()), y.to(dev())
    # views.reversed() alone: the model of the swapped edge list
    masks = seeded_masks(n, hidden, DROPOUT, nl, seed=32)
    want_logits, want_loss, want = _autograd(sd, [(dst, src)], n, x_rev, e, nl, directed, masks, lambda t: _bce(t, y))
    monkeypatch.setattr(train, "dropout_mask", MaskFeed(masks))
    rev = engine_gat.train_forward(m, views.reversed(), xrd, ed)
    loss = _bce(rev, yd)
    loss.backward()
    _compare(m, [rev], loss.item(), want_logits, want_loss, want, f"gat directed={directed} reversed")
    # both orientations in one graph, as trainer's symmetry loss sums them: two calls, one backward
    m.zero_grad(set_to_none=True)
    masks = seeded_masks(n, hidden, DROPOUT, 2 * nl, seed=33)
    sym = lambda a, b, t: _bce(a, t) + _bce(b, t) + 0.1 * ((a - b) ** 2).mean()  # noqa: E731
    want_logits, want_loss, want = _autograd(sd, [(src, dst), (dst, src)], n, x, e, nl, directed, masks, lambda a, b: sym(a, b, y))
    monkeypatch.setattr(train, "dropout_mask", MaskFeed(masks))
    org = engine_gat.train_forward(m, views, xd, ed)
    rev = engine_gat.train_forward(m, views.reversed(), xd, ed)
    loss = sym(org, rev, yd)
    loss.backward()
    _compare(m, [org, rev], loss.item(), want_logits, want_loss, want, f"gat directed={directed} both orientations")


def test_a_graph_without_edges_and_the_bipartite_six_edge_graph(monkeypatch):
    n, hidden, nl = 12, 64, 2
    g = torch.Generator().manual_seed(4)
    x, e = torch.rand(n, 2, generator=g), torch.randn(6, 2, generator=g)
    m = GATModel(2, 2, hidden, 16, nl, 64, "batch", dropout=DROPOUT)
    sd = bg.random_state_dict(m, seed=5)
    m.load_state_dict(sd)
    m.to(dev()).train()
    # every node sees its own loop alone: nothing to score, and the backward leaves zero (or no) gradients without a fault
    none = torch.zeros(0, dtype=torch.int32)
    monkeypatch.setattr(train, "dropout_mask", MaskFeed(seeded_masks(n, hidden, DROPOUT, nl, seed=6)))
    out = engine_gat.train_forward(m, (none, none, n), x.to(dev()), torch.zeros(0, 2, device=dev()))
    assert out.shape == (0, 1) and out.requires_grad
    out.sum().backward()
    assert all(p.grad is None or not p.grad.any() for p in m.parameters())
    # six edges from nodes 0..5 to nodes 6..11: sources have in-degree 0, targets one neighbour and themselves
    m.zero_grad(set_to_none=True)
    src, dst = torch.arange(0, 6, dtype=torch.int32), torch.arange(6, 12, dtype=torch.int32)
    y = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    masks = seeded_masks(n, hidden, DROPOUT, nl, seed=7)
    want_logits, want_loss, want = _autograd(sd, [(src, dst)], n, x, e, nl, True, masks, lambda t: _bce(t, y))
    monkeypatch.setattr(train, "dropout_mask", MaskFeed(masks))
    logits = engine_gat.train_forward(m, (src, dst, n), x.to(dev()), e.to(dev()))
    loss = _bce(logits, y.to(dev()))
    loss.backward()
    _compare(m, [logits], loss.item(), want_logits, want_loss, want, "gat bipartite")


def test_refusals_of_the_entry():
    src, dst, x, e = bg.model_graph(10, 30, seed=1)
    m = GATModel(2, 2, 64, 16, 1, 64, "batch").train()          # parameters on the CPU
    with pytest.raises(RuntimeError, match="compute device"):
        engine_gat.train_forward(m, (src, dst, 10), x.to(dev()), e.to(dev()))
    m.to(dev())
    with pytest.raises(ValueError, match="rows"):
        engine_gat.train_forward(m, (src, dst, 10), x[:5].to(dev()), e.to(dev()))
    logits = engine_gat.train_forward(m, (src, dst, 10), x.to(dev()), e.to(dev()))
    logits.sum().backward()
    with pytest.raises(RuntimeError, match="released"):
        logits.sum().backward()


def test_one_trainer_epoch_saves_a_loadable_checkpoint(tmp_path):
    from test_trainer import SMALL, _g14          # the tiny dataset fixture of tests/test_trainer.py
    train_set, valid_set = [_g14("single")], [_g14("multi")]
    hp = dict(SMALL, num_epochs=1, num_gnn_layers=2)
    records = trainer.train(train_set, valid_set, out="gat", hyperparameters=hp, dropout=0.1, seed=4, models_dir=str(tmp_path / "m"),
                            checkpoints_dir=str(tmp_path / "c"), model_class=GATModel)
    assert len(records) == 1 and records[0]["train/steps"] > 0
    assert records[0]["train/loss"] == records[0]["train/loss"] and abs(records[0]["train/loss"]) != float("inf")
    ckpt = torch.load(os.path.join(str(tmp_path / "c"), "ckpt_gat_seed4.pt"), map_location="cpu", weights_only=False)
    m = GATModel(2, 2, 64, 16, 2, 64, "batch")
    m.load_state_dict(ckpt["model_state_dict"], strict=True)
    assert all(torch.isfinite(v).all() for v in ckpt["model_state_dict"].values() if v.is_floating_point())
    g = train_set[0]
    m.to(dev()).eval()
    from gnnome_amd.features import degree_features
    views = ops.GraphViews(g["src"].to(dev()).int(), g["dst"].to(dev()).int(), g["num_nodes"])
    logits = m(views, degree_features(views), g["e"].to(dev()))
    assert logits.shape == (g["src"].numel(), 1) and torch.isfinite(logits).all()
