"""Train mode of GatedGCNModel with `training_step = "in_edge"`: the one-direction step (engine_gated.train_forward_in_edge, on
csrc/node_aggregate_in_bwd.hip) against torch autograd over the plain-torch restatement on the CPU - both `directed` values, both norms,
a reversed graph, the three widths - against the adapter route, under dropout, and through one epoch of trainer.train.
The bars are test_gated_training.py's: probabilities within 1e-4, loss within 1e-5, _check_grads(rtol=1e-3)."""
import os

import pytest
import torch
import torch.nn.functional as F

from gnnome_amd import trainer
from gnnome_amd.graph import views_for
from gnnome_amd.models import GatedGCNModel

import gated_graphs as gg
from test_hip_training import _check_grads          # the symmetric step's own gradient check and tolerances

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def _cpu_step(sd, names, src, dst, n, x, e, nl, y, pw, directed):
    """The restatement differentiated by torch on the CPU -> (logits, loss, {parameter name: gradient})."""
    leaves = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    logits = gg.gated_model(leaves, src, dst, n, x, e, nl, directed=directed, training=True)
    loss = F.binary_cross_entropy_with_logits(logits.squeeze(-1), y, pos_weight=pw)
    loss.backward()
    return logits.detach(), loss.item(), {k: leaves[k].grad for k in names}


def _gpu_step(m, graph, x, e, y, pw):
    logits = m(graph, x.to(dev()), e.to(dev()))
    loss = F.binary_cross_entropy_with_logits(logits.squeeze(-1), y.to(dev()), pos_weight=pw.to(dev()))
    loss.backward()
    return logits.detach().cpu(), loss.item(), {k: p.grad for k, p in m.named_parameters()}


def _problem(n, e_cnt, hidden, nl, norm, directed, seed=21, dropout=0.0):
    src, dst, x, e = gg.model_graph(n, e_cnt, seed=seed)
    y = (torch.rand(e_cnt, generator=torch.Generator().manual_seed(2)) < 0.6).float()
    m = GatedGCNModel(2, 2, hidden, 16, nl, 64, norm, dropout=dropout, directed=directed)
    sd = gg.random_gated_state_dict(m, seed=8)
    m.load_state_dict(sd)
    m.training_step = "in_edge"
    return src, dst, x, e, y, torch.tensor([1.5]), m, sd


def _compare(got, want, label):
    (logits, loss, grads), (want_logits, want_loss, want_grads) = got, want
    dp = (torch.sigmoid(logits) - torch.sigmoid(want_logits)).abs().max().item()
    print(f"{label}: max |dp| {dp:.3e}, loss {loss:.6f} against {want_loss:.6f}")
    assert dp < 1e-4
    assert abs(loss - want_loss) < 1e-5
    assert set(grads) == set(want_grads)
    _check_grads(grads, want_grads, rtol=1e-3)


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("norm", ("batch", "layer"))
def test_one_bce_step_matches_torch_autograd(norm, directed):
    n, e_cnt, hidden, nl = 60, 300, 64, 2
    src, dst, x, e, y, pw, m, sd = _problem(n, e_cnt, hidden, nl, norm, directed)
    names = [k for k, _ in m.named_parameters()]
    assert not any("A_3" in k for k in names)
    want = _cpu_step(sd, names, src, dst, n, x, e, nl, y, pw, directed)
    m.to(dev()).train()
    _compare(_gpu_step(m, (src, dst, n), x, e, y, pw), want, f"{norm} directed={directed}")
    if norm == "batch":          # bn_e is applied ONCE per layer (gated_gcn_full.py:207): one momentum update per step
        bufs = dict(m.named_buffers())
        assert bufs["gnn.convs.0.bn_e.num_batches_tracked"].item() == 4 and bufs["gnn.convs.0.bn_h.num_batches_tracked"].item() == 4
        with torch.no_grad():
            h0 = F.linear(torch.relu(F.linear(x, sd["node_encoder.linear1.weight"], sd["node_encoder.linear1.bias"])),
                          sd["node_encoder.linear2.weight"], sd["node_encoder.linear2.bias"])
            e0 = F.linear(torch.relu(F.linear(e, sd["edge_encoder.linear1.weight"], sd["edge_encoder.linear1.bias"])),
                          sd["edge_encoder.linear2.weight"], sd["edge_encoder.linear2.bias"])
            gs, gd = (src, dst) if directed else gg.doubled_edge_list(src, dst)          # directed=False: the mean runs over the 2E rows
            if not directed:
                e0 = torch.cat([e0, e0], 0)
            lin = lambda name, t: F.linear(t, sd[f"gnn.convs.0.{name}.weight"], sd[f"gnn.convs.0.{name}.bias"])  # noqa: E731
            xe = lin("B_1", h0)[gs.long()] + lin("B_2", h0)[gd.long()] + lin("B_3", e0)
            mean = 0.9 * sd["gnn.convs.0.bn_e.running_mean"] + 0.1 * xe.mean(0)
        assert torch.allclose(bufs["gnn.convs.0.bn_e.running_mean"].cpu(), mean, atol=1e-5, rtol=1e-4)


def test_the_in_edge_step_against_the_adapter_route():
    n, e_cnt, hidden, nl = 60, 300, 64, 2
    src, dst, x, e, y, pw, m, sd = _problem(n, e_cnt, hidden, nl, "batch", True)
    m.to(dev()).train()
    new = _gpu_step(m, (src, dst, n), x, e, y, pw)
    m.load_state_dict(sd)
    m.zero_grad(set_to_none=True)
    m.training_step = "symmetric"
    old = _gpu_step(m, (src, dst, n), x, e, y, pw)
    dp = (torch.sigmoid(new[0]) - torch.sigmoid(old[0])).abs().max().item()
    print(f"in_edge against symmetric: max |dp| {dp:.3e}, logits {'equal bit for bit' if torch.equal(new[0], old[0]) else 'differ'}")
    assert dp < 1e-4
    assert set(new[2]) == set(old[2])
    _check_grads(new[2], {k: v.detach().cpu() for k, v in old[2].items()}, rtol=1e-3)


@pytest.mark.parametrize("directed", (True, False))
def test_a_reversed_graph(directed):
    """Views of dgl.reverse(g) - the trainer's symmetry loss - against the restatement on the swapped edge list."""
    n, e_cnt, hidden, nl = 60, 300, 64, 2
    src, dst, x, e, y, pw, m, sd = _problem(n, e_cnt, hidden, nl, "batch", directed)
    names = [k for k, _ in m.named_parameters()]
    want = _cpu_step(sd, names, dst, src, n, x, e, nl, y, pw, directed)
    m.to(dev()).train()
    views = views_for((src, dst, n), dev())
    _compare(_gpu_step(m, views.reversed(), x, e, y, pw), want, f"reversed directed={directed}")


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("hidden", (128, 256))
def test_one_step_at_the_wider_widths(hidden, directed):
    n, e_cnt, nl = 40, 200, 1
    src, dst, x, e, y, pw, m, sd = _problem(n, e_cnt, hidden, nl, "batch", directed)
    names = [k for k, _ in m.named_parameters()]
    want = _cpu_step(sd, names, src, dst, n, x, e, nl, y, pw, directed)
    m.to(dev()).train()
    _compare(_gpu_step(m, (src, dst, n), x, e, y, pw), want, f"H={hidden} directed={directed}")


@pytest.mark.parametrize("directed", (True, False))
def test_dropout_steps_are_finite_and_reproducible_under_one_seed(directed):
    n, e_cnt, hidden, nl = 60, 300, 64, 2
    src, dst, x, e, y, pw, m, sd = _problem(n, e_cnt, hidden, nl, "batch", directed, dropout=0.5)
    m.to(dev()).train()
    runs = []
    for _ in range(2):
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        logits, _, grads = _gpu_step(m, (src, dst, n), x, e, y, pw)
        assert all(torch.isfinite(v).all() for v in grads.values()) and torch.isfinite(logits).all()
        runs.append((logits, {k: v.clone() for k, v in grads.items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


class _InEdgeUndirected(GatedGCNModel):
    training_step = "in_edge"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **dict(kwargs, directed=False))


def test_one_trainer_epoch_with_an_in_edge_subclass_saves_a_loadable_checkpoint(tmp_path):
    from test_trainer import SMALL, _g14          # the tiny dataset fixture of tests/test_trainer.py
    train_set, valid_set = [_g14("single")], [_g14("multi")]
    hp = dict(SMALL, num_epochs=1, num_gnn_layers=2)
    records = trainer.train(train_set, valid_set, out="gated_in", hyperparameters=hp, dropout=0.0, seed=4, models_dir=str(tmp_path / "m"),
                            checkpoints_dir=str(tmp_path / "c"), model_class=_InEdgeUndirected)
    assert len(records) == 1 and records[0]["train/steps"] > 0 and records[0]["train/loss"] == records[0]["train/loss"]
    ckpt = torch.load(os.path.join(str(tmp_path / "c"), "ckpt_gated_in_seed4.pt"), map_location="cpu", weights_only=False)
    m = GatedGCNModel(2, 2, 64, 16, 2, 64, "batch")
    m.load_state_dict(ckpt["model_state_dict"], strict=True)
    assert not any("A_3" in k for k in ckpt["model_state_dict"])
    saved = torch.load(os.path.join(str(tmp_path / "m"), "model_gated_in_seed4.pt"), map_location="cpu")
    m.load_state_dict(saved, strict=True)
    assert all(torch.isfinite(v).all() for v in saved.values() if v.is_floating_point())
