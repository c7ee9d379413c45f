"""engine_baselines._BaselineStep, the one autograd shell of the GCN / SAGE / GAT training steps, without a GPU: it takes its backend
from the WholeGraph / PartitionShard it is given, so a stub backend and a stub (draw, forward, backward) triple show what the shell
itself does - the masks drawn once, the range fallback and its reuse of the masks, the switches that drop the fallback, the zero
gradients of an edgeless graph, the refusal of a second backward, and what a shard changes.

The stub step is logits = p0 * e_raw[:, 0] + p1 on a graph of 3 nodes and 4 edges.  Inputs and loss weights are small integers, so the
analytic gradients d p0 = sum(w * e_raw[:, 0]), d p1 = sum(w) are exact in float32 in any order of summation."""
import contextlib
import types

import pytest
import torch

from gnnome_amd import dist as gdist
from gnnome_amd import engine_baselines as eb
from gnnome_amd.train import WholeGraph

E0 = torch.tensor([1.0, -2.0, 3.0, 5.0])      # e_raw[:, 0]
WEIGHT = torch.tensor([2.0, 1.0, -3.0, 4.0])  # loss = sum(WEIGHT * logits)
WANT = {"p0": torch.tensor([(WEIGHT * E0).sum().item()]), "p1": torch.tensor([WEIGHT.sum().item()])}   # 11, 4


class StubOps:
    """A backend that only records how often, and whether now, its bf16x6 context is entered.  It keeps no _TUNING."""

    def __init__(self):
        self.entered, self.depth = 0, 0

    @contextlib.contextmanager
    def bf16x6_arithmetic(self):
        self.entered += 1
        self.depth += 1
        try:
            yield
        finally:
            self.depth -= 1


class TwoParameters(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p0 = torch.nn.Parameter(torch.tensor([3.0]))
        self.p1 = torch.nn.Parameter(torch.tensor([-1.0]))


class StubStep:
    """The triple.  overflow: the forward leaves a non-finite entry unless it runs inside the backend's bf16x6 context."""

    def __init__(self, overflow=False):
        self.overflow, self.drawn, self.forwards, self.backwards = overflow, [], [], []
        self.triple = (self.draw, self.forward, self.backward)

    def draw(self, model, rows, x):
        self.drawn.append(rows)
        return [object()]

    def forward(self, ops, model, views, x, e_raw, masks):
        self.forwards.append((ops.depth > 0, masks))
        logits = model.p0.detach() * e_raw[:, 0] + model.p1.detach()
        if self.overflow and ops.depth == 0:
            logits[0] = float("inf")
        return logits, {}

    def backward(self, ops, model, views, x, e_raw, kept, dlogits):
        self.backwards.append(ops.depth > 0)
        dl = dlogits.reshape(-1)
        return {"p0": (dl * e_raw[:, 0]).sum().reshape(1), "p1": dl.sum().reshape(1)}


def run(sh, step, model=None, edges=4):
    model = TwoParameters() if model is None else model
    names, params = zip(*model.named_parameters())
    x, e_raw = torch.zeros(sh.n_local, 2), torch.stack([E0[:edges], torch.zeros(edges)], 1)
    out = eb._BaselineStep.apply(model, sh, x, e_raw, list(names), step.triple, *params)
    return model, out


def whole(ops, edges=4):
    return WholeGraph(types.SimpleNamespace(num_nodes=3, num_edges=edges), ops=ops)


def backward(out):
    (out.squeeze(1) * WEIGHT[:out.shape[0]]).sum().backward()


def test_finite_logits_one_draw_one_forward_no_bf16x6():
    ops, step = StubOps(), StubStep()
    model, out = run(whole(ops), step)
    assert torch.equal(out, (3.0 * E0 - 1.0).unsqueeze(1))
    backward(out)
    assert step.drawn == [3] and len(step.forwards) == 1 and step.backwards == [False]
    assert ops.entered == 0
    assert torch.equal(model.p0.grad, WANT["p0"]) and torch.equal(model.p1.grad, WANT["p1"])


def test_non_finite_logits_rerun_as_bf16x6_on_the_same_masks():
    ops, step = StubOps(), StubStep(overflow=True)
    model, out = run(whole(ops), step)
    assert step.drawn == [3]
    assert [inside for inside, _ in step.forwards] == [False, True]
    assert step.forwards[0][1] is step.forwards[1][1]          # the identical masks object
    assert torch.equal(out, (3.0 * E0 - 1.0).unsqueeze(1))     # the rerun's logits
    backward(out)
    assert step.backwards == [True] and ops.entered == 2 and ops.depth == 0
    assert torch.equal(model.p0.grad, WANT["p0"]) and torch.equal(model.p1.grad, WANT["p1"])


def test_range_check_off_neither_reads_the_flag_nor_reruns(monkeypatch):
    ops, step, model = StubOps(), StubStep(overflow=True), TwoParameters()
    model.range_check = False
    monkeypatch.setattr(eb, "_any_rank_not_finite", lambda *a: pytest.fail("the flag was read"))
    _, out = run(whole(ops), step, model)
    assert len(step.forwards) == 1 and ops.entered == 0
    assert not torch.isfinite(out).all()


def test_forced_bf16x6_has_no_finiteness_rerun(monkeypatch):
    ops, step = StubOps(), StubStep(overflow=True)
    ops._TUNING = {10: 1}
    monkeypatch.setattr(eb, "_any_rank_not_finite", lambda *a: pytest.fail("the flag was read"))
    run(whole(ops), step)
    assert len(step.forwards) == 1 and ops.entered == 0


def test_an_edgeless_graph_gives_zero_gradients_without_the_steps_backward():
    ops, step = StubOps(), StubStep()
    model, out = run(whole(ops, edges=0), step, edges=0)
    assert out.shape == (0, 1)
    backward(out)
    assert step.backwards == []
    for p in model.parameters():
        assert p.grad.shape == p.shape and torch.equal(p.grad, torch.zeros_like(p))


def test_a_second_backward_is_refused():
    _, out = run(whole(StubOps()), StubStep())
    out.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="released by its first backward"):
        out.sum().backward()


class FakeShard:
    """What the shell reads of a dist.PartitionShard that is not alone: fewer owned rows than local ones, gradients that cross ranks
    (here: doubled), a group for the any-rank decision."""
    alone, n_own, n_local, e_own = False, 2, 3, 4

    def __init__(self, ops):
        self.ops, self.views, self.group, self.summed = ops, types.SimpleNamespace(num_nodes=3, num_edges=4), object(), 0

    def sum_ranks(self, tensors):
        self.summed += 1
        return [2 * t for t in tensors]


def test_a_shard_draws_for_owned_rows_decides_with_every_rank_and_sums_the_gradients(monkeypatch):
    reduced = []

    def all_reduce_sum(t, group=None):   # one rank's all-reduce: the identity
        reduced.append((t.clone(), group))
        return t

    monkeypatch.setattr(gdist, "all_reduce_sum", all_reduce_sum)
    ops, step = StubOps(), StubStep()
    sh = FakeShard(ops)
    model, out = run(sh, step)
    assert step.drawn == [2]                                        # n_own, not n_local
    assert len(reduced) == 1 and reduced[0][1] is sh.group          # the finiteness flag went through the collective ...
    assert torch.equal(reduced[0][0], torch.zeros(1))               # ... as "no rank saw a non-finite entry"
    assert len(step.forwards) == 1 and ops.entered == 0
    backward(out)
    assert sh.summed == 1
    assert torch.equal(model.p0.grad, 2 * WANT["p0"]) and torch.equal(model.p1.grad, 2 * WANT["p1"])
