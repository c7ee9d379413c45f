"""The statements the GATModel training tests rest on, without a GPU: the fp64 gradient of the attention sum
(gat_training_cases.attention_sum_bwd_f64) against torch autograd through gat_graphs.attention_sum_f64, the unfold of the folded
projection's gradient (engine_gat.unfold) against autograd through the unfolded el = (feat * attn_l).sum(-1), and the entry's refusals."""
import pytest
import torch

import gat_graphs as gg
import gat_training_cases as cases
from gnnome_amd import engine_gat
from gnnome_amd.models import GATModel, GCNModel


def _graph(kind):
    if kind == "random":
        src, dst, _, _ = gg.model_graph(23, 90, seed=3)          # parallel edges 5 -> 6, the self-loop 7 -> 7, a sink and a source
        return src, dst, 23
    # hand-made: a multi-edge 0 -> 1 (three times), an own loop 2 -> 2, node 4 without any edge, a two-cycle 1 <-> 3
    return torch.tensor([0, 0, 0, 2, 1, 3, 0], dtype=torch.int32), torch.tensor([1, 1, 1, 2, 3, 1, 3], dtype=torch.int32), 5


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("kind", ("random", "hand"))
@pytest.mark.parametrize("slope", (0.2, 0.0))
def test_the_fp64_statement_is_autograd_through_the_forward_statement(kind, both, slope):
    src, dst, n = _graph(kind)
    H = 8
    g = torch.Generator().manual_seed(11)
    feat, el, er = torch.randn(n, 3 * H, generator=g), torch.randn(n, 4, generator=g), torch.randn(n, 4, generator=g)
    G, bias = torch.randn(n, 3 * H, generator=g), torch.randn(3 * H, generator=g)
    leaves = [t.double().requires_grad_(True) for t in (feat, el, er)]
    out, _ = gg.attention_sum_f64(leaves[0], leaves[1], leaves[2], src, dst, n, slope, bias, both)
    (out * G.double()).sum().backward()
    (dfeat, dl, dr), bounds = cases.attention_sum_bwd_f64(G, feat, el, er, src, dst, n, slope, both, bias)
    for got, want, what in ((dfeat, leaves[0].grad, "dfeat"), (dl, leaves[1].grad[:, :3], "del"), (dr, leaves[2].grad[:, :3], "der")):
        scale = want.abs().max().item()
        assert scale > 0 and (got - want).abs().max().item() <= 1e-12 * scale, what
    assert not leaves[1].grad[:, 3].any() and not leaves[2].grad[:, 3].any()          # the pad column is not read
    assert all(b.shape == v.shape and (b >= 0).all() for b, v in zip(bounds, (dfeat, dl, dr)))
    if kind == "hand":                                                                 # node 4 sees its loop alone: a = 1, dx = 0
        assert torch.equal(dfeat[4], G[4].double()) and not dl[4].any() and not dr[4].any()


def test_the_unfold_is_autograd_through_the_unfolded_scores():
    H = 64
    m = GATModel(2, 2, H, 16, 1, 64, "batch")
    conv = m.gnn.convs[0]
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in (conv.fc.weight, conv.attn_l, conv.attn_r):
            p.copy_(torch.randn(p.shape, generator=g))
    h = torch.randn(17, H, generator=g).double()
    dP = torch.randn(17, 3 * H + 64, generator=g).double()
    dP[:, 3 * H + 3], dP[:, 3 * H + 7:] = 0.0, 0.0                                     # what the backward kernel leaves there
    fc, al, ar = (p.detach().double().requires_grad_(True) for p in (conv.fc.weight, conv.attn_l, conv.attn_r))
    feat = (h @ fc.t()).view(17, 3, H)
    el, er = (feat * al).sum(-1), (feat * ar).sum(-1)                                  # DGL's, not folded
    loss = (feat.reshape(17, 3 * H) * dP[:, :3 * H]).sum() + (el * dP[:, 3 * H:3 * H + 3]).sum() + (er * dP[:, 3 * H + 4:3 * H + 7]).sum()
    loss.backward()

    class Conv64:                                                                      # the same parameters in fp64
        pass
    c64 = Conv64()
    c64.fc, c64.attn_l, c64.attn_r = Conv64(), al.detach(), ar.detach()
    c64.fc.weight = fc.detach()
    got = engine_gat.unfold(c64, dP.t() @ h)                                           # dWp = dP^T h
    for name, want in (("fc.weight", fc.grad), ("attn_l", al.grad), ("attn_r", ar.grad)):
        assert got[name].shape == want.shape
        assert (got[name] - want).abs().max().item() <= 1e-12 * want.abs().max().item(), name
    # ... and the fold on the device equals the host fold of the eval path
    assert torch.equal(engine_gat.fold_on_device(conv), engine_gat.projection_weight(conv))


def test_the_entry_exists_and_refuses_what_it_does_not_serve():
    src, dst, x, e = gg.model_graph(10, 30, seed=1)
    with pytest.raises(TypeError, match="GATModel"):
        engine_gat.train_forward(GCNModel(2, 2, 64, 16, 1, 64, "batch").train(), (src, dst, 10), x, e)
    if torch.cuda.is_available():
        x, e = x.cuda(), e.cuda()
    with pytest.raises(RuntimeError):                                                  # parameters on the CPU
        engine_gat.train_forward(GATModel(2, 2, 64, 16, 1, 64, "batch").train(), (src, dst, 10), x, e)
