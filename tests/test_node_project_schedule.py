"""k_node_project<128> (csrc/node_project.hip): the default schedule against the schedule before it (gnnome_set_tuning key 12 = 1).

A schedule decides when and how a workgroup's loads and stores are issued (the default: P through nontemporal stores), never what a
(row tile, column granule) unit computes: the two must agree bit for bit at every shape, and both stay at
tests/test_node_project.py's bar against an fp64 product (1e-5 of the scale 4).  Shapes: one lane, one wave short of / at / past its 32 rows,
one tile short of / at / past its 128 rows (M = 1 and M = 129: the lanes past M store the clamped row's bits again), three tiles, and
65 537 rows = 513 tiles - more than one round of the 512 resident workgroups, with a last tile of one row; one granule group (128 columns)
and five (640); dense and strided inputs and outputs (the forward writes column blocks of a wider P).
"""
import pytest
import torch

from gnnome_amd import ops

pytestmark = pytest.mark.gpu

K = 128
ROWS = (1, 31, 32, 33, 127, 128, 129, 257, 65_537)
COLS = (128, 640)


def dev():
    return torch.device("cuda", 0)


class _Schedule:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        ops.set_tuning(12, self.value)

    def __exit__(self, *exc):
        ops.set_tuning(12, 0)


_INPUTS = {}


def _inputs(nout):
    """One set of operands per width, made once: rows [0, M) of A serve every M; W, bias, the planes and the fp64 product of all rows."""
    if nout not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + nout)
        A = torch.randn(max(ROWS), K + 64, generator=g).to(dev())      # the strided form reads columns 32 .. 32 + K of this
        W = (torch.randn(nout, K, generator=g) / K ** 0.5).to(dev())
        b = torch.randn(nout, generator=g).to(dev())
        want = A[:, 32:32 + K].double() @ W.double().t() + b.double()
        _INPUTS[nout] = (A, W, b, ops.weight_planes(W), want)
    return _INPUTS[nout]


def _run(A, W, b, planes, nout, wide_out):
    m = A.shape[0]
    if not wide_out:
        return ops.linear(A, W, b, planes=planes), None
    wide = torch.full((m, nout + 128), 7.0, device=dev())
    ops.linear(A, W, b, out=wide[:, 64:64 + nout], planes=planes)
    return wide[:, 64:64 + nout], wide


@pytest.mark.parametrize("nout", COLS)
@pytest.mark.parametrize("m", ROWS)
def test_schedules_agree_bit_for_bit(m, nout):
    Awide, W, b, planes, want = _inputs(nout)
    strided_in = Awide[:m, 32:32 + K]
    dense_in = strided_in.contiguous()
    for a in (dense_in, strided_in):
        for wide_out in (False, True):
            with _Schedule(1):
                before, _ = _run(a, W, b, planes, nout, wide_out)
            got, wide = _run(a, W, b, planes, nout, wide_out)
            assert torch.equal(got, before), (m, nout, a.stride(0), wide_out)
            for out in (got, before):
                err = (out.double() - want[:m]).abs().max().item()
                assert err <= 1e-5 * 4.0, f"max abs err {err:.3e}"
            if wide is not None:
                assert (wide[:, :64] == 7.0).all() and (wide[:, 64 + nout:] == 7.0).all()


@pytest.mark.parametrize("m", (129, 65_537))
def test_two_launches_in_a_row_without_a_host_sync(m):
    """Nothing a launch leaves behind (in LDS, in device memory) may reach the next one on the stream."""
    nout = 640
    Awide, W, b, planes, _ = _inputs(nout)
    a = Awide[:m, 32:32 + K]
    with _Schedule(1):
        before = ops.linear(a, W, b, planes=planes)
    torch.cuda.synchronize()
    first, second = torch.empty_like(before), torch.empty_like(before)
    ops.linear(a, W, b, out=first, planes=planes)
    ops.linear(a, W, b, out=second, planes=planes)
    torch.cuda.synchronize()
    assert torch.equal(first, before) and torch.equal(second, before)
