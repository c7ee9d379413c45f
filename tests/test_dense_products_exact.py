"""Every dense product of the library against the exact probes of tests/product_probes.py, bit for bit (torch.equal).

A probe's true result, and every partial sum of the plane products it is made of, is an fp32 value (checked on the CPU in
tests/test_product_probes.py), so a kernel that keeps the plane products its header names returns the fp64 statement exactly, and one that
loses, doubles, misroutes or mis-scales one of them does not: the mutation table in test_product_probes.py says which family catches
which plane product.  A route is probed with the families of ITS arithmetic (product_probes.EXACT_UNDER): bf16x6 routes with d24 and mm
(and d22, mix, which are exact there too), fp16x3 routes with d22 and mix - d24 and mm need 24 bits of an operand and are NOT exact
under fp16x3 by its header (two planes of 11 bits).  Which arithmetic a route has is read from the kernels' dispatch
(csrc/linear.hip linear_impl, node_project.hip gnnome_linear_planes_route, edge_gate_bf.hip launch_pl, edge_gate_pl256.hip launch_pl256,
train_gemm.hip wgrad_impl, edge_score.hip), never from a run.

Every check starts with the premise on the device - 1.0 * 1.0 at position 0 of a one-row product is exactly 1.0 - so that a failure
separates "the recipe is wrong" from "the kernel is wrong".  Every check prints, for the record, which of ALL four families came out
exact; only the route's own families are asserted.

The inference gate and the fused data gradient add the operand itself to the product (A W^T + A): they run the residual probes
(product_probes.probe(residual=True): mm, d22 and mix, which between them still catch every mutant; d24 has no room for the second addend).
The scorer's streaming kernel writes no z1, so its first product is read through the logits, one z1 column per call, with a one-hot W2 / W3.
"""
import numpy as np
import pytest
import torch

import product_probes as pp
from gnnome_amd import ops

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _premise(product, k, n, with_base, residual=False, m=1):
    """1.0 * 1.0 at position 0 is exactly 1.0 (2.0 where the route adds the operand itself)."""
    A, W = np.zeros((m, k), np.float32), np.zeros((n, k), np.float32)
    A[0, 0] = W[0, 0] = 1.0
    base = A if residual else np.zeros((m, n), np.float32) if with_base else None
    got = product(_t(A), _t(W), None, _t(base)).cpu()
    want = torch.zeros(m, n)
    want[0, 0] = 2.0 if residual else 1.0
    assert torch.equal(got, want), "the premise fails on the device: 1.0 * 1.0 is not 1.0 on this route"


def _exact(product, split, m, k, n, bias=True, base=False, kpos=None, positive=False, seed=0, premise=True, residual=False):
    """product(A, W, bias, base) -> A W^T + bias + base on the device, compared with the fp64 statement of every family of `split`.
    kpos: {direction: k position of the sparse side's non-zero}."""
    if premise:
        _premise(product, k, n, base, residual)
    mine, report, wrong = pp.families_for(split), [], []
    for family in (pp.RESIDUAL_FAMILIES if residual else pp.FAMILIES):
        for direction in pp.DIRECTIONS:
            p = pp.probe(family, direction, m, k, n, seed=seed, bias=bias, base=base, kpos=None if kpos is None else kpos[direction],
                         positive=positive, residual=residual)
            want = torch.from_numpy(p.statement())
            got = product(_t(p.A), _t(p.W), _t(p.bias), _t(p.base)).cpu()
            same = torch.equal(got, want)
            off = (got.double() - want.double()).abs() / torch.from_numpy(np.spacing(np.abs(p.statement()))).double()
            report.append(f"{family}/{direction}:{'exact' if same else f'{int((off > 0).sum())} off, worst {off.max().item():.3g} ulp'}")
            if family in mine and not same:
                wrong.append(report[-1])
    print(f"[{split} m={m} k={k} n={n}] " + "  ".join(report))
    assert not wrong, f"{split} route, [{m} x {k}] x [{n} x {k}]^T: {wrong}"


# ------------------------------------------------------------------------------------------------ ops.linear

def _linear(planes=False, accumulate=False, strided=False):
    def product(A, W, bias, base):
        kw = {"planes": ops.weight_planes(W)} if planes else {}
        if accumulate:
            return ops.linear(A, W, bias, out=base.clone(), accumulate=True)
        if strided:      # a column block of a wider table: the sentinel columns stay as they are
            wide = torch.full((A.shape[0], W.shape[0] + 128), 7.0, device=dev())
            out = ops.linear(A, W, bias, out=wide[:, 64:64 + W.shape[0]], **kw)
            assert (wide[:, :64] == 7.0).all() and (wide[:, 64 + W.shape[0]:] == 7.0).all()
            return out.contiguous()
        return ops.linear(A, W, bias, **kw)
    return product


# (id, tuning key 2, inside bf16x6_arithmetic, caller-kept planes, arithmetic, K, Nout) - the arithmetic as linear_impl / gnnome_linear_planes_route decide it
LINEAR_ROUTES = [
    ("streaming-k64", 0, False, False, "bf16x6", 64, 320),              # k_linear_bf2<64, 4, 3, 1>
    ("streaming-k128", 0, False, False, "bf16x6", 128, 128),            # k_linear_bf2<128>: Nout < 256 keeps bf16x6
    ("tile-k128-n96", 0, False, False, "bf16x6", 128, 96),              # k_linear<4>: Nout no multiple of 64
    ("tile-k256-n64", 0, False, False, "bf16x6", 256, 64),              # k_linear<2>
    ("planes-k128", 0, False, False, "fp16x3", 128, 640),               # gnnome_linear_planes_f32, planes made per call
    ("planes-k256", 0, False, False, "fp16x3", 256, 1280),
    ("planes-k256-2hs", 0, False, False, "fp16x3", 256, 128),
    ("planes-kept-k64", 0, False, True, "fp16x3", 64, 320),             # K = 64 only on the caller's planes
    ("planes-kept-k128", 0, False, True, "fp16x3", 128, 640),
    ("planes-kept-k128-2hs", 0, False, True, "fp16x3", 128, 128),
    ("planes-kept-k256", 0, False, True, "fp16x3", 256, 1280),
    ("bf16x6-switch-k64", 0, True, False, "bf16x6", 64, 320),
    ("bf16x6-switch-k128", 0, True, False, "bf16x6", 128, 640),         # edge_gate_bf.hip mode 4 without F16
    ("bf16x6-switch-k256", 0, True, False, "bf16x6", 256, 1280),        # edge_gate_pl256.hip mode 4 without F16
    ("variant1-k64", 1, False, False, "bf16x6", 64, 320), ("variant1-k128", 1, False, False, "bf16x6", 128, 640),
    ("variant1-k256", 1, False, False, "bf16x6", 256, 1280),            # the tile kernel (gemm_tile.h)
    ("variant2-k64", 2, False, False, "fp32", 64, 320), ("variant2-k128", 2, False, False, "fp32", 128, 640),   # exact fp32 MFMA
    ("variant3-k64", 3, False, False, "bf16x6", 64, 320), ("variant3-k128", 3, False, False, "bf16x6", 128, 640),
    ("variant4-k64", 4, False, False, "bf16x6", 64, 320), ("variant5-k128", 5, False, False, "bf16x6", 128, 640),
    ("variant6-k64", 6, False, False, "bf16x6", 64, 320), ("variant6-k128", 6, False, False, "bf16x6", 128, 640),   # A-stationary, forced at a small size
    ("variant7-k64", 7, False, False, "bf16x6", 64, 320), ("variant7-k128", 7, False, False, "bf16x6", 128, 640),
    ("variant8-k64", 8, False, False, "bf16x6", 64, 320), ("variant8-k128", 8, False, False, "bf16x6", 128, 640),
    ("variant9-k128", 9, False, False, "fp16x3", 128, 640),             # the default route by name
    ("variant10-k128", 10, False, False, "fp16x3", 128, 640),           # edge_gate_bf.hip mode 4, F16
    ("variant10-k256", 10, False, False, "fp16x3", 256, 1280),          # edge_tile_f16.hip mode 4
]


@pytest.mark.parametrize("name,variant,switch,kept,split,k,nout", LINEAR_ROUTES, ids=[r[0] for r in LINEAR_ROUTES])
def test_linear(name, variant, switch, kept, split, k, nout):
    try:
        ops.set_tuning(2, variant)
        for i, m in enumerate(pp.row_counts(k)):
            run = lambda: _exact(_linear(planes=kept, strided=(m == 129)), split, m, k, nout, bias=(m != 33), seed=m, premise=(i == 0))  # noqa: E731
            if switch:
                with ops.bf16x6_arithmetic():
                    run()
            else:
                run()
    finally:
        ops.set_tuning(2, 0)


# accumulate=True is gnnome_linear_acc_f32.  From 32768 rows the square products leave the streaming / tile kernels for the edge-tile kernels
# as residual GEMMs (edge_gate_bf.hip mode 2 at K = 64 / 128, edge_gate_pl256.hip mode 2 at K = 256: bf16x6, their F16 forms are forward-only);
# key 2 = 1 is the tile kernel they replaced.
@pytest.mark.parametrize("k", [64, 128, 256])
@pytest.mark.parametrize("variant", [0, 1])
def test_linear_accumulate(k, variant):
    try:
        ops.set_tuning(2, variant)
        for i, m in enumerate(pp.row_counts(k)):
            _exact(_linear(accumulate=True), "bf16x6", m, k, k, bias=False, base=True, seed=m, premise=(i == 0))
        _exact(_linear(accumulate=True), "bf16x6", 129, k, 5 * k, bias=True, base=True, seed=7, premise=False)
        # just past the row count of the edge-sized residual kernels (33 MB at K = 256); the dense A repeats values where its form has fewer than M K
        _exact(_linear(accumulate=True), "bf16x6", 32768 + 33, k, k, bias=False, base=True, seed=8, premise=False)
    finally:
        ops.set_tuning(2, 0)


# ------------------------------------------------------------------------------------------------ column blocks and weight gradients

def _linear_blocks(width, accumulate, scaled):
    def product(A, W, bias, base):
        blocks = [A[:, i:i + width].contiguous() for i in range(0, A.shape[1], width)]
        assert ops.can_use_blocks(blocks)
        out = base.clone() if accumulate else torch.empty((A.shape[0], W.shape[0]), device=dev())
        return ops.linear_blocks(blocks, W, out, accumulate=accumulate, amax=_amax_of(A) if scaled else None)
    return product


@pytest.mark.parametrize("width,nblocks,nout", [(64, 5, 64), (128, 5, 128), (256, 5, 256), (32, 3, 32)])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
def test_linear_blocks(width, nblocks, nout, accumulate, scaled):
    """k_linear_blocks (gemm_tile.h's tile_gemm_blocks): bf16x6; with max |A| known (amax=) gnnome_linear_blocks_scaled_f32: ONE fp16x3 launch on
    the blocks scaled by a power of two.  K = nblocks * width, so the non-zero walks through every block."""
    k = width * nblocks
    for i, m in enumerate((1, 33, 129, 2 * width + 1)):
        _exact(_linear_blocks(width, accumulate, scaled), "fp16x3" if scaled else "bf16x6", m, k, nout, bias=False, base=accumulate, seed=m,
               premise=(i == 0))


def _spread(rows, ka, kb):
    """The sparse side's non-zero of column i at row (i step + 5) mod rows, the step sized by THAT side's column count, so that either side's
    non-zeros reach from the first row chunk to the last."""
    def of(count):
        step = max(rows // count, 1) | 1
        return lambda i: (i * step + 5) % rows
    return {"a_sparse": of(ka), "w_sparse": of(kb)}


def _amax_of(A):
    return A.abs().max().reshape(1).view(torch.int32).clone()     # the bits of max |A|, as bn_bwd_dgrad(..., amax=) leaves them


def _wgrad(scaled=False, blocks=0):
    """A W^T as a weight gradient: the kernel is handed the transposes, [rows, Ka] and [rows, Kb], and reduces over the rows."""
    def product(A, W, bias, base):
        At, Bt = A.t().contiguous(), W.t().contiguous()
        amax = _amax_of(At) if scaled else None
        if blocks:
            width = At.shape[1] // blocks
            C, sums = ops.wgrad_blocks([At[:, i * width:(i + 1) * width].contiguous() for i in range(blocks)], Bt, amax=amax)
            want = At.double().sum(0)
            if bool(((At != 0).sum(0) <= 1).all()):     # the bias gradients: one non-zero per column of a sparse A is an exact sum
                assert torch.equal(sums.double(), want)
            else:   # a dense A: any order of fp32 additions of n terms is within (n - 1) 2^-24 sum |a| of the true sum
                assert ((sums.double() - want).abs() <= (At.shape[0] - 1) * 2.0 ** -24 * At.double().abs().sum(0)).all()
            return C
        return ops.wgrad(At, Bt, amax=amax)
    return product


# (rows, Ka, Kb): ragged row chunks, several 128 x 128 tiles, and - one shape, 16 MB an operand - the 256 x 256 tile kernel that takes over from 16384 rows
WGRAD_SHAPES = [(1, 64, 64), (33, 128, 128), (2 * 128 + 1, 128, 64), (4099, 640, 128), (3001, 256, 256), (16384 + 17, 256, 256)]


@pytest.mark.parametrize("rows,ka,kb", WGRAD_SHAPES)
@pytest.mark.parametrize("scaled", [False, True])
def test_wgrad(rows, ka, kb, scaled):
    """gnnome_wgrad_f32 is bf16x6 (k_wgrad_partial, k_wgrad256_partial); with max |A| known, gnnome_wgrad_scaled_f32 is fp16x3 on A scaled by a
    power of two (k_wgrad_partial_h; the 256 x 256 kernel's one-accumulator form).  The dot product runs over the rows: the sparse side's
    non-zero is spread over them, so it falls into every row chunk the kernel reduces over, and the other chunks' partial sums are zeros."""
    split = "fp16x3" if scaled else "bf16x6"
    _premise(_wgrad(scaled), rows, kb, False, m=ka)
    _exact(_wgrad(scaled), split, ka, rows, kb, bias=False, kpos=_spread(rows, ka, kb), seed=rows, premise=False)


@pytest.mark.parametrize("rows,width,nblocks,kb", [(777, 64, 5, 64), (3001, 128, 5, 128), (2065, 256, 5, 256)])
@pytest.mark.parametrize("scaled", [False, True])
def test_wgrad_blocks(rows, width, nblocks, kb, scaled):
    """The concatenation-free form; scaled (fp16x3) where the block width is a whole number of 128-column tiles, bf16x6 otherwise (wgrad_impl)."""
    split = "fp16x3" if scaled and width % 128 == 0 else "bf16x6"
    ka = width * nblocks
    _premise(_wgrad(scaled, blocks=nblocks), rows, kb, False, m=ka)
    _exact(_wgrad(scaled, blocks=nblocks), split, ka, rows, kb, bias=False, kpos=_spread(rows, ka, kb), seed=rows, premise=False)


# ------------------------------------------------------------------------------------------------ the gate's and the scorer's products

def _graph(m):
    n = 50
    g = torch.Generator().manual_seed(m)
    src, dst = torch.randint(0, n, (m,), generator=g).int(), torch.randint(0, n, (m,), generator=g).int()
    return n, ops.GraphViews(src.to(dev()), dst.to(dev()), n)


def _gate(entry):
    """xe = B1h[src] + B2h[dst] + e W3^T with B1h = B2h = 0: the product alone; e rows are per sorted position and so are xe's."""
    def product(A, W, bias, base):
        n, views = _graph(A.shape[0])
        zeros = torch.zeros(n, A.shape[1], device=dev())
        if entry == "raw":
            return ops.edge_gate_raw(A, zeros, zeros, views, W)
        if entry == "stats":
            return ops.edge_gate_raw_stats(A, zeros, zeros, views, W)[0]
        return ops.edge_gate_raw_moments(A, zeros, zeros, views, W)[0]
    return product


def _gate_arithmetic(entry, H, switch):
    """gnnome_edge_gate_raw_f32 is the tile kernel (gemm_tile.h: bf16x6) at H = 64 / 128 and the plane form's raw mode at H = 256; the statistics
    entries are launch_bf at H = 64 (bf16x6 only), launch_pl at H = 128 and edge_tile_f16.hip at H = 256 (both fp16x3 unless the switch is on)."""
    if switch or H == 64 or (entry == "raw" and H == 128):
        return "bf16x6"
    return "fp16x3"


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("entry", ["raw", "stats", "moments"])
@pytest.mark.parametrize("switch", [False, True], ids=["default", "bf16x6_arithmetic"])
def test_gate_product(H, entry, switch):
    """The raw gate's e W3^T by default and inside ops.bf16x6_arithmetic().  (A first version of this test probed every default route as
    fp16x3; edge_gate.hip / edge_gate_bf.hip send H = 64, and edge_gate_raw at H = 128, to bf16x6 kernels, so those are probed as bf16x6.)"""
    def run():
        for i, m in enumerate(pp.row_counts(H)):
            _exact(_gate(entry), _gate_arithmetic(entry, H, switch), m, H, H, bias=False, seed=m, premise=(i == 0))
    if switch:
        with ops.bf16x6_arithmetic():
            run()
    else:
        run()


def _score_z1(hs):
    def product(A, W, bias, base):
        m = A.shape[0]
        n, views = _graph(m)
        zeros = torch.zeros(n, 2 * hs, device=dev())
        z1 = torch.full((m, hs), -1.0, device=dev())
        ops.edge_score(A, zeros[:, :hs], zeros[:, hs:], views, W, torch.zeros(32, hs, device=dev()), torch.zeros(32, device=dev()),
                       torch.zeros(32, device=dev()), torch.zeros(1, device=dev()), torch.zeros(m, device=dev()), z1_out=z1)
        return z1
    return product


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("hs", [32, 64])
def test_scorer_first_product(H, hs):
    """z1 = relu(Ps[src] + Qd[dst] + e W1e^T) with Ps = Qd = 0 and no negative operand: the product alone.  z1 is written by the tile kernel
    (gemm_tile.h, bf16x6) only; the streaming kernel is read through its logits in the next test."""
    for i, m in enumerate(pp.row_counts(H)):
        _exact(_score_z1(hs), "bf16x6", m, H, hs, bias=False, positive=True, seed=m, premise=(i == 0))


def _score_through_logits(hs):
    """The streaming kernel has no z1 output: column c of z1 is read as the logit with W2 = one 1.0 at [0, c], b2 = 0, W3 = (1, 0, ...), b3 = 0,
    one call per column.  relu(1.0 * z1[c]) * 1.0 stays the fp32 value z1[c] through either tail (exact fp32 MFMA, or fp16x3 on a z1 of
    at most 22 significant bits, which its two planes hold)."""
    W2 = torch.zeros(hs, 32, hs, device=dev())
    W2[torch.arange(hs), 0, torch.arange(hs)] = 1.0
    W3 = torch.zeros(32, device=dev())
    W3[0] = 1.0
    zeros32, zero1 = torch.zeros(32, device=dev()), torch.zeros(1, device=dev())

    def product(A, W, bias, base):
        m = A.shape[0]
        n, views = _graph(m)
        zeros = torch.zeros(n, 2 * hs, device=dev())
        out = torch.full((m, hs), -1.0, device=dev())
        for c in range(hs):
            out[:, c] = ops.edge_score(A, zeros[:, :hs], zeros[:, hs:], views, W, W2[c], zeros32, W3, zero1, torch.full((m,), -1.0, device=dev()),
                                       scatter_to_edge_id=False)
        return out
    return product


@pytest.mark.parametrize("H,switch", [(64, False), (128, False), (256, False), (64, True), (128, True)])
def test_scorer_first_product_on_the_streaming_kernel(H, switch):
    """k_edge_score_ws (inference, hs = 64, no z1 output): fp16x3 by default, bf16x6 inside ops.bf16x6_arithmetic() (H <= 128; H = 256 has the
    tile kernel there) - edge_score.hip's dispatch."""
    def run():
        for i, m in enumerate(pp.row_counts(H)):
            _exact(_score_through_logits(64), "bf16x6" if switch else "fp16x3", m, H, 64, bias=False, positive=True, seed=m, premise=(i == 0))
    if switch:
        with ops.bf16x6_arithmetic():
            run()
    else:
        run()


# ------------------------------------------------------------------------------------------------ product + operand: inference gate, fused data gradient

def _gate_inference(in_place):
    """e' = relu(scale (B1h[src] + B2h[dst] + e W3^T) + shift) + e with B = 0, scale = 1, shift = 0 and no negative operand: e W3^T + e."""
    def product(A, W, bias, base):
        n, views = _graph(A.shape[0])
        H = A.shape[1]
        zeros, one, zero = torch.zeros(n, H, device=dev()), torch.ones(H, device=dev()), torch.zeros(H, device=dev())
        if in_place:
            return ops.edge_gate(A.clone(), zeros, zeros, views, W, 0, one, zero)
        out = torch.full_like(A, -1.0)
        keep = A.clone()
        ops.edge_gate(A, zeros, zeros, views, W, 0, one, zero, out=out)
        assert torch.equal(A, keep)
        return out
    return product


def _gate_inference_arithmetic(H, in_place, switch, variant):
    """gnnome_edge_gate_f32's dispatch (edge_gate.hip): key 0 = 1 and H = 256 in place are the tile kernel (bf16x6), 5 / 6 the exact-fp32
    kernels, 8 and every H = 64 route launch_bf (bf16x6); the plane forms (H = 128: default and 7; H = 256 out of place) are fp16x3 unless the
    switch is on."""
    if variant in (5, 6):
        return "fp32"
    if switch or variant in (1, 8) or H == 64 or (H == 256 and in_place):
        return "bf16x6"
    return "fp16x3"


GATE_ROUTES = [(H, in_place, switch, 0) for H in (64, 128, 256) for in_place in (False, True) for switch in (False, True)] + \
              [(H, True, False, v) for H in (64, 128) for v in (1, 5, 6, 7, 8)] + [(256, True, False, 1)]


@pytest.mark.parametrize("H,in_place,switch,variant", GATE_ROUTES)
def test_inference_gate_product(H, in_place, switch, variant):
    try:
        ops.set_tuning(0, variant)

        def run():
            for i, m in enumerate(pp.row_counts(H)):
                _exact(_gate_inference(in_place), _gate_inference_arithmetic(H, in_place, switch, variant), m, H, H, bias=False, positive=True,
                       seed=m, premise=(i == 0), residual=True)
        if switch:
            with ops.bf16x6_arithmetic():
                run()
        else:
            run()
    finally:
        ops.set_tuning(0, 0)


def _dgrad(with_amax):
    """dxe = a (de [xe scale + shift > 0] - c1 - (xe - mean) rstd c2) and de += dxe Wt^T with xe = 1, scale = a = rstd = 1 and
    shift = c1 = c2 = mean = 0: dxe is de itself, bit for bit, and the updated de is de Wt^T + de."""
    def product(A, W, bias, base):
        H = A.shape[1]
        one, zero = torch.ones(H, device=dev()), torch.zeros(H, device=dev())
        de = A.clone()
        amax = torch.zeros(1, dtype=torch.int32, device=dev()) if with_amax else None
        dxe = ops.bn_bwd_dgrad(de, torch.ones_like(A), one, zero, one, zero, zero, zero, one, W, amax=amax)
        assert torch.equal(dxe, A), "dxe is not the probe operand"
        if with_amax:
            assert torch.equal(amax, _amax_of(A))
        return de
    return product


@pytest.mark.parametrize("H,with_amax,switch", [(64, False, False), (128, False, False), (128, True, False), (256, False, False), (256, True, False),
                                                (128, False, True), (256, False, True)])
def test_data_gradient_inside_bn_bwd_dgrad(H, with_amax, switch):
    """edge_gate_bf.hip mode 3 (H = 64 / 128: bf16x6, launch_pl's F16 forms are forward-only) and edge_gate_pl256.hip mode 3 (fp16x3 in one
    accumulator; bf16x6 inside ops.bf16x6_arithmetic()), with and without the max |dxe| slot.  Asserted on the updated de (`c`)."""
    def run():
        for i, m in enumerate(pp.row_counts(H)):
            _exact(_dgrad(with_amax), "fp16x3" if H == 256 and not switch else "bf16x6", m, H, H, bias=False, seed=m, premise=(i == 0), residual=True)
    if switch:
        with ops.bf16x6_arithmetic():
            run()
    else:
        run()
