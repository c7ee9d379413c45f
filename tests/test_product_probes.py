"""The exact-probe recipe of tests/product_probes.py, checked on the CPU against the numpy emulators of the two splits.

PREMISE: every family, direction and shape, through the emulator of every arithmetic the family is declared exact under, in several
accumulation orders (k steps forward and reversed, bias / base first or last, the plane products in every order, the fp16x3 second
accumulator folded at the end or after every k step), equals the fp64 statement bit for bit.

DISCRIMINATION: the emulator with one kept plane product removed, or with the second accumulator's 2^-11 applied twice or not at all, must
differ from the statement on at least one family.  The table test_every_mutant_is_caught prints, and asserts row by row (K = 128, 129 rows,
256 columns, bias on; a family "catches" when at least one output element differs; the test also prints the share of elements that differ
and the smallest difference among them in last places of the statement).  That smallest difference is 2^23 for a lost leading product,
thousands for a wrong scale, 4 to 40 for d22 / mix - but exactly 1 last place for hm, mh, hl, lh under d24 and 2 for mm under mm: the
low planes ARE the last places.  A tolerance of even one last place would let those through; torch.equal does not:

    mutant                               caught by (family/direction)
    bf16x6 without xh.wh                 d24/a_sparse d24/w_sparse mm/a_sparse mm/w_sparse d22/a_sparse d22/w_sparse mix/a_sparse mix/w_sparse
    bf16x6 without xh.wm                 d24/a_sparse mm/a_sparse mm/w_sparse d22/a_sparse mix/a_sparse
    bf16x6 without xm.wh                 d24/w_sparse mm/a_sparse mm/w_sparse d22/w_sparse mix/w_sparse
    bf16x6 without xm.wm                 mm/a_sparse mm/w_sparse
    bf16x6 without xh.wl                 d24/a_sparse d22/a_sparse mix/a_sparse
    bf16x6 without xl.wh                 d24/w_sparse d22/w_sparse mix/w_sparse
    fp16x3 without x1.w1                 d22/a_sparse d22/w_sparse mix/a_sparse mix/w_sparse
    fp16x3 without x1.w2                 d22/a_sparse mix/a_sparse
    fp16x3 without x2.w1                 d22/w_sparse mix/w_sparse
    fp16x3 with 2^-11 applied twice      d22/a_sparse d22/w_sparse mix/a_sparse mix/w_sparse
    fp16x3 with 2^-11 not applied        d22/a_sparse d22/w_sparse mix/a_sparse mix/w_sparse

so a device result that equals the statement on d24 + mm (a bf16x6 route) or on d22 + mix (an fp16x3 route), in both directions, has every
kept plane product in it once and at its scale.  No real-valued (randn) family is used: the exact ones already catch every mutant.

The routes that add the operand itself to the product (inference gate, fused data gradient) run the residual probes, A W^T + A, whose
premise and mutation table (mm, d22, mix: every mutant caught) are test_premise_of_the_residual_restatement and
test_every_mutant_is_caught_by_the_residual_probes.
"""
import numpy as np
import pytest

import product_probes as pp

SHAPES = [(m, k) for k in (64, 128, 256) for m in pp.row_counts(k)]


def _orders(split, every_plane_order):
    if every_plane_order:
        return pp.all_plane_orders(split)
    if split == "bf16x6":
        return [{}, {"reverse": True}, {"order": tuple(reversed(pp.BF16X6_ORDER))}]
    return [{}, {"reverse": True}, {"fold": "step"}, {"order": ("21", "12"), "fold": "step", "reverse": True}]


def _check_premise(p, every_plane_order=False):
    want = p.statement()          # asserts that the fp64 statement is an fp32 value
    init = p.init()
    for split in ("bf16x6", "fp16x3"):
        if split not in pp.EXACT_UNDER[p.family]:
            continue
        for kw in _orders(split, every_plane_order):
            got = pp.EMULATOR[split](p.A, p.W, init=init, **kw)      # bias + base first: the accumulator starts from them
            assert np.array_equal(got, want), (p.family, p.direction, split, kw, "init")
            if init is not None:                                     # ... or last: added to the finished product
                got = (pp.EMULATOR[split](p.A, p.W, **kw) + init).astype(np.float32)
                assert np.array_equal(got, want), (p.family, p.direction, split, kw, "tail")


@pytest.mark.parametrize("m,k", SHAPES)
@pytest.mark.parametrize("direction", pp.DIRECTIONS)
@pytest.mark.parametrize("family", pp.FAMILIES)
def test_premise_every_family_direction_and_shape(family, direction, m, k):
    n = k + 64          # the sparse W walks every k position and wraps
    _check_premise(pp.probe(family, direction, m, k, n, seed=1, bias=True, base=False))
    _check_premise(pp.probe(family, direction, m, k, n, seed=2, bias=False, base=True))


@pytest.mark.parametrize("direction", pp.DIRECTIONS)
@pytest.mark.parametrize("family", pp.FAMILIES)
def test_premise_with_the_planes_in_every_order(family, direction):
    _check_premise(pp.probe(family, direction, 33, 64, 96, seed=3, bias=True, base=True), every_plane_order=True)


@pytest.mark.parametrize("direction", pp.DIRECTIONS)
@pytest.mark.parametrize("family", pp.FAMILIES)
def test_premise_of_the_weight_gradient_layout(family, direction):
    """A^T B: the dot product runs over the rows, the non-zero is spread over them (what the device tests hand to ops.wgrad)."""
    rows, ka, kb = 2064, 128, 64
    p = pp.probe(family, direction, ka, rows, kb, seed=4, bias=False, kpos=lambda i: (i * 97 + 5) % rows)
    assert np.unique(np.nonzero(p.A if direction == "a_sparse" else p.W)[1] // 256).size >= 8       # the non-zeros reach every 256-row chunk
    _check_premise(p)


@pytest.mark.parametrize("m,k", SHAPES)
@pytest.mark.parametrize("positive", [False, True])
def test_premise_of_the_residual_restatement(m, k, positive):
    """A W^T + A (square W): the inference gate relu(1 * (e W3^T) + 0) + e with no negative operand, and the fused data gradient
    de + dxe Wt^T with a = 1, c1 = c2 = 0 and an open relu mask, so that dxe = de.  d24 has no room for the second addend and is left out."""
    for family in pp.RESIDUAL_FAMILIES:
        for direction in pp.DIRECTIONS:
            p = pp.probe(family, direction, m, k, k, seed=7, bias=False, residual=True, positive=positive)
            assert np.array_equal(p.base, p.A)
            _check_premise(p)
    if m > 1:
        with pytest.raises(AssertionError):
            pp.probe("d24", "w_sparse", m, k, k, seed=7, bias=False, residual=True, positive=positive).statement()


def test_every_mutant_is_caught_by_the_residual_probes():
    probes = [pp.probe(f, d, 129, 128, 128, seed=8, bias=False, residual=True) for f in pp.RESIDUAL_FAMILIES for d in pp.DIRECTIONS]
    for name, (split, kw) in pp.mutants().items():
        caught = [f"{p.family}/{p.direction}" for p in probes if split in pp.EXACT_UNDER[p.family]
                  and not np.array_equal(pp.EMULATOR[split](p.A, p.W, init=p.init(), **kw), p.statement())]
        print(f"{name:36s} " + " ".join(caught))
        assert caught, name


def test_planes_are_normal_numbers_or_zero():
    """Whether the matrix cores flush 16-bit subnormals is not something the probes may depend on."""
    for family in pp.FAMILIES:
        for direction in pp.DIRECTIONS:
            p = pp.probe(family, direction, 129, 128, 256, seed=5)
            for x in (p.A, p.W):
                assert np.abs(x[x != 0]).min() >= 2.0 ** -2 and np.abs(x).max() <= 2.0 ** 9
                planes = [(pl, 2.0 ** -126) for pl in pp.split_bf16(x)]              # bf16 has fp32's exponent range
                if "fp16x3" in pp.EXACT_UNDER[family]:
                    planes += [(pl, 2.0 ** -14) for pl in pp.split_f16(x)]
                    assert np.array_equal(sum(pl.astype(np.float64) / s for pl, s in zip(pp.split_f16(x), (1.0, 2048.0))), x.astype(np.float64))
                for pl, smallest_normal in planes:
                    mag = np.abs(pl[pl != 0])
                    assert mag.size == 0 or (mag.min() >= smallest_normal and mag.max() <= 2.0 ** 10), (family, direction)
            sparse = p.A if direction == "a_sparse" else p.W
            assert ((sparse != 0).sum(1) == 1).all() and np.signbit(sparse[sparse == 0]).any() and not np.signbit(sparse[sparse == 0]).all()


def test_every_mutant_is_caught():
    m, k, n = 129, 128, 256
    probes = [pp.probe(f, d, m, k, n, seed=6) for f in pp.FAMILIES for d in pp.DIRECTIONS]
    table = {}
    for name, (split, kw) in pp.mutants().items():
        caught = []
        for p in probes:
            if split not in pp.EXACT_UNDER[p.family]:
                continue
            want = p.statement()
            assert np.array_equal(pp.EMULATOR[split](p.A, p.W, init=p.init()), want)      # the unmutated emulator on the same inputs
            got = pp.EMULATOR[split](p.A, p.W, init=p.init(), **kw)
            diff = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
            if (diff > 0).any():
                caught.append((f"{p.family}/{p.direction}", float((diff > 0).mean()), float(diff[diff > 0].min())))
        table[name] = caught
    print(f"\n{'mutant':36s} caught by family/direction (share of elements that differ, smallest difference in last places)")
    for name, caught in table.items():
        print(f"{name:36s} " + " ".join(f"{c[0]} ({c[1]:.2f}, {c[2]:.3g})" for c in caught))
    missed = [name for name, caught in table.items() if not caught]
    assert not missed, f"no family catches: {missed}"
    assert len(table) == 6 + 3 + 2
    # the families the device tests run on a route of either split are enough by themselves
    for name, caught in table.items():
        mine = ("d24", "mm") if name.startswith("bf16x6") else ("d22", "mix")
        assert any(c[0].split("/")[0] in mine for c in caught), name
