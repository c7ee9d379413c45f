"""Exact probes for the split-arithmetic dense products (gnnome_amd/csrc/operand_planes.h), and numpy emulators of the two splits.

Helpers only, no tests.  tests/test_product_probes.py checks the recipe on the CPU, tests/test_dense_products_exact.py runs it on
the device.

THE RECIPE.  A probe is a pair of operands A[M, K], W[N, K] (and a bias[N], and a base[M, N] for the accumulating forms) for which
A W^T + bias + base is an fp32 value, and so is EVERY partial sum of the plane products it is made of, in any order and through any
arrangement of accumulators.  A kernel that keeps the plane products its header names must then return the fp64 statement bit for bit;
one that loses, doubles, misroutes or mis-scales a plane product differs - by 2^23 last places for a leading product, by as little as ONE
for a low plane under d24 (the low planes are the last places), which is why the comparison is torch.equal and not a tolerance.

  * One non-zero per dot product.  Row r of the sparse operand holds one value, at k = kpos(r) (r mod K by default); every other position is
    a zero, every third of them -0.0.  The sum over k is then exact whatever a matrix instruction does inside, and the non-zero walks
    through every k position of every 16-wide step, so a wrong lane <-> k mapping of one plane shows.
  * Both directions: `a_sparse` (A sparse against a dense W: the W planes meet A's first plane) and `w_sparse` (the mirror; output
    column n picks k = kpos(n)).
  * All values of the dense side are distinct, as in test_node_project._split_test_weights, where the family's form has that many values
    (d24, d22, mix); the `mm` form has 8 * 7 * 2 = 112 values, laid out so that neighbours in a row and in a column differ.  The sparse
    side's value of row r is (-1)^i 2^(i // 2 - 2), i = (r // K + r mod K) mod 10: the rows that share a k position (r, r + K, ...) hold
    different values, up to ten of them; rows with different k are told apart by the dense side.
  * Every plane of every operand is a NORMAL fp16 / bf16 number or zero: all magnitudes lie in [2^-2, 2^9], second fp16 planes are
    >= 2^-10.

THE FAMILIES (name: dense side x sparse side; the plane products they reach, x plane first)
    d24   24 significant bits in [1, 2) x +-2^p          bf16x6: w_sparse hh mh lh, a_sparse hh hm hl.  NOT exact under fp16x3 (22 bits).
    mm    +-2^a (1 + c 2^-11) x +-2^p (1 + d 2^-11)      bf16x6: hh hm mh mm; the dropped ml, lm, ll are zero.  NOT exact under fp16x3
                                                         (the sparse side's second plane meets the dense side's: x2 w2 != 0).
    d22   22 significant bits in [1, 2) x +-2^p          fp16x3: w_sparse 11 21, a_sparse 11 12.  Exact under bf16x6 too (8 + 8 + 6 bits).
    mix   18 significant bits in [1, 8) x +-2^p (1+c/8)  fp16x3: 11 21 / 11 12 with a first plane that is no power of two; x2 w2 = 0
                                                         because the sparse side has no second plane.  Exact under bf16x6 too.
Bias and base are integer multiples (|multiple| <= 8) of the family's `quantum`, the last place of its largest results, so the premise
holds with them.
"""
import itertools

import numpy as np

# ------------------------------------------------------------------------------------------------ the two splits, in numpy


def split_f16(a):
    a1 = a.astype(np.float16)
    r = ((a - a1.astype(np.float32)) * np.float32(2048)).astype(np.float32)      # exact: a - a1 fits fp32, so does its 2^11-fold
    return a1.astype(np.float32), r.astype(np.float16).astype(np.float32)


def trunc_bf16(a):
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split_bf16(a):
    h = trunc_bf16(a)
    r = (a - h).astype(np.float32)
    m = trunc_bf16(r)
    return h, m, (r - m).astype(np.float32)


def _step(a, b, k0):
    return a[:, k0:k0 + 16].astype(np.float64) @ b[:, k0:k0 + 16].astype(np.float64).T


def chain(terms, k=None, reverse=False, init=None):
    """fp32 accumulator over 16-wide k steps; within a step the products are exact and summed before one rounding (a model of one MFMA).
    `init`: what the accumulator starts from (a bias row, a base tile); `reverse`: the k steps last to first."""
    rows, cols = terms[0][0].shape[0], terms[0][1].shape[0]
    k = terms[0][0].shape[1] if k is None else min(k, terms[0][0].shape[1])
    out = np.zeros((rows, cols), np.float32) if init is None else np.broadcast_to(init, (rows, cols)).astype(np.float32)
    steps = range(0, k, 16)
    for k0 in (reversed(steps) if reverse else steps):
        for a, b in terms:
            out = (out.astype(np.float64) + _step(a, b, k0)).astype(np.float32)
    return out


BF16X6_KEPT = ("hh", "hm", "mh", "mm", "hl", "lh")     # x plane first: six of the nine
BF16X6_ORDER = ("lh", "hl", "mm", "mh", "hm", "hh")    # smallest terms first, as k_linear_bf2 issues them
F16X3_KEPT = ("11", "12", "21")                        # three of the four; 12 and 21 go to the second accumulator
F16X3_SCALE = 2.0 ** -11


def bf16x6(x, w, keep=BF16X6_KEPT, order=BF16X6_ORDER, reverse=False, init=None):
    """x w^T as the bf16x6 kernels compute it: the plane products named in `keep`, issued in `order` within every k step, one fp32 accumulator."""
    xp = dict(zip("hml", split_bf16(x)))
    wp = dict(zip("hml", split_bf16(w)))
    terms = [(xp[t[0]], wp[t[1]]) for t in order if t in keep]
    return chain(terms, reverse=reverse, init=init)


def f16x3(x, w, keep=F16X3_KEPT, order=("12", "21"), reverse=False, fold="end", scale=F16X3_SCALE, init=None):
    """x w^T as the fp16x3 kernels compute it: x1 w1 in the main accumulator, x1 w2 and x2 w1 in a second one that is folded in with `scale`
    (2^-11) - once at the end (fold="end", the edge-tile kernels) or after every k step (fold="step")."""
    xp = dict(zip("12", split_f16(x)))
    wp = dict(zip("12", split_f16(w)))
    main_terms = [(xp["1"], wp["1"])] if "11" in keep else []
    corr_terms = [(xp[t[0]], wp[t[1]]) for t in order if t in keep]
    rows, cols = x.shape[0], w.shape[0]
    zero = np.zeros((rows, cols), np.float32)
    s = np.float32(scale)
    if fold == "end":
        main = chain(main_terms, reverse=reverse, init=init) if main_terms else (zero if init is None else np.broadcast_to(init, zero.shape).astype(np.float32))
        corr = chain(corr_terms, reverse=reverse) if corr_terms else zero
        return (main + corr * s).astype(np.float32)
    assert fold == "step"
    main = zero if init is None else np.broadcast_to(init, zero.shape).astype(np.float32)
    steps = range(0, x.shape[1], 16)
    for k0 in (reversed(steps) if reverse else steps):
        for a, b in main_terms:
            main = (main.astype(np.float64) + _step(a, b, k0)).astype(np.float32)
        corr = zero
        for a, b in corr_terms:
            corr = (corr.astype(np.float64) + _step(a, b, k0)).astype(np.float32)
        main = (main + corr * s).astype(np.float32)
    return main


def mutants():
    """name -> (split, emulator keywords): every kept plane product removed in turn, and the second accumulator's scale applied twice / not at all."""
    out = {}
    for t in BF16X6_KEPT:
        out[f"bf16x6 without x{t[0]}.w{t[1]}"] = ("bf16x6", {"keep": tuple(u for u in BF16X6_KEPT if u != t)})
    for t in F16X3_KEPT:
        out[f"fp16x3 without x{t[0]}.w{t[1]}"] = ("fp16x3", {"keep": tuple(u for u in F16X3_KEPT if u != t)})
    out["fp16x3 with 2^-11 applied twice"] = ("fp16x3", {"scale": 2.0 ** -22})
    out["fp16x3 with 2^-11 not applied"] = ("fp16x3", {"scale": 1.0})
    return out


EMULATOR = {"bf16x6": bf16x6, "fp16x3": f16x3}

# ------------------------------------------------------------------------------------------------ the probes

FAMILIES = ("d24", "mm", "d22", "mix")
DIRECTIONS = ("a_sparse", "w_sparse")
EXACT_UNDER = {   # which arithmetic a family's premise holds for ("fp32": a kernel that multiplies fp32 operands exactly)
    "d24": ("bf16x6", "fp32"), "mm": ("bf16x6", "fp32"), "d22": ("bf16x6", "fp16x3", "fp32"), "mix": ("bf16x6", "fp16x3", "fp32"),
}
QUANTUM = {"d24": 2.0 ** -21, "mm": 2.0 ** -13, "d22": 2.0 ** -19, "mix": 2.0 ** -16}   # the last place of the family's largest results


def families_for(split):
    return tuple(f for f in FAMILIES if split in EXACT_UNDER[f])


def row_counts(K):
    return (1, 31, 33, 129, 2 * K + 1)


def _sparse_sign_exp(idx, K, exps=(-2, -1, 0, 1, 2)):
    i = (idx // K + idx % K) % (2 * len(exps))
    return np.where(i % 2 == 0, 1.0, -1.0), np.asarray(exps)[i // 2]


def _dense_values(family, rows, K, rng, positive=False, residual=False):
    count = rows * K
    sign = np.ones(count) if positive else rng.choice([-1.0, 1.0], size=count)
    if family == "mm":
        n, k = np.divmod(np.arange(count), K)
        i = (k + 17 * n) % 112
        v = (1.0 if positive else np.where(i % 2 == 0, 1.0, -1.0)) * np.exp2(0 if residual else i // 2 % 8) * (1.0 + (i // 16 + 1) * 2.0 ** -11)
        return v.astype(np.float32).reshape(rows, K)
    repeats = []

    def draw(population):   # distinct while the form has that many values (a threshold shape of some 10^7 elements has not)
        repeats.append(count > population)
        return rng.choice(population, size=count, replace=count > population)

    if family == "d24":     # (2^23 + j) 2^-23 with j odd (a low plane in every value) and 2^12 last places of headroom below 2
        j = draw(2 ** 22 - 2 ** 11) * 2 + 1
        v = sign * (2.0 ** 23 + j) * 2.0 ** -23
    elif family == "d22":   # (2^21 + j) 2^-21, j odd: the second fp16 plane is never zero
        j = draw(2 ** 20 - 2 ** 9) * 2 + 1
        v = sign * (2.0 ** 21 + j) * 2.0 ** -21
    elif family == "mix":   # 18 significant bits over three binades
        j = draw(3 * 2 ** 17 - 2 ** 8)
        v = sign * (2.0 ** 17 + j % 2 ** 17) * 2.0 ** -17 * np.exp2(j // 2 ** 17)
    else:
        raise ValueError(family)
    v = v.astype(np.float32)
    assert repeats[0] or np.unique(v.view(np.uint32)).size == v.size
    return v.reshape(rows, K)


def _sparse_values(family, rows, K, kpos, positive=False, exps=(-2, -1, 0, 1, 2)):
    idx = np.arange(rows)
    sign, p = _sparse_sign_exp(idx, K, exps)
    sign = np.ones(rows) if positive else sign
    v = sign * np.exp2(p)
    if family == "mm":
        v = v * (1.0 + ((3 * idx + idx // K) % 7 + 1) * 2.0 ** -11)
    elif family == "mix":
        v = v * (1.0 + ((3 * idx + idx // K) % 7 + 1) / 8.0)
    out = np.zeros((rows, K), np.float32)
    out.reshape(-1)[2::3] = -0.0
    out[idx, kpos(idx)] = v.astype(np.float32)
    return out


class Probe:
    """A, W, bias, base as fp32 numpy arrays (bias / base None when not asked for) and the fp64 statement of A W^T + bias + base."""

    def __init__(self, family, direction, A, W, bias, base):
        self.family, self.direction, self.A, self.W, self.bias, self.base = family, direction, A, W, bias, base

    def statement64(self):
        s = self.A.astype(np.float64) @ self.W.astype(np.float64).T
        if self.bias is not None:
            s = s + self.bias.astype(np.float64)
        if self.base is not None:
            s = s + self.base.astype(np.float64)
        return s

    def statement(self):
        """The statement as fp32 - the premise is that the cast loses nothing."""
        s = self.statement64()
        s32 = s.astype(np.float32)
        assert np.array_equal(s32.astype(np.float64), s), f"{self.family}/{self.direction}: the statement is not an fp32 value"
        return s32

    def init(self):
        """bias + base as one fp32 array an accumulator may start from (exact: both are small multiples of one quantum)."""
        if self.bias is None and self.base is None:
            return None
        t = np.zeros((self.A.shape[0], self.W.shape[0]), np.float64)
        if self.bias is not None:
            t = t + self.bias.astype(np.float64)
        if self.base is not None:
            t = t + self.base.astype(np.float64)
        return t.astype(np.float32)


RESIDUAL_FAMILIES = ("mm", "d22", "mix")


def probe(family, direction, M, K, N, seed=0, bias=True, base=False, kpos=None, positive=False, residual=False):
    """The probe of `family` for an [M, K] x [N, K]^T product.  kpos(index) -> k position of the sparse side's non-zero (default index mod K;
    the weight gradients, whose K is the row count, spread it over the row chunks they reduce over).  positive: no negative operand
    (for a product that is followed by a relu).

    residual: the base IS the operand, A W^T + A with a square W - what the inference gate (relu(e W3^T) + e) and the fused data gradient
    (de + dxe Wt^T with dxe = de) compute.  The sum of two unrelated dense values needs a common window, so the sparse side's exponents are 0
    and 1 only and the `mm` dense side stays in [1, 2).  RESIDUAL_FAMILIES hold the premise then; d24 does not (24 bits leave no room for a
    second addend of the same size).  test_product_probes.py proves both, and that d22 + mix + mm still catch every mutant."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), DIRECTIONS.index(direction), M, K, N])
    kpos = (lambda i: i % K) if kpos is None else kpos
    if residual:
        assert N == K and not bias and not base
        if direction == "a_sparse":
            A, W = _sparse_values(family, M, K, kpos, positive, exps=(0, 1)), _dense_values(family, N, K, rng, positive, residual=True)
        else:
            A, W = _dense_values(family, M, K, rng, positive, residual=True), _sparse_values(family, N, K, kpos, positive, exps=(0, 1))
        return Probe(family, direction, A, W, None, A.copy())
    if direction == "a_sparse":
        A, W = _sparse_values(family, M, K, kpos, positive), _dense_values(family, N, K, rng, positive)
    else:
        A, W = _dense_values(family, M, K, rng, positive), _sparse_values(family, N, K, kpos, positive)
    q = QUANTUM[family]
    b = (rng.integers(-8, 9, size=N) * q).astype(np.float32) if bias else None
    c = (rng.integers(-8, 9, size=(M, N)) * q).astype(np.float32) if base else None
    return Probe(family, direction, A, W, b, c)


def all_plane_orders(split):
    if split == "bf16x6":
        return [{"order": o} for o in itertools.permutations(BF16X6_ORDER)]
    return [{"order": o, "fold": f} for o in itertools.permutations(("12", "21")) for f in ("end", "step")]
