"""Integer cases of the edge gate whose fp64 statement is an fp32 value on every route, the statement itself and its mutants.

    x = e W3^T + B1h[src] + B2h[dst],   e' = relu(x * scale + shift) + e           (include/gnnome_hip.h, "fused edge gate")

Why the result is exact on every arithmetic (csrc/operand_planes.h, edge_gate_bf.hip, edge_tile_f16.hip):
  * e holds integers of at most 8 significant bits (|e| <= 64) and W3 holds -1, 0, 1.  bf16x6 splits an operand by truncation into three
    bf16 planes that add up to it EXACTLY, so an 8-bit integer is its first plane and the other two are zero; fp16x3's first plane is
    RN16(x), exact for |x| <= 2048, and its second plane is then zero.  Every plane product is an integer, every partial sum of the
    matrix cores' fp32 adder is an integer below 2^11 (three non-zeros of W3 per row), and the exact-fp32 MFMA and the reference-order
    fma chain add the same integers.
  * the gathered tables hold integers, |x| < 2^22: B1h[src] + B2h[dst] and its sum with the product are exact in any order.
  * scale is 0.5, 1 or 2 and shift an integer: x * scale + shift is a multiple of 0.5 below 2^23, exact as mul + add and as one fma;
    relu and the residual (an integer |e| <= 64) keep that.
  * the folded encoder has integer weights and integer raw features: t = relu(W1 e_raw + b1) and e0 = W2 t + b2 are small integers in
    any order, and so are W3 W2 and W3 b2 of the algebraic fold.
  * bf16 storage (the _x16 entries) rounds x to 8 significant bits: the "small" recipe keeps 257 <= |x| <= 1023 with many odd values, so
    the rounding happens, ties included (257 lies half way between 256 and 258).
  * the fused statistics add d = x - centre and d * d per column: the "flat" and "outlier" recipes keep every such sum an integer
    below 2^24, whatever the order of the additions.
tests/test_gate_cases.py checks all of this on the CPU; tests/test_edge_gate_adversarial.py runs the cases on the device.
"""
import numpy as np
import torch

from cpu_ops import CpuViews

N_NODES = 997          # prime: the endpoint patterns below have no period shorter than it
SENTINEL = -12345.5    # what guard rows and guard columns hold; no case produces it
GRAPHS = ("uniform", "one_dst", "one_src", "ends", "n1", "dups", "straddle", "reversed", "node_perm")


# ---------------------------------------------------------------------------------------------------- inputs

def edge_rows(E, H, span=8):
    """e[r, c] = ((7 r + 3 c) mod (2 span + 1)) - span: integers in [-span, span], no period shorter than 2 span + 1 in row or channel."""
    r, c = np.arange(E, dtype=np.int64)[:, None], np.arange(H, dtype=np.int64)[None, :]
    return torch.from_numpy((((7 * r + 3 * c) % (2 * span + 1)) - span).astype(np.float32))


def gate_weight(H):
    """W3[j, :]: +1, -1, +1 at three columns that move with j at different steps: not symmetric, no permutation, rows all different."""
    W, j = torch.zeros(H, H), torch.arange(H)
    W[j, (5 * j + 1) % H] = 1.0
    W[j, (11 * j + 7) % H] = -1.0
    W[j, (3 * j + H // 2 + 2) % H] = 1.0
    return W


def node_tables(N, H, recipe="wide"):
    """(B1h, B2h)[N, H] integers.  wide: G = B1h[s] + B2h[d] = s + N d + N^2 (c mod 4) names the source row, the destination row and the
    channel.  small: 300 <= G <= 948 with every parity.  flat: G within 12 of 640.  outlier: flat, with node 0 (the source of sorted row 0
    alone) 58 lower: the other rows lie about 64 (58 to 68) above the centre."""
    n, c = torch.arange(N, dtype=torch.float64)[:, None], torch.arange(H, dtype=torch.float64)[None, :]
    if recipe == "wide":
        B1, B2 = n + float(N * N) * (c % 4), float(N) * n + 0 * c
    elif recipe == "small":
        B1, B2 = 300 + (n % 200) + 100 * (c % 4), ((7 * n) % 150) + 0 * c
    else:
        B1, B2 = 640 + 2 * (n % 4) + (c % 4), (n % 3) + 0 * c
        if recipe == "outlier":
            B1[0] -= 58
    return B1.float(), B2.float()


def graph(kind, E, T=32, R=256):
    """(src, dst, N, node_perm) of E edges in their ORIGINAL order (the views sort them by destination).  T, R: the tile height and the tiles
    per round of the route the case is for (the straddling runs sit on a tile boundary and on a round boundary)."""
    r, N, perm = np.arange(E, dtype=np.int64), N_NODES, None
    src, dst = (37 * r + 11) % N, (101 * r + 3) % N
    if kind == "one_dst":
        dst = np.full(E, N - 2)
    elif kind == "one_src":
        src = np.full(E, 5)
    elif kind == "ends":
        src, dst = np.where((5 * r) % 3 == 0, 0, N - 1), np.where((7 * r) % 4 < 2, N - 1, 0)
    elif kind == "n1":
        N, src, dst = 1, np.zeros(E, np.int64), np.zeros(E, np.int64)
    elif kind == "dups":   # runs of five copies of one edge (their e rows, and their raw features, differ)
        src, dst = (37 * (r // 5) + 11) % N, (101 * (r // 5) + 3) % N
    elif kind == "straddle":
        dst = r * (N - 2) // max(E, 1)
        for edge in (T, R * T):     # one run of equal dst over [edge - 3, edge + 5)
            if edge - 3 >= 0 and edge - 3 < E:
                dst[edge - 3:edge + 5] = dst[edge - 3]
        order = np.random.default_rng(E).permutation(E)
        src, dst = src[order], dst[order]
    elif kind == "node_perm":
        perm = torch.from_numpy(np.random.default_rng(7).permutation(N))
    elif kind not in ("uniform", "reversed"):
        raise KeyError(kind)
    return torch.from_numpy(src).int(), torch.from_numpy(dst).int(), N, perm


_PRODUCTS = {}


class Case:
    """One gate call.  src / dst: the caller's edge list; views: its sorted form (CpuViews over the renumbered endpoints where node_perm is
    given); width: the channels from `width` on are zero padding; swapped: the call runs on views.reversed(), for which the host hands the
    B2 block in as B1h and the B1 block as B2h (engine.layer); table1 / table2 are the blocks in the order of the statement: x = e W3^T + table1[first] + table2[second]."""

    def __init__(self, H, E, kind="uniform", T=32, R=256, recipe="wide", rows=None, width=None):
        self.H, self.E, self.kind, self.T, self.R, self.recipe, self.width = H, E, kind, T, R, recipe, width
        self.rows = E if rows is None else rows           # rows of the e buffer; E < rows: the num_edges prefix
        self.src, self.dst, self.N, self.node_perm = graph(kind, self.rows, T, R)
        if recipe == "outlier":     # node 0 is the source of the edge that sorts first, and of no other
            first = torch.sort(self.dst.long(), stable=True).indices[0]
            self.src[self.src == 0] = 1
            self.src[first] = 0
        s, d = self.src.long(), self.dst.long()
        if self.node_perm is not None:
            s, d = self.node_perm[s], self.node_perm[d]
        self.views = CpuViews(s, d, self.N)
        self.swapped = kind == "reversed"
        self.e = edge_rows(self.rows, H, span=8 if recipe in ("wide", "small") else 1)
        self.W3 = gate_weight(H)
        self.B1h, self.B2h = node_tables(self.N, H, recipe)
        if width is not None:       # a model of `width` channels zero-padded to H (GNNOME_NORM_LAYER_OVER's premise): the padding holds exact zeros
            for t in (self.e, self.B1h, self.B2h, self.W3):
                t[:, width:] = 0.0
            self.W3[width:] = 0.0
        c = torch.arange(H)
        self.scale = torch.tensor([0.5, 1.0, 2.0])[c % 3]
        self.shift = self._shift()
        self.shift_ln = ((c % 5) - 2).float()

    def release_host(self):
        """Drop the host copy of e once the device holds it (the largest cases are 33 MB each and a test keeps many).  x64() still works
        afterwards: a case without zero padding takes e W3^T from product64's shared rows, which depend on the row index alone."""
        assert self.width is None, "a zero-padded case multiplies its own e"
        self.e = None

    @property
    def name(self):
        return f"{self.recipe}/{self.kind}/H{self.H}/E{self.E}" + (f"of{self.rows}" if self.rows != self.E else "")

    def first_second(self):
        """The node rows the two table terms are read at, per sorted position."""
        s, d = self.views.srt_src.long(), self.views.srt_dst.long()
        return (d, s) if self.swapped else (s, d)

    def product64(self, rows, e=None):
        """e W3^T in fp64.  The case's own e rows depend on the row index alone, so the product is computed once per width for the largest
        row count asked for so far and every case takes its leading rows."""
        if e is None and self.width is not None:
            e = self.e
        if e is not None:
            return e[:rows].double() @ self.W3.double().t()
        key = (self.H, self.recipe in ("wide", "small"))
        have = _PRODUCTS.get(key)
        if have is None or have.shape[0] < rows:
            full = edge_rows(max(rows, 4 * 32 * 256 + 1), self.H, span=8 if key[1] else 1)
            have = _PRODUCTS[key] = full.double() @ self.W3.double().t()
        return have[:rows]

    def x64(self, rows=None, e=None, first_second=None):
        a, b = self.first_second() if first_second is None else first_second
        rows = self.rows if rows is None else rows
        return self.product64(rows, e) + self.B1h.double()[a[:rows]] + self.B2h.double()[b[:rows]]

    def _shift(self):
        """Per channel the integer that puts one row of the column exactly on the relu's zero and about half of the rows on either side:
        -scale * (the column's median x over an even-strided sample of at most ~2000 rows; at scale 0.5 the median of its even values, so
        that the shift is an integer)."""
        if self.E == 0:
            return torch.zeros(self.H)
        x = self.x64(self.E)[::max(1, self.E // 1024)]
        half = (self.scale == 0.5)[None, :]
        usable = ~half | (x % 2 == 0)
        usable = usable | ~usable.any(0, keepdim=True)        # a column without an even value: any row (the shift is floored below)
        ranked = torch.where(usable, x, torch.full_like(x, float("inf"))).sort(0).values
        median = ranked.gather(0, (usable.sum(0) // 2)[None, :])[0]
        return (-self.scale.double() * median).floor().float()


def statement(case, norm=0, e=None, x=None, first_second=None):
    """e'[E, H] in fp64.  norm 0: affine; 1: LayerNorm over all channels; (w << 8) | 1: LayerNorm over the first w (cpu_ops._norm's words)."""
    E = case.E
    e = case.e if e is None else e
    x = case.x64(E, e=e, first_second=first_second) if x is None else x
    if norm == 0:
        z = x * case.scale.double() + case.shift.double()
    else:
        w = (norm >> 8) or case.H
        mu = x[:, :w].mean(1, keepdim=True)
        var = ((x[:, :w] - mu) ** 2).mean(1, keepdim=True)
        z = (x - mu) * torch.rsqrt(var + 1e-5) * case.scale.double() + case.shift_ln.double()
    return torch.relu(z) + e[:E].double()


# ---------------------------------------------------------------------------------------------------- folded encoder

def encoder(H):
    """(W1[16,2], b1[16], W2[H,16], b2[H]) of small integers."""
    j, c = torch.arange(16), torch.arange(H)
    W1 = torch.stack([(j % 4) - 1, ((3 * j) % 5) - 2], 1).float()
    b1 = ((j % 3) - 1).float()
    W2 = torch.zeros(H, 16)
    W2[c, (5 * c + 1) % 16] = 1.0
    W2[c, (3 * c + 8) % 16] = -1.0
    W2[c, (7 * c + 4) % 16] = 1.0
    return W1, b1, W2, ((c % 7) - 3).float()


def raw_features(E):
    """e_raw[E, 2] integers in the ORIGINAL edge order; neighbouring edge ids differ, so copies of one edge carry different features."""
    i = torch.arange(E)
    return torch.stack([((3 * i) % 7) - 3, (5 * i) % 4], 1).float()


def encoded64(case, gather=True):
    W1, b1, W2, b2 = (w.double() for w in encoder(case.H))
    raw = raw_features(case.rows).double()
    if gather:
        raw = raw[case.views.srt_eid.long()]
    return torch.relu(raw @ W1.t() + b1) @ W2.t() + b2


# ---------------------------------------------------------------------------------------------------- bf16 storage and statistics

def to_bf16_nearest_even(x64):
    return x64.float().to(torch.bfloat16)


def to_bf16_truncated(x64):
    return (x64.float().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def shifted_sums(x64, extra_last=False):
    """(centre, S1, S2, rows): d = x - x[0]; S1 = sum d, S2 = sum d^2 per column."""
    d = x64 - x64[0]
    if extra_last:
        d = torch.cat([d, d[-1:]])
    return x64[0], d.sum(0), (d * d).sum(0), d.shape[0]


def mean_var(x64, extra_last=False):
    c, s1, s2, rows = shifted_sums(x64, extra_last)
    return c + s1 / rows, s2 / rows - (s1 / rows) ** 2


# ---------------------------------------------------------------------------------------------------- edge counts and routes

def edge_counts(T, R, ring=True):
    """The table of the issue: ragged and full first tile, most workgroups idle, a second round of one one-row tile, the 4-slot ring's wrap
    for exactly one workgroup.  Kernels without rounds (ring=False: one tile per workgroup, or pieces of their own) stop at 9 T + 1:
    more tiles than XCDs, so the tile-to-workgroup remap is no identity."""
    first = [1, T - 1, T, T + 1, 4 * T + 1]
    return first + ([R * T - 1, R * T, R * T + 1, 4 * R * T, 4 * R * T + 1] if ring else [9 * T + 1])


def persistent_grid(cu_count):
    """csrc/common.h persistent_grid(): the CU count rounded down to a multiple of the 8 XCDs, capped at 256."""
    g = min(int(cu_count), 256)
    return max(g - g % 8, 8)


# gnnome_edge_gate_f32's dispatch (csrc/edge_gate.hip) written out: (hidden, key 0, out of place) -> kernel.  Aligned tables, affine norm.
#   bf    k_edge_gate_bf        edge_gate_bf.hip, GateBF::TM = 64 at H = 64, 32 at H = 128; bf16x6; persistent, 4-slot ring
#   pl    k_edge_gate_pl        edge_gate_bf.hip launch_pl, 32-row tiles; fp16x3, bf16x6 under key 10; persistent, 4-slot ring
#   ws    k_edge_gate_ws        edge_gate.hip, GateWS::TM as GateBF; exact fp32 MFMA; persistent, 4-slot ring (5: counters, 6: barriers)
#   tile  k_edge_gate           edge_gate.hip, kTileM = 128, one tile per workgroup; bf16x6
#   f16   edge_tile_f16.hip     H = 256, 32-row tiles, two workgroups per tile (grid_pl256() / 2 tiles per round); fp16x3;
#                               under key 10 k_edge_gate_pl256 (edge_gate_pl256.hip), same tiles, bf16x6
#   stream k_edge_gate_stream   edge_gate_stream.hip, 256-row tiles, launches cut into pieces (key 4)
def gate_kernel(H, key0, out_of_place, aligned=True, affine=True):
    if affine and H in (64, 128) and key0 != 1 and aligned:
        if key0 in (0, 7, 8):
            return "pl" if H == 128 and key0 != 8 else "bf"
        if key0 in (5, 6):
            return "ws"
    if affine and H == 256 and key0 in (0, 9) and out_of_place:
        return "f16" if key0 == 0 and aligned else "stream"
    return "tile"


def tile_height(kernel, H):
    return {"bf": 64 if H == 64 else 32, "pl": 32, "ws": 64 if H == 64 else 32, "tile": 128, "f16": 32, "stream": 256}[kernel]


def tiles_per_round(kernel, grid):
    """grid: persistent_grid().  f16: grid_pl256() = grid rounded down to 16 (at least 16), two workgroups per tile."""
    if kernel == "f16":
        return max(grid - grid % 16, 16) // 2
    return grid


def ref_geometry(H, key8, grid):
    """gnnome_edge_gate_ref_f32 -> (kernel, rows per workgroup pass, workgroups per round).  refm: k_edge_gate_refm
    (reference_order_mfma.hip launch_gate_refm) - persistent, 4 * persistent_grid() workgroups, each pass 32 * RG rows with
    RG = 4 / (H / 64) row groups (1 at H = 256): the default, and the only form at 256.  scalar: k_edge_gate_ref (reference_order.hip
    launch_gate_ref, key 8 = 1) - one row per thread, kRefThreads = 256 rows per workgroup, one pass."""
    if key8 == 0 or H == 256:
        return "refm", {64: 128, 128: 64, 256: 32}[H], 4 * grid
    return "scalar", 256, None


GATE_KEYS = (0, 1, 5, 6, 7, 8, 9)
# (id, hidden, key 0, key 10, out of place)
GATE_ROUTES = [(f"H{H}-key{k}-{'out' if oop else 'inplace'}" + ("-bf16x6" if sw else ""), H, k, sw, oop)
               for H in (64, 128, 256) for oop in (False, True) for k, sw in [(k, 0) for k in GATE_KEYS] + [(0, 1)]]


# ---------------------------------------------------------------------------------------------------- mutants of the statement

def mutant_gather_next_row(case):
    """The last row of every tile gathers the table rows of its successor (clamped to the last row)."""
    a, b = case.first_second()
    r = torch.arange(case.E)
    nxt = torch.where(r % case.T == case.T - 1, torch.clamp(r + 1, max=case.E - 1), r)
    return statement(case, first_second=(a[nxt], b[nxt]))


def mutant_src_dst_swapped(case):
    a, b = case.first_second()
    return statement(case, first_second=(b, a))


def mutant_ragged_tile_not_stored(case):
    y = statement(case)
    y[(case.E // case.T) * case.T:] = SENTINEL
    return y


def mutant_second_round_stored_twice(case):
    """The first tile of the second round lands on its right-hand neighbour as well."""
    y, T, t = statement(case), case.T, case.R
    lo, hi = (t + 1) * T, min((t + 2) * T, case.E)
    if hi > lo:
        y[lo:hi] = y[t * T:t * T + hi - lo]
    return y


def mutant_residual_from_updated_row(case):
    """In place: the residual is read after the row was written, e' = relu(.) + e'."""
    y = statement(case)
    return y + (y - case.e[:case.E].double())


def mutant_relu_dropped(case):
    x = case.x64(case.E)
    return x * case.scale.double() + case.shift.double() + case.e[:case.E].double()


def mutant_shift_ignored_on_last_channels(case):
    keep = case.shift.clone()
    try:
        case.shift = keep.clone()
        case.shift[-4:] = 0.0
        return statement(case)
    finally:
        case.shift = keep


def mutant_srt_eid_ignored(case):
    return statement(case, e=encoded64(case, gather=False))


def encode_statement(case):
    return statement(case, e=encoded64(case))


def x16_statement(case):
    return to_bf16_nearest_even(case.x64(case.E)).double()


def mutant_bf16_truncated(case):
    return to_bf16_truncated(case.x64(case.E)).double()


def stats_statement(case):
    return torch.stack(mean_var(case.x64(case.E)))


def mutant_stats_one_row_more(case):
    return torch.stack(mean_var(case.x64(case.E), extra_last=True))


# name -> (what the unmutated code states, the mutant, the case that catches it: (H, E, graph, T, R, recipe))
MUTANTS = {
    "gather row r + 1 on a tile's last row": (statement, mutant_gather_next_row, (128, 33, "uniform", 32, 256, "wide")),
    "src and dst swapped": (statement, mutant_src_dst_swapped, (64, 1, "uniform", 64, 256, "wide")),
    "last ragged tile not stored": (statement, mutant_ragged_tile_not_stored, (128, 4 * 32 + 1, "one_dst", 32, 256, "wide")),
    "first tile of the second round stored twice": (statement, mutant_second_round_stored_twice, (128, 4 * 256 * 32 + 1, "straddle", 32, 256, "wide")),
    "residual from the updated row": (statement, mutant_residual_from_updated_row, (128, 31, "one_src", 32, 256, "wide")),
    "relu dropped": (statement, mutant_relu_dropped, (64, 63, "ends", 64, 256, "wide")),
    "shift ignored on the last 4 channels": (statement, mutant_shift_ignored_on_last_channels, (128, 32, "n1", 32, 256, "wide")),
    "srt_eid ignored by the folded encoder": (encode_statement, mutant_srt_eid_ignored, (64, 65, "dups", 64, 256, "wide")),
    "bf16 rounding by truncation": (x16_statement, mutant_bf16_truncated, (128, 31, "uniform", 32, 256, "small")),
    "statistics over E + 1 rows": (stats_statement, mutant_stats_one_row_more, (128, 4000, "uniform", 32, 256, "outlier")),
}
