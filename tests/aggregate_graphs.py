"""Seeded graphs that aim at the list and hub edge cases of the gated aggregation (gnnome_amd/csrc/node_aggregate.hip), and the
exact-arithmetic input recipe of tests/test_aggregate_adversarial.py.  The CPU tests of this module are in tests/test_aggregate_graphs.py.

Every family returns a dict

    src, dst        int32 edge list (in a shuffled edge order), n nodes
    in_degree       what the construction CLAIMS per node (int64[n]) - written down from the family's specification, the pool nodes'
    out_degree      share counted while the lists are dealt out; the CPU tests compare it with a count over src / dst
    hubs            sorted ids of the nodes whose in-list + out-list exceed HUB_THRESHOLD items
    spec            {node id: (din, dout)} of the nodes the family is about
    probe_on / probe_off / probe_src
                    two nodes with ONE in-edge each and no out-edge, both fed by probe_src (whose only edges these are): the tests
                    open the gate of the first and close the gate of the second

The families:

    lists()         one node per (din, dout) in LIST_LENGTHS x LIST_LENGTHS - the lengths sit on the step sizes of all three widths (G U
                    = 16 items at H = 64, 8 at 128, 2 at 256), on the pair kernel's steps (4 and 2 items, batches of 32) and on the
                    64-item batch boundaries; neighbours come from a pool of low-degree nodes; self-loops (one node carries two),
                    a triplicate parallel edge, isolated nodes at index 0 and n - 1
    hub_edges()     lists around HUB_THRESHOLD: 4095 / 4096 items (not split) and 4097 (split), in-edges only, out-edges only, an
                    in / out boundary inside a 64-item batch with empty later chunks, a long hub, self-loops inside a hub's
                    lists, hubs at node 0 and at node n - 1
    many_hubs(k)    k hubs of 4100 - 4400 items at every MANY_HUBS_STRIDE-th node id, written in shuffled order; every hub edge
                    joins a hub to a non-hub node
    tails(n, e, k)  (not in FAMILIES: no probes) tiny graphs whose highest-numbered nodes have no edge and whose last in-list ends at
                    position E - 1, for the aggregation backward's clamped index requests

Two exact recipes: exact_inputs / exact_sums (gates of GATE_ON / GATE_OFF: integer node sums) and, for the aggregation's BACKWARD, the
HALVES recipe exact_backward_inputs / exact_backward / exact_backward_bound (a third gate value GATE_HALF = 0 with a sigmoid of exactly
0.5: every output a multiple of 1/4), described where they are defined.
"""
import numpy as np
import torch

# gnnome_amd/csrc/node_aggregate.hip: kHubThreshold, kHubChunks, kHubCap and the 64 items a wave fetches the indices of at once
HUB_THRESHOLD = 4096      # a node with MORE items (in-edges + out-edges) than this is a hub
HUB_CHUNKS = 128          # chunks a hub's list is cut into: whole 64-item batches each
HUB_CAP = 64              # hubs per graph that get the split path - the lowest node ids
BATCH = 64

LIST_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 127, 128, 129)
MANY_HUBS = (63, 64, 65, 70)
MANY_HUBS_STRIDE = 37

# The exact recipe: gate inputs whose device sigmoid rcp(1 + exp(-x)) is exactly 1.0f or exactly 0.0f.  exp(-64) vanishes next to 1, so
# +64 gives rcp(1) = 1.  The closed side needs exp(-x) to OVERFLOW (x < -88.7): 1 + inf = inf, rcp(inf) = 0.  At -64, which was the
# first choice, exp(64) = 6.2e27 is an ordinary float and the sigmoid is 1.6e-28 - not zero: a sum that ends at the integer 0 would
# keep such crumbs, in an order-dependent amount (tests/test_aggregate_adversarial.py::test_a_gate_of_minus_64_is_not_exactly_closed measures it).
GATE_ON, GATE_OFF = 64.0, -128.0
TABLE_MAX = 8             # table rows are integers in [-TABLE_MAX, TABLE_MAX]
EXACT_LIMIT = 1 << 24     # below this every integer is an fp32 value: integer sums have the same bits in every order


class _Builder:
    def __init__(self, n, seed):
        self.n, self.rng = n, np.random.default_rng(seed)
        self.src, self.dst = [], []
        self.din, self.dout = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self.spec = {}

    def claim(self, node, din, dout):
        """`node` is specified to end with exactly these degrees (edges added before and after count)."""
        self.spec[int(node)] = (int(din), int(dout))
        self.din[node], self.dout[node] = din, dout

    def edges(self, u, v, count_u=True, count_v=True):
        """Edges u[i] -> v[i]; the endpoints that are not `claim`ed nodes have their share counted here."""
        u, v = np.broadcast_arrays(np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64))
        self.src += u.tolist()
        self.dst += v.tolist()
        if count_u:
            np.add.at(self.dout, u, 1)
        if count_v:
            np.add.at(self.din, v, 1)

    def lists_of(self, node, din, dout, pool, replace=False, loops=0):
        """`node` gets din in-edges and dout out-edges, `loops` of each being self-loops, the rest from / to nodes of `pool`."""
        self.claim(node, din, dout)
        self.edges(self.rng.choice(pool, size=din - loops, replace=replace), node, count_v=False)
        self.edges(node, self.rng.choice(pool, size=dout - loops, replace=replace), count_u=False)
        if loops:
            self.edges([node] * loops, node, count_u=False, count_v=False)

    def probes(self, probe_src, probe_on, probe_off):
        self.claim(probe_src, 0, 2)
        self.claim(probe_on, 1, 0)
        self.claim(probe_off, 1, 0)
        self.edges([probe_src, probe_src], [probe_on, probe_off], count_u=False, count_v=False)
        self.probe = dict(probe_src=int(probe_src), probe_on=int(probe_on), probe_off=int(probe_off))

    def finish(self):
        order = self.rng.permutation(len(self.src))
        src = torch.from_numpy(np.asarray(self.src, dtype=np.int32)[order])
        dst = torch.from_numpy(np.asarray(self.dst, dtype=np.int32)[order])
        din, dout = torch.from_numpy(self.din), torch.from_numpy(self.dout)
        hubs = torch.nonzero(din + dout > HUB_THRESHOLD).flatten().tolist()
        return dict(src=src, dst=dst, n=self.n, in_degree=din, out_degree=dout, hubs=hubs, spec=dict(self.spec), **self.probe)


def lists(seed=11):
    pairs = [(a, b) for a in LIST_LENGTHS for b in LIST_LENGTHS]
    n_pool, extra = 4000, 12
    n = len(pairs) + n_pool + extra + 2
    b = _Builder(n, seed)
    ids = b.rng.permutation(np.arange(1, n - 1))           # node 0 and node n - 1 stay isolated
    special, ids = ids[:len(pairs) + extra], ids[len(pairs) + extra:]
    pool = np.sort(ids)
    for node, (din, dout) in zip(special, pairs):
        b.lists_of(node, din, dout, pool)
    x = [int(v) for v in special[len(pairs):]]
    b.lists_of(x[0], 1 + 3, 1 + 2, pool, loops=1)           # one self-loop among other edges
    b.lists_of(x[1], 2 + 17, 2 + 64, pool, loops=2)         # two self-loops
    b.lists_of(x[2], 1, 1, pool, loops=1)                   # nothing but a self-loop
    b.claim(x[3], 2, 3)                                     # x3 -> x4 three times (and two more edges at each end)
    b.claim(x[4], 3 + 1, 1)
    b.edges([x[3]] * 3, x[4], count_u=False, count_v=False)
    b.edges(b.rng.choice(pool, size=2, replace=False), x[3], count_v=False)
    b.edges(b.rng.choice(pool, size=1), x[4], count_v=False)
    b.edges(x[4], b.rng.choice(pool, size=1), count_u=False)
    b.claim(x[5], 0, 0)                                     # an isolated node inside the range
    b.probes(x[6], x[7], x[8])
    for node in x[9:]:
        b.claim(node, 0, 0)
    b.claim(0, 0, 0)
    b.claim(n - 1, 0, 0)
    return b.finish()


HUB_EDGE_SPECS = (          # (din, dout, self-loops inside both lists)
    (2048, 2047, 0),        # 4095 items: one below the threshold
    (2048, 2048, 0),        # 4096: AT the threshold, not split
    (2049, 2048, 0),        # 4097: the shortest split list
    (4097, 0, 0),           # in-edges only
    (0, 4097, 0),           # out-edges only
    (1, 4096, 0),
    (4130, 37, 0),          # chunks of 64: the boundary falls inside the batch of chunk 64, chunks 66 .. 127 are empty
    (8321, 8190, 0),        # chunks of 192 items
    (2150, 2150, 50),       # 50 self-loops inside either list
)


def hub_edges(seed=12):
    n_pool = 9000
    n = n_pool + len(HUB_EDGE_SPECS) + 3 + 2
    b = _Builder(n, seed)
    inner = b.rng.permutation(np.arange(1, n - 1))
    # node 0: the in-edges-only hub, node n - 1: the out-edges-only hub; the others anywhere in between
    place = {3: 0, 4: n - 1}
    rest = iter(inner[:len(HUB_EDGE_SPECS) + 3])
    nodes = [place[i] if i in place else int(next(rest)) for i in range(len(HUB_EDGE_SPECS))]
    probe_nodes = [int(next(rest)) for _ in range(3)]
    taken = set(nodes) | set(probe_nodes)
    pool = np.asarray([v for v in range(n) if v not in taken], dtype=np.int64)
    for node, (din, dout, loops) in zip(nodes, HUB_EDGE_SPECS):
        b.lists_of(node, din, dout, pool, loops=loops)
    b.probes(*probe_nodes)
    return b.finish()


def many_hubs(k, seed=13):
    n = MANY_HUBS_STRIDE * k + 11
    b = _Builder(n, seed + k)
    hub_ids = 5 + MANY_HUBS_STRIDE * np.arange(k)
    probe_nodes = [2, 3, n - 2]
    taken = set(hub_ids.tolist()) | set(probe_nodes)
    pool = np.asarray([v for v in range(n) if v not in taken], dtype=np.int64)
    for node in b.rng.permutation(hub_ids):                 # written in shuffled order
        items = int(b.rng.integers(HUB_THRESHOLD + 4, 4401))
        din = int(b.rng.integers(0, items + 1)) if b.rng.random() < 0.8 else int(b.rng.choice([0, items, 1, items - 1]))
        b.lists_of(int(node), din, items - din, pool, replace=True)
    b.probes(*probe_nodes)
    return b.finish()


FAMILIES = {"lists": lists, "hub_edges": hub_edges, **{f"many_hubs{k}": (lambda k=k: many_hubs(k)) for k in MANY_HUBS}}
_CACHE = {}


def graph(name):
    """The named graph, built once per process (read-only: the tests share it)."""
    if name not in _CACHE:
        _CACHE[name] = FAMILIES[name]()
    return _CACHE[name]


# ---------------------------------------------------------------------------------------------- the exact recipe

def exact_inputs(num_edges, n, hidden, seed):
    """(gate inputs [E, H] of GATE_ON / GATE_OFF, A2 [n, H], A3 [n, H], X [E, H]): the tables and the X rows hold integers in
    [-TABLE_MAX, TABLE_MAX], a different random row per node / edge.  Rows are per SORTED position and per internal node id - the
    caller indexes them with the views' own arrays."""
    g = torch.Generator().manual_seed(seed)
    on = torch.randint(0, 2, (num_edges, hidden), generator=g, dtype=torch.int8).bool()
    gates = torch.where(on, torch.tensor(GATE_ON), torch.tensor(GATE_OFF))
    tab = lambda rows: torch.randint(-TABLE_MAX, TABLE_MAX + 1, (rows, hidden), generator=g).float()  # noqa: E731
    return gates, tab(n), tab(n), tab(num_edges)


def exact_sums(s, d, gates, A2, A3, n, dtype=torch.int64):
    """sum_in[i] = sum over positions p with d[p] = i of open(p) * A2[s[p]], sum_out[i] = sum over s[p] = i of open(p) * A3[d[p]], and
    the open-gate counts of both lists - evaluated in `dtype` (int64: the statement; float32: the same sums as index_add forms them), on the
    device the inputs are on."""
    s, d = s.long(), d.long()
    on = (gates > 0).to(dtype)
    zeros = torch.zeros((n, gates.shape[1]), dtype=dtype, device=gates.device)
    return dict(sum_in=zeros.index_add(0, d, on * A2.to(dtype)[s]), sum_out=zeros.index_add(0, s, on * A3.to(dtype)[d]),
                cnt_in=zeros.index_add(0, d, on), cnt_out=zeros.index_add(0, s, on))


def exact_segment_sums(s, d, X, n, dtype=torch.int64):
    """(sum of X rows over every node's in-list, over its out-list), rows per sorted position."""
    zeros = torch.zeros((n, X.shape[1]), dtype=dtype, device=X.device)
    return zeros.index_add(0, d.long(), X.to(dtype)), zeros.index_add(0, s.long(), X.to(dtype))


# ---------------------------------------------------------------------------------------------- the halves recipe
#
# The exact recipe above never tests a gradient term: at a device sigmoid of exactly 1 or 0 the factor s (1 - s) of the aggregation's
# backward vanishes.  A THIRD gate value, 0, is to give a device sigmoid of exactly 0.5 (exp(-0) = 1, 1 + 1 = 2, rcp(2) = 0.5 - the
# premise the device tests open with) and s (1 - s) = 0.25.  With small INTEGER tables, de0, xe and mean, scale in {1, 2} and shift an odd
# multiple of 0.5, every output of the backward
#     sum_in[i]  = sum_{p: d_p = i} s_p Tb[s_p]                    sum_out[i] = sum_{p: s_p = i} s_p Tf[d_p]
#     de'[p]     = de0[p] + s_p (1 - s_p) (Tf[d_p] A2[s_p] - Uf[d_p] + Tb[s_p] A3[d_p] - Ub[s_p])
#     s1 = sum_p de'[p] m_p                                        s2 = sum_p de'[p] m_p (xe[p] - mean),   m_p = (xe[p] scale + shift > 0)
# is a multiple of 1/4, and as long as the sum of the ABSOLUTE values of a sum's terms stays below 2^24 quarters (exact_backward_bound) so
# is every partial sum, in every order, with or without fma contraction: the fp32 result has ONE possible bit pattern.  xe scale + shift is
# exact and never 0, so the relu mask does not depend on how the expression is rounded either; the integer xe is its own bfloat16 copy.
GATE_HALF = 0.0
BACKWARD_MAX = 2          # tables, de0, xe and mean are integers in [-BACKWARD_MAX, BACKWARD_MAX]
NODE_TABLES = ("Tf", "Uf", "Tb", "Ub", "A2", "A3")


def exact_backward_inputs(num_edges, n, hidden, seed):
    """The inputs of the halves recipe as a dict: gates [E, H] of GATE_HALF (about half of them) / GATE_ON / GATE_OFF, mixed within rows;
    Tf, Uf, Tb, Ub, A2, A3 [n, H], de0 and xe [E, H], mean [H]: integers in [-BACKWARD_MAX, BACKWARD_MAX]; scale [H] in {1, 2}; shift [H] an
    odd multiple of 0.5.  Edge rows are per SORTED position, node rows per internal node id."""
    g = torch.Generator().manual_seed(seed)
    kind = torch.randint(0, 4, (num_edges, hidden), generator=g, dtype=torch.int8)
    gates = torch.full((num_edges, hidden), GATE_HALF)
    gates[kind == 2], gates[kind == 3] = GATE_ON, GATE_OFF
    ints = lambda *shape: torch.randint(-BACKWARD_MAX, BACKWARD_MAX + 1, shape, generator=g).float()  # noqa: E731
    out = dict(gates=gates, **{k: ints(n, hidden) for k in NODE_TABLES}, de0=ints(num_edges, hidden), xe=ints(num_edges, hidden))
    out["scale"] = torch.randint(1, 3, (hidden,), generator=g).float()
    out["shift"] = torch.randint(-3, 3, (hidden,), generator=g).float() + 0.5
    out["mean"] = ints(hidden)
    return out


def _quarters(s, d, t):
    """The integer parts of the statement, int64, in the units that make them integers: q = 4 sigmoid (0 / 2 / 4), half = [s (1 - s) = 1/4],
    the relu mask m, the bracket of de' and the tables gathered at the endpoints."""
    i64 = lambda x: x.round().long()  # noqa: E731
    gates = t["gates"]
    known = (gates == GATE_ON) | (gates == GATE_OFF) | (gates == GATE_HALF)
    assert bool(known.all()), "a gate that is none of GATE_ON / GATE_OFF / GATE_HALF"
    q = 4 * (gates == GATE_ON).long() + 2 * (gates == GATE_HALF).long()
    tb_s, ub_s, a2_s = i64(t["Tb"])[s], i64(t["Ub"])[s], i64(t["A2"])[s]
    tf_d, uf_d, a3_d = i64(t["Tf"])[d], i64(t["Uf"])[d], i64(t["A3"])[d]
    m = (2 * i64(t["xe"]) * i64(t["scale"]) + i64(2 * t["shift"]) > 0).long()
    return q, (q == 2).long(), m, (tf_d, a2_s, uf_d, tb_s, a3_d, ub_s)


def exact_backward(s, d, t, n):
    """The statement of the aggregation's backward on the sorted endpoint arrays (s, d) and the inputs `t` of exact_backward_inputs, in
    int64 quarters, returned as float64: dict(sum_in, sum_out [n, H], de [E, H], s1, s2 [H]).  On the device the inputs are on."""
    s, d = s.long(), d.long()
    q, half, m, (tf_d, a2_s, uf_d, tb_s, a3_d, ub_s) = _quarters(s, d, t)
    zeros = torch.zeros((n, q.shape[1]), dtype=torch.int64, device=q.device)
    de = 4 * t["de0"].round().long() + half * (tf_d * a2_s - uf_d + tb_s * a3_d - ub_s)
    xc = t["xe"].round().long() - t["mean"].round().long()
    out = dict(sum_in=zeros.index_add(0, d, q * tb_s), sum_out=zeros.index_add(0, s, q * tf_d), de=de, s1=(de * m).sum(0), s2=(de * m * xc).sum(0))
    return {k: v.double() / 4.0 for k, v in out.items()}


def exact_backward_bound(s, d, t, n):
    """The condition of the halves recipe: per output, the largest sum of the absolute values of the terms of one of its sums, in quarters
    (every product counted factor by factor, so that a kernel may also distribute them).  All below EXACT_LIMIT = 2^24: every partial sum
    any kernel may form is an fp32 value."""
    s, d = s.long(), d.long()
    q, half, m, (tf_d, a2_s, uf_d, tb_s, a3_d, ub_s) = _quarters(s, d, t)
    zeros = torch.zeros((n, q.shape[1]), dtype=torch.int64, device=q.device)
    de = 4 * t["de0"].round().long().abs() + half * ((tf_d * a2_s).abs() + uf_d.abs() + (tb_s * a3_d).abs() + ub_s.abs())
    xc = t["xe"].round().long().abs() + t["mean"].round().long().abs()
    big = lambda v: int(v.max()) if v.numel() else 0  # noqa: E731
    return dict(sum_in=big(zeros.index_add(0, d, (q * tb_s).abs())), sum_out=big(zeros.index_add(0, s, (q * tf_d).abs())), de=big(de),
                s1=big((de * m).sum(0)), s2=big((de * m * xc).sum(0)))


# The clamp and tail cases of the fused backward (k_agg_bwd_fused requests the first 64 neighbour ids of both lists of every node before it
# knows the lists' lengths, clamped to position E - 1): the HIGHEST-numbered nodes have no edge at all (in_ptr[node] = out_ptr[node] = E: every
# prefetch of theirs is clamped), the last node that has in-edges ends its list at position E - 1, n is no multiple of the 4 nodes of a
# workgroup, E goes down to 1.  (n, E, items in the last in-list)
TAILS = ((1, 1, 1), (1, 3, 3), (5, 1, 1), (5, 2, 1), (5, 9, 4), (33, 1, 1), (33, 40, 5), (33, 200, 70), (33, 131, 64))


def tails(n, num_edges, last_list, seed=14):
    """n nodes of which the highest min(3, n - 1) are isolated; the highest-numbered node that is not gets `last_list` in-edges, the other
    edges fall anywhere among the nodes that may have edges (self-loops and parallel edges included)."""
    rng = np.random.default_rng(seed + 1000 * n + num_edges)
    active = max(1, n - 3)
    src = rng.integers(0, active, size=num_edges)
    dst = rng.integers(0, active, size=num_edges)
    dst[:last_list] = active - 1
    if active > 1:
        dst[last_list:] = rng.integers(0, active - 1, size=num_edges - last_list)
    order = rng.permutation(num_edges)
    src, dst = src[order], dst[order]
    return dict(src=torch.from_numpy(src.astype(np.int32)), dst=torch.from_numpy(dst.astype(np.int32)), n=n, active=active, last_list=last_list,
                in_degree=torch.bincount(torch.from_numpy(dst), minlength=n), out_degree=torch.bincount(torch.from_numpy(src), minlength=n), hubs=[],
                spec={}, probe_src=None, probe_on=None, probe_off=None)
