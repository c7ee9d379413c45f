"""The nb_pos_enc > 0 half of the reference's add_positional_encoding (utils/data_utils.py:59-90) restated densely in torch fp64, and the
graphs the positional-encoding tests run on.  A restatement, line by line, of what the reference computes with scipy sparse
matrices - none of its text.  tests/test_positional_statement.py pins it on hand-computed cases; tests/test_positional.py holds the
device kernels (gnnome_amd/csrc/positional.hip) to it."""
import random

import torch

F64 = torch.float64


def adjacency(src, dst, n, sources_on_rows=True):
    """g.adjacency_matrix(scipy_fmt="csr") (:61, :76) as a dense fp64 matrix: one count per edge, so a parallel edge counts once per
    copy (scipy sums duplicate entries when it multiplies).  sources_on_rows: A[u, v] = mult(u -> v); False: the transposed convention."""
    A = torch.zeros((n, n), dtype=F64)
    s, d = torch.as_tensor(src).long(), torch.as_tensor(dst).long()
    A.index_put_((s, d) if sources_on_rows else (d, s), torch.ones(s.numel(), dtype=F64), accumulate=True)
    return A


def degrees(src, dst, n):
    """(g.in_degrees(), g.out_degrees()) (:50-51) as int64[n]."""
    return (torch.bincount(torch.as_tensor(dst).long(), minlength=n), torch.bincount(torch.as_tensor(src).long(), minlength=n))


def rw(src, dst, n, pe_dim, sources_on_rows=True):
    """type_pos_enc == 'RW' (:59-72) -> fp64 [n, pe_dim], before the reference's .float()."""
    A = adjacency(src, dst, n, sources_on_rows)                      # :61
    in_deg, _ = degrees(src, dst, n)
    Dinv = torch.diag(in_deg.clamp(min=1).to(F64) ** -1.0)           # :62  in_degrees().clip(1) ** -1.0
    RW = A @ Dinv                                                    # :63
    M = RW                                                           # :64
    PE = [M.diagonal().clone()]                                      # :66
    M_power = M                                                      # :67
    for _ in range(pe_dim - 1):                                      # :68
        M_power = M_power @ M                                        # :69
        PE.append(M_power.diagonal().clone())                        # :70
    return torch.stack(PE, dim=-1)                                   # :71


def pr(src, dst, n, pe_dim):
    """type_pos_enc == 'PR' (:74-90) -> fp64 [n, pe_dim], before the reference's .float().  The reference reads the row sums of A as
    out-degrees (:77), that is, sources on the rows."""
    A = adjacency(src, dst, n)                                       # :76
    D = A.sum(dim=1)                                                 # :77  out degree
    Dinv = 1.0 / (D + 1e-9)                                          # :78
    Dinv[D < 1e-9] = 0                                               # :78  nodes without outgoing edges
    P = (torch.diag(Dinv) @ A).T                                     # :79-80
    One = torch.ones(n, dtype=F64)                                   # :82
    x = One / n                                                      # :83
    PE = []
    alpha = 0.95                                                     # :85
    for _ in range(pe_dim):                                          # :86
        x = alpha * (P @ x) + (1.0 - alpha) / n * One                # :87
        PE.append(x)                                                 # :88
    return torch.stack(PE, dim=-1)                                   # :89


def rw_expansion_sizes(src, dst, n, pe_dim):
    """What the device kernel's `capacity` counts: sizes[i][t] = sum of outdeg(u) over the nodes u with (M^t)[i, u] != 0, t = 0 ..
    pe_dim-1 - the (node, value) pairs node i's row expands to in step t + 1.  All terms are positive: the support is structural."""
    _, out_deg = degrees(src, dst, n)
    A = adjacency(src, dst, n)
    reach = torch.eye(n, dtype=F64)
    sizes = []
    for _ in range(pe_dim):
        sizes.append(((reach > 0).to(torch.int64) * out_deg.unsqueeze(0)).sum(dim=1))
        reach = ((reach @ A) > 0).to(F64)
    return torch.stack(sizes, dim=1).tolist()


def longest_chain(src, dst, n, pe_dim):
    """An upper bound of the additions and multiplications on the longest dependency chain of one entry, for either encoding and
    either side of the comparison: a step adds at most max in-degree terms into a node and multiplies twice on the way."""
    in_deg, _ = degrees(src, dst, n)
    return pe_dim * (int(in_deg.max()) + 3 if n else 3)


# ---- graphs: (src, dst, n) as int lists ------------------------------------------------------------------------------------------------

def triangle():
    return [0, 1, 2], [1, 2, 0], 3


def two_cycle():
    return [0, 1], [1, 0], 2


def self_loop_in_degree_two():
    """node 0 has a self-loop and the edge 1 -> 0: in-degree 2."""
    return [0, 1], [0, 0], 2


def one_edge():
    return [0], [1], 2


def dag():
    return [0, 0, 1, 1, 2, 3], [1, 2, 2, 3, 4, 4], 5


def four_nodes():
    """cycles of length 1, 2 and 3, a parallel edge and unequal in-degrees: the two adjacency conventions differ off the diagonal."""
    return [0, 1, 2, 0, 2, 3, 3, 1], [1, 2, 0, 2, 2, 0, 0, 0], 4


def single_node():
    return [], [], 1


def parallel_two_cycle():
    """0 -> 1 twice, 1 -> 0 once."""
    return [0, 0, 1], [1, 1, 0], 2


def source_and_sink():
    """node 0 has no in-edge, node 3 no out-edge; 1 <-> 2 keeps a cycle."""
    return [0, 0, 1, 2, 2], [1, 2, 2, 1, 3], 4


def mixed_small():
    """a parallel edge, a self-loop, a sink, a source and a 3-cycle in one graph."""
    return [0, 0, 1, 2, 3, 3, 4, 5, 5], [1, 1, 2, 0, 3, 0, 0, 1, 4], 7


def wide_in_lists():
    """node 0 has an in-list of 65, node 1 one of 130 (the wavefront width crossed once and twice), in interleaved edge order;
    the two feed the others back in turn, so that the values differ from step to step."""
    n = 2 + 130
    src, dst = [], []
    for k in range(130):
        src.append(2 + k), dst.append(1)
        if k < 65:
            src.append(2 + 2 * k), dst.append(0)
    for k in range(130):
        src.append(k % 2), dst.append(2 + k)
    return src, dst, n


def random_graph(n, e, seed):
    rng = random.Random(seed)
    return [rng.randrange(n) for _ in range(e)], [rng.randrange(n) for _ in range(e)], n


def hub_three_cycle():
    """hub 0 with in-degree 70: 0 -> 1, 1 -> each of the 70 nodes 2..71, each of those -> 0.  Every node lies on 3-cycles through the
    hub, and the hub's row merges a run of 70 equal ids in its third step."""
    src, dst = [0], [1]
    for k in range(70):
        src += [1, 2 + k]
        dst += [2 + k, 0]
    return src, dst, 72


def banded(reads=200, seed=5):
    """An overlap-like graph of `reads` reads in layout order: node 2r is read r, 2r + 1 its reverse complement; read r overlaps two
    to four of the next five reads on a strand of its own choice, and every edge (u, v) has its mate (v ^ 1, u ^ 1).  400 nodes at
    the default."""
    rng = random.Random(seed)
    src, dst = [], []
    for r in range(reads):
        for off in rng.sample((1, 2, 3, 4, 5), rng.randint(2, 4)):
            t = r + off
            if t >= reads:
                continue
            s = rng.randrange(2)
            u, v = 2 * r + s, 2 * t + s
            src += [u, v ^ 1]
            dst += [v, u ^ 1]
    order = list(range(len(src)))
    rng.shuffle(order)
    return [src[k] for k in order], [dst[k] for k in order], 2 * reads
