"""CHECKER backend for GCNModel / SAGEModel: tests/cpu_ops.py plus a torch-CPU statement of the neighbour-sum entries
(include/gnnome_hip.h: gnnome_node_neighbour_sum_f32, _bwd_f32, their partition forms _part_f32 / _bwd_part_f32, gnnome_relu_rows_f32,
gnnome_relu_mul_rows_f32).

Test infrastructure only: it lets the host logic of the partitioned baselines (gnnome_amd/dist.py, engine_baselines' partition section) run
on CPU ranks over gloo.  The sums here are index_add sums: the CONTRACT of the entries (which rows are read, which are written), not their
association - bit equality with the whole-graph entry is a property of the kernels and is tested on the device."""
import contextlib
import types

import torch

import cpu_ops


class Views(cpu_ops.CpuViews):
    """CpuViews with the cache engine_baselines.scales_for keeps its scale vectors in."""

    def __init__(self, src, dst, num_nodes):
        super().__init__(src, dst, num_nodes)
        self._derived = {}


def _list_sum(t, ptr, idx, rows):
    """sum over the list entries of rows 0 .. rows of t[entry]."""
    p = ptr[:rows + 1].long()
    owner = torch.repeat_interleave(torch.arange(rows), p[1:] - p[:-1])
    entries = idx[int(p[0]):int(p[-1])].long() if rows else idx[:0].long()
    return torch.zeros((rows, t.shape[1]), dtype=t.dtype).index_add(0, owner, t[entries])


def _rows_of(rows, n_own):
    return torch.arange(n_own) if rows is None else rows.long()


def node_neighbour_sum_part(h, views, n_own, sscale=None, dscale=None, both=False, out=None, rows=None):
    n_own = int(n_own)
    assert h.shape[0] == views.num_nodes and 0 <= n_own <= h.shape[0] and not views.transposed
    assert sscale is None or sscale.numel() >= h.shape[0]
    t = h if sscale is None else h * sscale[:h.shape[0], None]
    s = t[:n_own] + _list_sum(t, views.in_ptr, views.srt_src, n_own)
    if both:
        s = s + _list_sum(t, views.out_ptr, views.out_dst, n_own)
    if dscale is not None:
        s = s * dscale[:n_own, None]
    if out is None:
        out = torch.full((n_own, h.shape[1]), float("nan"), dtype=h.dtype)   # rows that are not listed are not written
    r = _rows_of(rows, n_own)
    assert r.numel() == 0 or (int(r.min()) >= 0 and int(r.max()) < n_own and torch.unique(r).numel() == r.numel())
    out[r] = s[r]
    return out


def node_neighbour_sum(h, views, sscale=None, dscale=None, both=False, out=None):
    assert not views.transposed
    if out is None:
        out = torch.empty_like(h)
    return node_neighbour_sum_part(h, views, views.num_nodes, sscale, dscale, both, out)


def node_neighbour_sum_bwd_part(g, views, n_own, rscale=None, oscale=None, both=False, add=None, y=None, mult=None, out=None, rows=None):
    n_own = int(n_own)
    assert g.shape[0] == views.num_nodes and 0 <= n_own <= g.shape[0] and not views.transposed
    assert rscale is None or rscale.numel() >= g.shape[0]
    t = g if rscale is None else g * rscale[:g.shape[0], None]
    v = t[:n_own] + _list_sum(t, views.out_ptr, views.out_dst, n_own)
    if both:
        v = v + _list_sum(t, views.in_ptr, views.srt_src, n_own)
    if oscale is not None:
        v = v * oscale[:n_own, None]
    if add is not None:
        v = add[:n_own] + v
    if mult is not None:
        v = v * mult[:n_own]
    if y is not None:
        v = torch.where(y[:n_own] > 0, v, torch.zeros_like(v))
    if out is None:
        out = torch.full((n_own, g.shape[1]), float("nan"), dtype=g.dtype)
    r = _rows_of(rows, n_own)
    out[r] = v[r]
    return out


def node_neighbour_sum_bwd(g, views, rscale=None, oscale=None, both=False, add=None, y=None, mult=None, out=None):
    if out is None:
        out = torch.empty_like(g)
    return node_neighbour_sum_bwd_part(g, views, views.num_nodes, rscale, oscale, both, add, y, mult, out)


def relu_rows(x):
    x.copy_(torch.relu(x))
    return x


def relu_mul_rows(x, mult, relu=True):
    x.copy_((torch.relu(x) if relu else x) * mult)
    return x


@contextlib.contextmanager
def bf16x6_arithmetic():
    yield


BACKEND = types.SimpleNamespace(**{k: v for k, v in vars(cpu_ops).items() if not k.startswith("_") and k != "GraphViews"},
                                GraphViews=Views, node_neighbour_sum=node_neighbour_sum, node_neighbour_sum_part=node_neighbour_sum_part,
                                node_neighbour_sum_bwd=node_neighbour_sum_bwd, node_neighbour_sum_bwd_part=node_neighbour_sum_bwd_part,
                                relu_rows=relu_rows, relu_mul_rows=relu_mul_rows, bf16x6_arithmetic=bf16x6_arithmetic, _TUNING={})
