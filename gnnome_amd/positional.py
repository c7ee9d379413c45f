"""Positional encodings on the device: the nb_pos_enc > 0 half of the reference's add_positional_encoding (utils/data_utils.py:44-92),
which its dataset class runs on every loaded graph after preprocess_graph (graph_dataset.py:50-52).

    pe = positional_encoding(graph, 8, "RW")                     # [N, 8] float32: diag((A D^-1)^t), t = 1..8
    pe = positional_encoding(graph, 8, "PR")                     # [N, 8] float32: the k-step PageRank features
    g = add_positional_encoding(g, nb_pos_enc=8, type_pos_enc="PR")   # the reference's call on a graph dict: in_deg, out_deg, pe

The reference marks the block obsolete and ships nb_pos_enc = 0; its models never read ndata['pe'] (node_features = 2), and neither do
this package's.  The kernels (csrc/positional.hip) hold one node's neighbourhood at a time, where the reference multiplies whole scipy
matrices that fill in with every power.  tests/positional_statement.py is the dense torch restatement the results are checked against."""
import logging

import torch

from . import features, ops
from .graph import views_for

PE_TYPES = ("RW", "PR")
_log = logging.getLogger(__name__)
_warned = set()


def _unknown_type(pe_type):
    """The reference's two `if pe_type == ...` fall through for any other value and no pe is set (data_utils.py:59,74); said once per value."""
    if pe_type not in _warned:
        _warned.add(pe_type)
        _log.warning("type_pos_enc=%r is neither 'RW' nor 'PR': no positional encoding is computed, as in the reference", pe_type)


def _views_on(graph, device):
    device = device or (graph.device if isinstance(graph, ops.GraphViews) else torch.device("cuda", torch.cuda.current_device()))
    views = graph if isinstance(graph, ops.GraphViews) else views_for(graph, device)
    views.check_range()
    return views


def _encode(graph, pe_dim, pe_type, device, dtype, capacity):
    views = _views_on(graph, device)
    if pe_type == "PR":
        return ops.pagerank_steps(views, pe_dim, dtype)
    return ops.rw_return(views, pe_dim, dtype, capacity)


def positional_encoding(graph, pe_dim, pe_type, device=None, dtype=torch.float32, capacity=None):
    """g.ndata['pe'] of utils/data_utils.py:53-90 -> [N, pe_dim] on the device, or None where the reference sets nothing: pe_dim == 0
    (it returns before touching pe, :56-57) and a pe_type other than 'RW' / 'PR' (logged once).
    graph: (src, dst, N), an object with edges() / num_nodes(), or GraphViews.  dtype: float32 (the reference's .float()) or float64
    (the table before that one cast).  capacity ('RW' only): the (node, value) pairs one step of a node's row may expand to, default
    ops.RW_DEFAULT_CAPACITY; a row that outgrows it raises RuntimeError naming the first such node, the size it needed and this
    keyword, before anything is returned."""
    pe_dim = int(pe_dim)
    if pe_dim == 0:
        return None
    if pe_dim < 0:
        raise ValueError(f"pe_dim={pe_dim} is negative")
    if pe_type not in PE_TYPES:
        _unknown_type(pe_type)
        return None
    return _encode(graph, pe_dim, pe_type, device, dtype, capacity)


def add_positional_encoding(g, nb_pos_enc=0, type_pos_enc="none", device=None):
    """utils/data_utils.py:44-92 on a graph dict (src, dst, num_nodes, ...; gfa.read_gfa / trainer.process): sets g['in_deg'] and
    g['out_deg'] (float32[N], :50-51) and, when nb_pos_enc > 0 and type_pos_enc is 'RW' or 'PR', g['pe'] (float32[N, nb_pos_enc]); the
    tensors stay on the device.  Returns g."""
    views = _views_on((g["src"], g["dst"], int(g["num_nodes"])), device)   # built once, for the degrees and the encoding
    g["in_deg"], g["out_deg"] = features.stored_degrees(views, device=device)
    pe = positional_encoding(views, nb_pos_enc, type_pos_enc, device=device)
    if pe is not None:
        g["pe"] = pe
    return g
