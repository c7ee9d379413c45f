"""Host logic of the two sum / mean baselines, GCNModel (models/full_graph.py:56-75, layers/processor.py:35-46) and SAGEModel
(full_graph.py:100-119, processor.py:73-84): weight preparation and kernel sequences, beside engine.py and engine_gated.py.

Both run their convolutions on g' = add_self_loop(g) (directed=True) or add_self_loop(add_reverse_edges(g)) (directed=False) and
score the ORIGINAL graph with the encoded e, which no layer touches.  g' is never built: a node's neighbours in g' are its in-list,
itself, and (directed=False) its out-list, all of which GraphViews already holds.  Eval mode, per layer (N nodes, H hidden):
    GCN   a  = din'^-1/2 * sum_{j in N'(i)} dout'[j]^-1/2 h[j]       gnnome_node_neighbour_sum_f32 (csrc/node_neighbour.hip)
          h' = a weight + bias                                        gnnome_linear_planes_f32 / gnnome_linear_f32 on weight^T
    SAGE  m  = 1/din' * sum_{j in N'(i)} h[j]                         the same kernel, writing the right half of a [N,2H] table T = h | m
          h' = T [fc_self | fc_neigh]^T + bias                        one product over the table
a ReLU (gnnome_relu_rows_f32, in place) after every layer but the last, then the symmetric model's scorer.
Degrees in g': directed=True din' = in + 1, dout' = out + 1; directed=False din' = dout' = in + out + 1 - never zero.  The three scale
vectors are made once per (graph, directed) from in_ptr / out_ptr differences and kept with the views (GraphViews._derived).
Train mode is not built: the models raise NotImplementedError.
"""
import torch

from . import engine
from . import ops as hip_ops
from .engine_gated import in_edge_views
from .graph import views_for

KINDS = ("gcn", "sage")


def built_width(width, built=engine.BUILT_HIDDEN, what="hidden_features"):
    """The baselines run at the built widths only (zero-padding is not served for them)."""
    if width not in built:
        raise ValueError(f"{what}={width}: GCNModel / SAGEModel / GATModel are built for {what} in {tuple(built)}")
    return width


class Scales:
    """The per-node scale vectors of one (graph, directed): din'^-1/2, dout'^-1/2 (GraphConv norm='both') and 1/din' (SAGEConv 'mean')."""
    __slots__ = ("din_rsqrt", "dout_rsqrt", "din_inv")

    def __init__(self, views, directed):
        din = (views.in_ptr[1:] - views.in_ptr[:-1]).to(torch.float32)
        dout = (views.out_ptr[1:] - views.out_ptr[:-1]).to(torch.float32)
        if directed:
            din, dout = din + 1.0, dout + 1.0
        else:
            din = dout = din + dout + 1.0
        self.din_rsqrt, self.dout_rsqrt = din.pow(-0.5).contiguous(), dout.pow(-0.5).contiguous()
        self.din_inv = (1.0 / din).contiguous()


def scales_for(views, directed):
    """(views: not transposed - run_stack hands in in_edge_views' result)"""
    key = ("baseline_scales", bool(directed))
    hit = views._derived.get(key)
    if hit is None:
        hit = views._derived[key] = Scales(views, bool(directed))
    return hit


class BaselineLayer:
    """One convolution as the dense product reads it: W[H, K] row-major (K = H for GCN, 2H for SAGE), bias[H], W's fp16x3 planes or None."""
    __slots__ = ("W", "bias", "planes")


def prepare_layer(conv, kind, device):
    def dev(t):
        return t.detach().to(device=device, dtype=torch.float32).contiguous()

    lw = BaselineLayer()
    if kind == "gcn":
        lw.W = dev(conv.weight.t())                                        # GraphConv keeps [in, out]; the product wants [out, in]
    else:
        lw.W = dev(torch.cat([conv.fc_self.weight, conv.fc_neigh.weight], 1))   # [H, 2H] on the table h | m
    lw.bias = dev(conv.bias)
    hidden, K = lw.W.shape
    built_width(hidden)
    lw.planes = hip_ops.weight_planes(lw.W) if hip_ops.planes_supported(K, hidden) and lw.W.is_cuda else None
    return lw


class Prepared:
    """Device-resident, kernel-ready copies of a GCNModel's / SAGEModel's parameters (eval semantics)."""

    def __init__(self, model, device):
        def dev(t):
            return t.detach().to(device=device, dtype=torch.float32).contiguous()

        self.device, self.kind = device, model.kind
        assert self.kind in KINDS
        self.hidden = built_width(model.node_encoder.linear2.out_features)
        self.enc_node = tuple(dev(t) for t in (model.node_encoder.linear1.weight, model.node_encoder.linear1.bias,
                                               model.node_encoder.linear2.weight, model.node_encoder.linear2.bias))
        self.enc_edge = tuple(dev(t) for t in (model.edge_encoder.linear1.weight, model.edge_encoder.linear1.bias,
                                               model.edge_encoder.linear2.weight, model.edge_encoder.linear2.bias))
        self.layers = [prepare_layer(conv, self.kind, device) for conv in model.gnn.convs]
        self.predictor = engine.prepare_predictor(model.predictor, device)
        weights = [lw.W for lw in self.layers] + [self.predictor["_W1"], self.predictor["W2"]]
        amax = max((float(t.abs().max()) if t.numel() else 0.0) for t in weights)
        self.force_bf16x6 = not (amax < engine.hip_ops_fp16_max())   # fp16x3's operand range, checked once for the weights
        self.range_verified = self.range_failed = None


# ---------------------------------------------------------------------------------------------------
# kernel sequences (ops = gnnome_amd.ops)
# ---------------------------------------------------------------------------------------------------

def gcn_stack(ops, layers, views, sc, h, both):
    """processor.py:42-46 on g'."""
    for i, lw in enumerate(layers):
        a = ops.node_neighbour_sum(h, views, sscale=sc.dout_rsqrt, dscale=sc.din_rsqrt, both=both)
        h = ops.linear(a, lw.W, lw.bias, planes=lw.planes)
        if i + 1 < len(layers):
            ops.relu_rows(h)
    return h


def sage_stack(ops, layers, views, sc, h, both):
    """processor.py:80-84 on g': two [N,2H] tables h | m take turns, the product of one layer writes the left half of the other."""
    if not layers:
        return h
    N, H = h.shape
    tables = [torch.empty((N, 2 * H), dtype=torch.float32, device=h.device) for _ in range(min(len(layers), 2))]
    tables[0][:, :H].copy_(h)
    for i, lw in enumerate(layers):
        T = tables[i % 2]
        ops.node_neighbour_sum(T[:, :H], views, dscale=sc.din_inv, both=both, out=T[:, H:])
        if i + 1 == len(layers):
            return ops.linear(T, lw.W, lw.bias, planes=lw.planes)
        nxt = tables[(i + 1) % 2][:, :H]
        ops.linear(T, lw.W, lw.bias, out=nxt, planes=lw.planes)
        ops.relu_rows(nxt)


def run_stack(ops, prep, views, x, e_raw, directed=True):
    """Encoders -> L convolutions on g' -> scorer on g; logits[E] at the original edge ids."""
    views = in_edge_views(views)
    h = engine.encode_nodes(ops, views, x, prep.enc_node)
    e = ops.encode(e_raw, *prep.enc_edge, gather=views.srt_eid, rows=views.num_edges)   # sorted order: what the scorer reads
    stack = gcn_stack if prep.kind == "gcn" else sage_stack
    h = stack(ops, prep.layers, views, scales_for(views, directed), h, not directed)
    logits = torch.empty(views.num_edges, dtype=torch.float32, device=h.device)
    engine.score_step(ops, prep.predictor, views, h, e, logits)
    return logits


def forward_in_range(ops, prep, views, x, e, xd, ed, directed, check=True, run_stack=run_stack):
    """engine_gated.forward_in_range for these stacks (run_stack: this module's, or engine_gat's): a forward whose logits are not all
    finite left fp16x3's operand range and is run again as bf16x6; checked once per set of inputs."""
    if ops._TUNING.get(10, 0) == 1:
        return run_stack(ops, prep, views, xd, ed, directed)
    if prep.force_bf16x6 or engine._same_inputs(prep.range_failed, views, x, e):
        with ops.bf16x6_arithmetic():
            return run_stack(ops, prep, views, xd, ed, directed)
    logits = run_stack(ops, prep, views, xd, ed, directed)
    if not check or engine._same_inputs(prep.range_verified, views, x, e):
        return logits
    if bool(torch.isfinite(logits).all()):
        prep.range_verified = engine._inputs_key(views, x, e)
        return logits
    prep.range_failed = engine._inputs_key(views, x, e)
    with ops.bf16x6_arithmetic():
        return run_stack(ops, prep, views, xd, ed, directed)


def model_forward(model, graph, x, e, prepared=Prepared, stack=run_stack):
    """models/full_graph.py:65-75 / :109-119 on the MI355X (and, with engine_gat's `prepared` and `stack`, :87-97)."""
    if model.training:
        raise NotImplementedError(f"{type(model).__name__} is built for eval mode only: call .eval() (train mode of the GCN / SAGE / GAT "
                                  "baselines is not served)")
    out_device = x.device
    device = engine.compute_device(x, e)
    prep = engine.prepared_for(model, device, prepared)
    views = views_for(graph, device, node_order="input")
    if x.shape[0] != views.num_nodes or e.shape[0] != views.num_edges:
        raise ValueError(f"x has {x.shape[0]} rows for {views.num_nodes} nodes, e has {e.shape[0]} rows for {views.num_edges} edges")
    with torch.no_grad():
        xd = x.detach().to(device=device, dtype=torch.float32).contiguous()
        ed = e.detach().to(device=device, dtype=torch.float32).contiguous()
        logits = forward_in_range(hip_ops, prep, views, x, e, xd, ed, bool(model.directed), check=getattr(model, "range_check", True),
                                  run_stack=stack)
    views.check_range()   # a fresh graph's deferred endpoint check, after the whole forward has been enqueued
    return logits.unsqueeze(1).to(out_device)
