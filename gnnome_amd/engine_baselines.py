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

Train mode: `model(graph, x, e)` keeps raising NotImplementedError (its tests pin that); the training step is the explicit entry
train_forward(model, graph, x, e), which trainer.train calls for these models - ONE torch.autograd.Function (_BaselineStep) whose inputs
are the model's parameters, as train._TrainStep is for the symmetric model.  Forward = the eval sequence on the live parameters, plus
SAGEConv's feat_drop: one scaled keep-mask per layer (train.dropout_mask), applied to the layer's input where its ReLU touches the row
(gnnome_relu_mul_rows_f32), so the self and the neighbour path both read the dropped rows.  Kept for the backward: GCN each layer's a and
post-ReLU input, SAGE each layer's table T = h_d | m and mask, the scorer's z1.  Backward, per layer from the last (dY = the gradient of
the layer's product):
    dW, db = dY^T input, column sums of dY                            gnnome_wgrad_f32, gnnome_colsum2_f32
    dIn    = dY W                                                     gnnome_linear_f32
    GCN   dY' = [h > 0] dout'^-1/2 * sum^T(din'^-1/2 dA)              gnnome_node_neighbour_sum_bwd_f32 (csrc/node_neighbour_bwd.hip), one launch
    SAGE  dY' = [h_d > 0] mask * (dT[:, :H] + sum^T(dT[:, H:] / din'))  the same kernel: add = the left half of dT, mult = mask, y = T[:, :H]
the scorer's and the encoders' backward on the symmetric step's kernels.  No atomics anywhere: two steps from equal state leave equal
gradient bits.  A forward whose logits are not all finite left fp16x3's operand range and is run again as bf16x6, like forward_in_range
(one host sync per step; `model.range_check = False` drops it); its backward then runs as bf16x6 too.

Several GPUs: the last section of this file - the same two sequences on one rank of a destination-range partition (dist.PartitionedRunner),
on gnnome_node_neighbour_sum_part_f32 / _bwd_part_f32, under the same autograd.Function: _BaselineStep is handed where the rows live
(train.WholeGraph or dist.PartitionShard) and the sequences of that place, here and in engine_gat.
"""
import contextlib

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
        self.directed = bool(model.directed)   # (read by the partitioned forward, which dist.run_partitioned reaches with the weights alone)
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


def bf16x6_forced(ops):
    """True when the caller has already selected bf16x6 (ops.set_tuning(10, 1)): nothing is left to fall back to, so no forward of this
    module checks its logits then.  A backend that keeps no record of its tuning (a checker) has no such selection."""
    return getattr(ops, "_TUNING", {}).get(10, 0) == 1


def forward_in_range(ops, prep, views, x, e, xd, ed, directed, check=True, run_stack=run_stack):
    """engine_gated.forward_in_range for these stacks (run_stack: this module's, or engine_gat's): a forward whose logits are not all
    finite left fp16x3's operand range and is run again as bf16x6; checked once per set of inputs."""
    if bf16x6_forced(ops):
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


# ---------------------------------------------------------------------------------------------------
# train mode: one autograd.Function over the whole step
# ---------------------------------------------------------------------------------------------------

def _conv_weight(conv, kind):
    """The layer's product weight as ops.linear reads it, [H, K] (prepare_layer's layout) from the live parameters."""
    if kind == "gcn":
        return conv.weight.detach().t().contiguous()
    return torch.cat([conv.fc_self.weight.detach(), conv.fc_neigh.weight.detach()], 1)


def live_encoders(model):
    """The two encoders as ops.encode reads them, from the live parameters -> ((W1, b1, W2, b2) of the node encoder, of the edge encoder)."""
    return tuple(tuple(t.detach().contiguous() for t in (enc.linear1.weight, enc.linear1.bias, enc.linear2.weight, enc.linear2.bias))
                 for enc in (model.node_encoder, model.edge_encoder))


def live_predictor(pred, H):
    """The scorer as its kernels read it, from the live parameters -> (W1, W_nodes [2 hs, H] = W1's src block over its dst block,
    b_nodes = 0 | b1, tail = the five weight arguments of ops.edge_score)."""
    d = lambda t: t.detach().contiguous()  # noqa: E731
    W1 = d(pred.W1.weight)
    W_nodes = torch.cat([W1[:, :H], W1[:, H:2 * H]], 0).contiguous()
    b_nodes = torch.cat([torch.zeros_like(pred.W1.bias), pred.W1.bias]).detach().contiguous()
    return W1, W_nodes, b_nodes, (W1[:, 2 * H:], d(pred.W2.weight), d(pred.W2.bias), d(pred.W3.weight.reshape(-1)), d(pred.W3.bias.reshape(-1)))


def encoders_forward(ops, model, views, x, e_raw):
    """The two encoders on the live parameters -> (h [N,H], e [E,H] in sorted order: what the scorer reads).  Shared with engine_gat's step."""
    enc_node, enc_edge = live_encoders(model)
    h = engine.encode_nodes(ops, views, x, enc_node)
    e = ops.encode(e_raw, *enc_edge, gather=views.srt_eid, rows=views.num_edges)
    return h, e


def score_forward(ops, model, views, h, e):
    """The scorer on the live parameters, keeping z1 -> (logits[E], what score_backward reads).  Shared with engine_gat's step."""
    hs = model.predictor.W1.out_features
    W1, W_nodes, b_nodes, tail = live_predictor(model.predictor, h.shape[1])
    PQ = ops.linear(h, W_nodes, b_nodes)
    z1 = torch.empty((views.num_edges, hs), dtype=torch.float32, device=h.device)
    logits = torch.empty(views.num_edges, dtype=torch.float32, device=h.device)
    ops.edge_score(e, PQ[:, :hs], PQ[:, hs:], views, *tail, logits, z1_out=z1)
    return logits, dict(h=h, e=e, z1=z1, W1=W1, W_nodes=W_nodes)


def score_backward(ops, model, views, kept, dlogits, g):
    """The scorer's backward (score_predictor.py:12-17), as train._TrainStep.backward runs it on one rank: the predictor's gradients into
    g -> (dY = the gradient of the last layer's output [N,H], de = the gradient of the encoded e, which no layer touches)."""
    d = lambda t: t.detach().contiguous()  # noqa: E731
    pred = model.predictor
    N, H = kept["h"].shape
    hs = pred.W1.out_features
    dl = dlogits.reshape(-1).contiguous().float()
    dz1, dz2, u = ops.score_tail_bwd(kept["z1"], dl, views, d(pred.W2.weight), d(pred.W2.bias), d(pred.W3.weight.reshape(-1)))
    g["predictor.W2.weight"] = ops.wgrad(dz2, kept["z1"])
    g["predictor.W2.bias"] = ops.colsum2(dz2)[0]
    g["predictor.W3.weight"] = ops.colsum2(u)[0].reshape(1, 32)
    g["predictor.W3.bias"] = dl.sum().reshape(1)
    W1 = kept["W1"]
    de = ops.linear(dz1, W1[:, 2 * H:].t().contiguous(), None)   # the layers never touch e: this is the edge encoder's gradient
    gW1e = ops.wgrad(dz1, kept["e"])
    dPQ = torch.empty((N, 2 * hs), dtype=torch.float32, device=dl.device)
    ops.segment_sum2(dz1, views, N, out_in=dPQ[:, hs:], out_out=dPQ[:, :hs])   # gathered by srt_dst / srt_src in the forward
    g["predictor.W1.bias"] = ops.colsum2(dPQ[:, hs:].contiguous())[0]
    gWn = ops.wgrad(dPQ, kept["h"])
    g["predictor.W1.weight"] = torch.cat([gWn[:hs], gWn[hs:], gW1e], 1)
    return ops.linear(dPQ, kept["W_nodes"].t().contiguous(), None), de


def encoders_backward(ops, model, views, g, dY, de, x, e_raw):
    """The two encoders' gradients into g (models/full_graph.py:63-64) from dY = d h [N,H] and de = d e [E,H]."""
    from .train import encoder_bwd
    ne, ee = model.node_encoder, model.edge_encoder
    encoder_bwd(ops, g, dY, x, getattr(views, "node_gather", None), views.num_nodes, ne.linear1, ne.linear2, "node_encoder.linear1",
                "node_encoder.linear2")
    encoder_bwd(ops, g, de, e_raw, views.srt_eid, views.num_edges, ee.linear1, ee.linear2, "edge_encoder.linear1", "edge_encoder.linear2")


def draw_masks(model, rows, x):
    """feat_drop's scaled keep-masks [rows, H], one per layer with p > 0 (SAGEConv, GATConv; GraphConv has none: all None), drawn once
    per step: a forward that is run again as bf16x6 drops the same elements.  rows: the step's OWNED node rows - on a shard the owner
    drops its rows before the exchange, so the halo rows arrive dropped."""
    from . import train
    if model.kind == "gcn":
        return [None] * len(model.gnn.convs)
    H = model.node_encoder.linear2.out_features   # (train.dropout_mask is looked up here, at call time: tests substitute known masks)
    return [train.dropout_mask(rows, H, conv.feat_drop.p, x.device) if conv.feat_drop.p > 0 else None for conv in model.gnn.convs]


def _step_forward(ops, model, views, x, e_raw, masks):
    """The train-mode forward on sorted-order e -> (logits[E], what the backward reads)."""
    d = lambda t: t.detach().contiguous()  # noqa: E731
    kind, both, convs = model.kind, not model.directed, model.gnn.convs
    sc = scales_for(views, model.directed)
    h, e = encoders_forward(ops, model, views, x, e_raw)
    N, H = h.shape
    layers = []
    if kind == "gcn":
        for i, conv in enumerate(convs):
            a = ops.node_neighbour_sum(h, views, sscale=sc.dout_rsqrt, dscale=sc.din_rsqrt, both=both)
            layers.append(dict(a=a, y=h if i > 0 else None))   # (y: this layer's input, post-ReLU - the gate of its backward)
            h = ops.linear(a, _conv_weight(conv, kind), d(conv.bias))
            if i + 1 < len(convs):
                ops.relu_rows(h)
    elif len(convs):
        T = torch.empty((N, 2 * H), dtype=torch.float32, device=h.device)
        T[:, :H].copy_(h)
        if masks[0] is not None:
            ops.relu_mul_rows(T[:, :H], masks[0], relu=False)   # the encoder's output has no ReLU
        for i, conv in enumerate(convs):
            ops.node_neighbour_sum(T[:, :H], views, dscale=sc.din_inv, both=both, out=T[:, H:])
            layers.append(dict(T=T, mask=masks[i]))
            if i + 1 == len(convs):
                h = ops.linear(T, _conv_weight(conv, kind), d(conv.bias))
                break
            nxt = torch.empty((N, 2 * H), dtype=torch.float32, device=h.device)   # (every layer's table is kept: no two take turns here)
            ops.linear(T, _conv_weight(conv, kind), d(conv.bias), out=nxt[:, :H])
            if masks[i + 1] is not None:
                ops.relu_mul_rows(nxt[:, :H], masks[i + 1])
            else:
                ops.relu_rows(nxt[:, :H])
            T = nxt
    logits, kept = score_forward(ops, model, views, h, e)
    kept["layers"] = layers
    return logits, kept


def _step_backward(ops, model, views, x, e_raw, kept, dlogits):
    """-> {parameter name: gradient}."""
    d = lambda t: t.detach().contiguous()  # noqa: E731
    kind, both, convs = model.kind, not model.directed, model.gnn.convs
    sc = scales_for(views, model.directed)
    N, H = kept["h"].shape
    g = {}
    dY, de = score_backward(ops, model, views, kept, dlogits, g)
    # ---- layers, last to first (layers/processor.py:42-46, :80-84)
    for i in range(len(convs) - 1, -1, -1):
        conv, s, pfx = convs[i], kept["layers"][i], f"gnn.convs.{i}."
        g[pfx + "bias"] = ops.colsum2(dY)[0]
        if kind == "gcn":
            g[pfx + "weight"] = ops.wgrad(s["a"], dY)              # GraphConv keeps [in, out]
            dA = ops.linear(dY, d(conv.weight), None)              # dY weight^T
            dY = ops.node_neighbour_sum_bwd(dA, views, rscale=sc.din_rsqrt, oscale=sc.dout_rsqrt, both=both, y=s["y"])
        else:
            gW = ops.wgrad(dY, s["T"])                             # [H, 2H] = d fc_self | d fc_neigh
            g[pfx + "fc_self.weight"], g[pfx + "fc_neigh.weight"] = gW[:, :H], gW[:, H:]
            dT = ops.linear(dY, _conv_weight(conv, kind).t().contiguous(), None)
            dY = ops.node_neighbour_sum_bwd(dT[:, H:], views, rscale=sc.din_inv, both=both, add=dT[:, :H], mult=s["mask"],
                                            y=s["T"][:, :H] if i > 0 else None)
        kept["layers"][i] = s = None
    encoders_backward(ops, model, views, g, dY, de, x, e_raw)
    return g


class _BaselineStep(torch.autograd.Function):
    """One training step of GCNModel / SAGEModel / GATModel as ONE autograd node whose inputs are the model's parameters, on a whole graph
    (train.WholeGraph) or on one rank of a destination-range partition (dist.PartitionShard).  `sh` says where the rows live: the backend,
    the owned rows the masks are drawn for, whether the range fallback is decided with the other ranks, how the gradients are summed.
    `step` = (draw, forward, backward) is the model's kernel sequence for that place (_STEP here and in engine_gat; train_forward_on's
    for a shard); the range fallback, the empty graph and the release of the kept activations are the same for all of them."""

    @staticmethod
    def forward(ctx, model, sh, x, e_raw, names, step, *params):
        ops = sh.ops
        draw, fwd, _ = step
        masks = draw(model, sh.n_own, x)
        bf16x6 = bf16x6_forced(ops)
        logits, kept = fwd(ops, model, sh.views, x, e_raw, masks)
        if not bf16x6 and getattr(model, "range_check", True) and _any_rank_not_finite(logits, sh.alone, sh.group):
            bf16x6 = True   # fp16x3's operand range did not hold (forward_in_range): the step runs as bf16x6
            with ops.bf16x6_arithmetic():
                logits, kept = fwd(ops, model, sh.views, x, e_raw, masks)
        ctx.model, ctx.sh, ctx.names, ctx.step, ctx.kept, ctx.inputs, ctx.bf16x6 = model, sh, names, step, kept, (x, e_raw), bf16x6
        return logits.unsqueeze(1)

    @staticmethod
    def backward(ctx, dlogits):
        if ctx.kept is None:
            raise RuntimeError("the activations of this training step were released by its first backward(); "
                               "retain_graph=True is not supported - run the forward again")
        model, sh, bwd = ctx.model, ctx.sh, ctx.step[2]
        if sh.e_own == 0:   # nothing was scored: no parameter has a gradient (a whole graph only: a shard without scored edges is refused)
            grads = [torch.zeros_like(p) for _, p in model.named_parameters()]
        else:
            with sh.ops.bf16x6_arithmetic() if ctx.bf16x6 else contextlib.nullcontext():
                g = bwd(sh.ops, model, sh.views, *ctx.inputs, ctx.kept, dlogits)
            grads = [g[n].contiguous() for n in ctx.names]
        ctx.kept = None
        return (None, None, None, None, None, None) + tuple(sh.sum_ranks(grads))


_STEP = (draw_masks, _step_forward, _step_backward)


def run_train_step(model, graph, x, e, step):
    """What train_forward and engine_gat.train_forward share: the refusals, the views, the inputs on the compute device, the step."""
    from .train import TRAIN_SCORE_HIDDEN, WholeGraph
    device = engine.compute_device(x, e)
    names = [n for n, _ in model.named_parameters()]
    params = [p for _, p in model.named_parameters()]
    if any(p.device != device for p in params):
        raise RuntimeError("training needs the model on the compute device: call model.to(device) first")
    built_width(model.node_encoder.linear2.out_features)
    built_width(model.predictor.W1.out_features, TRAIN_SCORE_HIDDEN, "hidden_edge_scores")
    views = in_edge_views(views_for(graph, device, node_order="input"))
    if x.shape[0] != views.num_nodes or e.shape[0] != views.num_edges:
        raise ValueError(f"x has {x.shape[0]} rows for {views.num_nodes} nodes, e has {e.shape[0]} rows for {views.num_edges} edges")
    xd = x.detach().to(device=device, dtype=torch.float32).contiguous()
    ed = e.detach().to(device=device, dtype=torch.float32).contiguous()
    out = _BaselineStep.apply(model, WholeGraph(views), xd, ed, names, step, *params)
    views.check_range()   # a fresh graph's deferred endpoint check, after the whole forward has been enqueued
    return out


def train_forward(model, graph, x, e):
    """The training step of GCNModel / SAGEModel (the reference's train.py:138-145 runs `model(g, x, e)` in train mode; here that call keeps
    raising and this is the explicit entry, as train.train_forward is the symmetric model's): logits [E,1] on the compute device, with
    autograd history to model.parameters().  `graph` as for the model's call; views of a reversed graph (GraphViews.reversed) are the
    model of the swapped edge list."""
    kind = getattr(model, "kind", None)
    if kind == "gat":
        raise NotImplementedError("the training step of GATModel is engine_gat.train_forward (its edge-softmax backward is another "
                                  "kernel): engine_baselines.train_forward serves GCNModel and SAGEModel")
    if kind not in KINDS:
        raise TypeError(f"engine_baselines.train_forward serves GCNModel and SAGEModel, not {type(model).__name__}")
    return run_train_step(model, graph, x, e, _STEP)


def model_forward(model, graph, x, e, prepared=Prepared, stack=run_stack):
    """models/full_graph.py:65-75 / :109-119 on the MI355X (and, with engine_gat's `prepared` and `stack`, :87-97)."""
    if model.training:
        raise NotImplementedError(f"{type(model).__name__} is built for eval mode only: call .eval() (the training step of the GCN / SAGE / "
                                  "GAT baselines is the explicit entry train_forward of engine_baselines / engine_gat)")
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


# ---------------------------------------------------------------------------------------------------
# destination-range partitions (gnnome_amd/dist.py): one rank's rows of the same two sequences
# ---------------------------------------------------------------------------------------------------
# GCN and SAGE have no normalisation layer and no per-edge activation, so nothing but node rows crosses ranks.  On the DEFAULT partition
# (every edge with an owned end) an owned node's in- and out-list are complete, so with the halo rows of the layer's input fetched (one
# exchange, the symmetric model's) the rank computes its owned rows with the whole graph's association: the neighbour sums are BIT-EQUAL
# to the single-rank run at any world size.  The same holds backward once the halo rows of the incoming gradient are fetched - a
# FORWARD-direction exchange of g, no halo transpose and no partial sums in the convolution stack.  Only the scorer's node gradient
# (halo_bwd) and the parameter gradients (sum_ranks, once, at the end) are summed across ranks.
# The rows split into INTERIOR (no list entry is a halo id: launched while the exchange is in flight) and BOUNDARY (launched after it)
# through the row-list form of the part entries; PARTITION_SPLIT selects that or one unsplit launch after the exchange - equal bits.

# the default of every split= argument below (dist.PartitionedRunner(..., split=)): not measured on two devices yet
# (tools/baseline_partition_time.py), so it is the unsplit launch
PARTITION_SPLIT = False
MAX_EXACT_DEGREE = 1 << 24   # the largest degree of g' accepted: every integer up to 2^24 is a float32, in + out + 1 formed in float32 included


class ShardLists:
    """What the part entries read of a shard: the local in-lists as GraphViews built them (ascending edge id: the whole graph's order) and
    the local out-lists RE-SORTED into the whole graph's order - ascending GLOBAL far-end id, then edge id; GraphViews orders them by
    local id, which puts the halo after the owned nodes."""
    __slots__ = ("num_nodes", "num_edges", "in_ptr", "srt_src", "out_ptr", "out_dst", "transposed")

    def __init__(self, views, node_gid):
        self.num_nodes, self.num_edges, self.transposed = views.num_nodes, views.num_edges, False
        self.in_ptr, self.srt_src, self.out_ptr = views.in_ptr, views.srt_src, views.out_ptr
        counts = (views.out_ptr[1:] - views.out_ptr[:-1]).long()
        owner = torch.repeat_interleave(torch.arange(views.num_nodes, device=counts.device), counts)
        far = node_gid.to(counts.device)[views.out_dst.long()]
        bound = int(node_gid.max()) + 1 if node_gid.numel() else 1
        order = torch.sort(owner * bound + far, stable=True).indices    # (ties - parallel edges - keep their edge-id order)
        self.out_dst = views.out_dst[order].contiguous()


class PartitionPlan:
    """One (partition, directed): the scale vectors of ALL local rows - Scales' formulas on the whole graph's degrees, the halo rows'
    fetched once from their owners -, the lists, and the interior / boundary rows of the forward and of the backward launch."""
    __slots__ = ("lists", "din_rsqrt", "dout_rsqrt", "din_inv", "rows_fwd", "rows_bwd")

    def __init__(self, ops, part, directed, group=None):
        from .dist import HaloExchange
        views, n_own, n_local = part.views, part.n_own, part.n_local
        dev = views.in_ptr.device
        # the owned rows' degrees are complete locally: the partition keeps every edge with an owned end
        deg = torch.zeros((n_local, 4), dtype=torch.float32, device=dev)   # in | out | 0 | 0 (rows of four floats: what gather_rows moves)
        own_in = (views.in_ptr[1:n_own + 1] - views.in_ptr[:n_own])
        own_out = (views.out_ptr[1:n_own + 1] - views.out_ptr[:n_own])
        # the degrees of g' are formed in float32 (here and in Scales): in + 1, out + 1, or in + out + 1 - refused where the largest of them
        # passes 2^24, up to which every integer and every such sum is exact (a halo row's is refused by its owner, which makes the same plan)
        top = 0 if not n_own else int((own_in.long() + own_out.long()).max()) + 1 if not directed else max(int(own_in.max()), int(own_out.max())) + 1
        if top > MAX_EXACT_DEGREE:
            raise ValueError(f"a node of degree {top} in the self-looped{'' if directed else ', doubled'} graph: degrees cross ranks and are "
                             f"summed as float32, exact up to {MAX_EXACT_DEGREE}")
        deg[:n_own, 0], deg[:n_own, 1] = own_in.float(), own_out.float()
        xchg = HaloExchange(part, ops, group)
        xchg.start(deg)
        xchg.finish()
        din, dout = deg[:, 0], deg[:, 1]
        if directed:
            din, dout = din + 1.0, dout + 1.0
        else:
            din = dout = din + dout + 1.0
        self.din_rsqrt, self.dout_rsqrt = din.pow(-0.5).contiguous(), dout.pow(-0.5).contiguous()
        self.din_inv = (1.0 / din).contiguous()
        self.lists = ShardLists(views, part.node_gid)
        halo_in = _rows_with_halo(views.in_ptr, views.srt_src, n_own)
        halo_out = _rows_with_halo(views.out_ptr, views.out_dst, n_own)
        both = not directed
        self.rows_fwd = _split_rows(halo_in | halo_out if both else halo_in)     # the forward walks the in-list (both: and the out-list)
        self.rows_bwd = _split_rows(halo_in | halo_out if both else halo_out)    # the backward the out-list (both: and the in-list)


def _rows_with_halo(ptr, idx, n_own):
    """bool[n_own]: the list of row i names an id >= n_own."""
    hit = torch.cat([torch.zeros(1, dtype=torch.int64, device=idx.device), torch.cumsum((idx >= n_own).long(), 0)])
    p = ptr[:n_own + 1].long()
    return (hit[p[1:]] - hit[p[:-1]]) > 0


def _split_rows(boundary):
    """-> (interior, boundary) int32 row lists, ascending."""
    return torch.nonzero(~boundary).squeeze(1).int().contiguous(), torch.nonzero(boundary).squeeze(1).int().contiguous()


def plan_for(ops, part, directed, group=None):
    """Made once per (partition, directed) - a COLLECTIVE the first time (the halo rows' degrees): every rank calls it at the same place."""
    hit = part._baseline.get(bool(directed))
    if hit is None:
        hit = part._baseline[bool(directed)] = PartitionPlan(ops, part, bool(directed), group)
    return hit


def check_partition(model, part):
    """The refusals of GCNModel / SAGEModel on a partition, before anything is allocated."""
    from .dist import check_shard
    if getattr(part, "in_edges_only", False):
        raise ValueError(f"{type(model).__name__} runs on the default partition, not in_edges_only=True: GraphConv scales every source by its "
                         "OUT-degree and the backward walks the owned nodes' out-lists, which an in-edge-only partition does not hold")
    check_shard(part)
    built_width(model.node_encoder.linear2.out_features)


def _sum_launch(ops, xchg_finish, split, rows, call):
    """The layer's neighbour-sum launch around the end of the halo exchange: interior rows under it and boundary rows after it, or one
    launch after it.  call(rows) launches the part entry for a row list (None: every owned row)."""
    if split and rows[1].numel():
        call(rows[0])
        xchg_finish()
        call(rows[1])
    else:
        xchg_finish()
        call(None)


def _gcn_layer_part(ops, plan, n_own, h, both, split, finish):
    a = torch.empty((n_own, h.shape[1]), dtype=torch.float32, device=h.device)
    _sum_launch(ops, finish, split, plan.rows_fwd, lambda rows: ops.node_neighbour_sum_part(
        h, plan.lists, n_own, sscale=plan.dout_rsqrt, dscale=plan.din_rsqrt, both=both, out=a, rows=rows))
    return a


def _sage_layer_part(ops, plan, n_own, T, both, split, finish):
    H = T.shape[1] // 2
    _sum_launch(ops, finish, split, plan.rows_fwd, lambda rows: ops.node_neighbour_sum_part(
        T[:, :H], plan.lists, n_own, dscale=plan.din_inv, both=both, out=T[:, H:], rows=rows))


def score_part(ops, part, group, e, h, pw_nodes, w_tail, z1_out=None):
    """The symmetric model's scorer on the owned in-edges (engine.score_tail, after the node halves' product): h [n_local,H] with its halo
    rows fetched, e the encoded scored rows -> logits[E_global] in edge-id order, complete on every rank.  GATModel's sequences end here too."""
    W_nodes, b_nodes, planes = pw_nodes
    hs = W_nodes.shape[0] // 2
    PQ = ops.linear(h, W_nodes, b_nodes, planes=planes)
    sc = part.scored
    return engine.score_tail(ops, engine.scored_rows(ops, e, sc.rows, sc.count), PQ[:, :hs], PQ[:, hs:], w_tail, sc.score_views,
                             sc.count, sc.total, z1_out=z1_out, **part.logits_finish(group))


def run_partitioned(ops, prep, part, x_local, e_local, group=None, directed=None, split=None):
    """run_stack on one rank: x_local [n_local,F] (owned, then halo), e_local [e_local,F] in local edge-id order -> logits[E_global].
    Per layer: the halo rows of the layer's input (layer 0's come straight from x), the neighbour sum over the owned rows, the product
    and the ReLU on the owned rows; one more exchange of the last h, then the scorer on the owned in-edges."""
    from .dist import HaloExchange
    split = PARTITION_SPLIT if split is None else split
    directed = prep.directed if directed is None else bool(directed)
    if getattr(part, "in_edges_only", False):
        raise ValueError("GCNModel / SAGEModel run on the default partition, not in_edges_only=True (the sources' out-degrees and the owned "
                         "nodes' out-lists are not there)")
    views, n_own, n_local, H = part.views, part.n_own, part.n_local, prep.hidden
    plan = plan_for(ops, part, directed, group)
    both = not directed
    xchg = HaloExchange(part, ops, group)
    h = ops.encode(x_local, *prep.enc_node)
    e = ops.encode(e_local, *prep.enc_edge, gather=views.srt_eid[:part.n_score], rows=part.n_score)   # the scored rows, sorted order
    L = len(prep.layers)
    new = lambda cols: torch.empty((n_local, cols), dtype=torch.float32, device=h.device)  # noqa: E731
    if prep.kind == "gcn":
        for i, lw in enumerate(prep.layers):
            if i > 0:
                xchg.start(h)
            a = _gcn_layer_part(ops, plan, n_own, h, both, split, xchg.finish)
            h = new(H)
            ops.linear(a, lw.W, lw.bias, out=h[:n_own], planes=lw.planes)
            if i + 1 < L:
                ops.relu_rows(h[:n_own])
    elif L:
        tables = [new(2 * H) for _ in range(min(L, 2))]
        tables[0][:, :H].copy_(h)
        for i, lw in enumerate(prep.layers):
            T = tables[i % 2]
            if i > 0:
                xchg.start(T[:, :H])
            _sage_layer_part(ops, plan, n_own, T, both, split, xchg.finish)
            if i + 1 == L:
                h = new(H)
                ops.linear(T[:n_own], lw.W, lw.bias, out=h[:n_own], planes=lw.planes)
                break
            nxt = tables[(i + 1) % 2]
            ops.linear(T[:n_own], lw.W, lw.bias, out=nxt[:n_own, :H], planes=lw.planes)
            ops.relu_rows(nxt[:n_own, :H])
    if L:
        xchg.start(h)
        xchg.finish()
    pw = prep.predictor
    return score_part(ops, part, group, e, h, (pw["W_nodes"], pw["b_nodes"], pw.get("planes")), engine.tail_weights(pw))


def _any_rank_not_finite(logits, alone, group):
    """True on every rank when the logits of one are not all finite: the fp16x3 -> bf16x6 decision must not differ between ranks.
    alone (train.WholeGraph, dist._alone): this process's flag, read once; otherwise the all-reduced flag."""
    from .dist import all_reduce_sum
    finite = torch.isfinite(logits).all()
    if alone:
        return not bool(finite)
    return bool(all_reduce_sum((~finite).reshape(1).to(torch.float32), group) > 0)


def forward_partitioned(ops, model, prep, part, x_local, e_local, group, run):
    """forward_in_range on a partition, for run = this module's run_partitioned (with its split= bound) or engine_gat's: logits that are
    not all finite left fp16x3's operand range and the forward is run again as bf16x6 - decided on the all-reduced flag, so every rank
    takes the same route; checked on every call (no cache: the inputs are the runner's)."""
    from .dist import _alone
    directed = bool(model.directed)
    if prep.force_bf16x6:
        with ops.bf16x6_arithmetic():
            return run(ops, prep, part, x_local, e_local, group, directed)
    logits = run(ops, prep, part, x_local, e_local, group, directed)
    if bf16x6_forced(ops) or not getattr(model, "range_check", True):
        return logits
    if not _any_rank_not_finite(logits, _alone(part.world), group):
        return logits
    with ops.bf16x6_arithmetic():
        return run(ops, prep, part, x_local, e_local, group, directed)


def encoders_backward_on_shard(ops, model, sh, g, dY, de, x, e_raw):
    """encoders_backward on a shard (models/full_graph.py:63-64): every node row's gradient is complete at its owner, every scored edge's
    at its scorer."""
    from .train import encoder_bwd
    ne, ee = model.node_encoder, model.edge_encoder
    encoder_bwd(ops, g, dY.contiguous(), x[:sh.n_own], None, sh.n_own, ne.linear1, ne.linear2, "node_encoder.linear1", "node_encoder.linear2")
    encoder_bwd(ops, g, de, e_raw, sh.views.srt_eid[:sh.e_own], sh.e_own, ee.linear1, ee.linear2, "edge_encoder.linear1", "edge_encoder.linear2")


def check_step_on(model, shard, x_local, e_local):
    """What every train_forward_on refuses once its check_partition has passed -> (names, params) of the model's parameters."""
    from .train import TRAIN_SCORE_HIDDEN
    built_width(model.predictor.W1.out_features, TRAIN_SCORE_HIDDEN, "hidden_edge_scores")
    names, params = zip(*model.named_parameters())
    if any(p.device != x_local.device for p in params):
        raise RuntimeError("training needs the model on the compute device: call model.to(device) first")
    if x_local.shape[0] != shard.n_local or e_local.shape[0] != shard.e_local:
        raise ValueError(f"x has {x_local.shape[0]} rows for {shard.n_local} local nodes, e has {e_local.shape[0]} rows for {shard.e_local} local edges")
    return list(names), params


def _part_step_forward(ops, model, sh, x, e_raw, masks, split):
    """_step_forward on a shard -> (logits[E_global], what the backward reads).  Owned rows: the products, the ReLU, the masks; all local
    rows: the layer inputs the neighbour sum gathers from."""
    d = lambda t: t.detach().contiguous()  # noqa: E731
    part, views, n_own, n_local = sh.part, sh.views, sh.n_own, sh.n_local
    kind, both, convs = model.kind, not model.directed, model.gnn.convs
    plan = plan_for(ops, part, model.directed, sh.group)
    enc_node, enc_edge = live_encoders(model)
    h = ops.encode(x, *enc_node)
    e = ops.encode(e_raw, *enc_edge, gather=views.srt_eid[:sh.e_own], rows=sh.e_own)
    H, L = h.shape[1], len(convs)
    new = lambda cols: torch.empty((n_local, cols), dtype=torch.float32, device=h.device)  # noqa: E731
    layers = []
    if kind == "gcn":
        for i, conv in enumerate(convs):
            if i > 0:
                sh.halo_start(h)
            a = _gcn_layer_part(ops, plan, n_own, h, both, split, sh.halo_finish)
            layers.append(dict(a=a, y=h if i > 0 else None))
            h = new(H)
            ops.linear(a, _conv_weight(conv, kind), d(conv.bias), out=h[:n_own])
            if i + 1 < L:
                ops.relu_rows(h[:n_own])
    elif L:
        T = new(2 * H)
        T[:, :H].copy_(h)
        if masks[0] is not None:
            ops.relu_mul_rows(T[:n_own, :H], masks[0], relu=False)
        for i, conv in enumerate(convs):
            if i > 0 or masks[0] is not None:   # (a dropped layer-0 input: the halo rows are the OWNERS' dropped rows, not what x encodes to)
                sh.halo_start(T[:, :H])
            _sage_layer_part(ops, plan, n_own, T, both, split, sh.halo_finish)
            layers.append(dict(T=T, mask=masks[i]))
            if i + 1 == L:
                h = new(H)
                ops.linear(T[:n_own], _conv_weight(conv, kind), d(conv.bias), out=h[:n_own])
                break
            nxt = new(2 * H)
            ops.linear(T[:n_own], _conv_weight(conv, kind), d(conv.bias), out=nxt[:n_own, :H])
            if masks[i + 1] is not None:
                ops.relu_mul_rows(nxt[:n_own, :H], masks[i + 1])
            else:
                ops.relu_rows(nxt[:n_own, :H])
            T = nxt
    if L:
        sh.halo_start(h)
        sh.halo_finish()
    W1, W_nodes, b_nodes, tail = live_predictor(model.predictor, H)
    z1 = torch.empty((sh.e_own, model.predictor.W1.out_features), dtype=torch.float32, device=h.device)
    logits = score_part(ops, part, sh.group, e, h, (W_nodes, b_nodes, None), tail, z1_out=z1)
    return logits, dict(h=h, e=e, z1=z1, W1=W1, W_nodes=W_nodes, layers=layers)


def _part_step_backward(ops, model, sh, x, e_raw, kept, dlogits, split):
    """_step_backward on a shard -> {parameter name: this rank's share of the gradient}.  Per layer dW, db and dIn = dY W on the owned
    rows, then the halo rows of the gradient table are FETCHED (the forward's exchange, on g) and the backward kernel runs over the owned
    rows: every owned row's dY' is complete and has the single-rank run's association.  Only the scorer's node gradient returns partial
    rows to their owners (halo_bwd)."""
    from .train import score_backward_on_shard
    d = lambda t: t.detach().contiguous()  # noqa: E731
    part, n_own, n_local, e_own = sh.part, sh.n_own, sh.n_local, sh.e_own
    kind, both, convs = model.kind, not model.directed, model.gnn.convs
    plan = plan_for(ops, part, model.directed, sh.group)
    pred = model.predictor
    H = kept["h"].shape[1]
    dev = dlogits.device
    g = {}
    # ---- scorer: train._TrainStep.backward's, on the e_own encoded rows (the layers never touch e); dh's halo rows are partial sums
    dh, de = score_backward_on_shard(ops, pred, sh, g, dlogits, kept["z1"], kept["e"], kept["h"], kept["W1"], kept["W_nodes"], e_own)
    sh.halo_bwd(dh)
    dY = dh[:n_own]
    # ---- layers, last to first (layers/processor.py:42-46, :80-84)
    for i in range(len(convs) - 1, -1, -1):
        conv, s, pfx = convs[i], kept["layers"][i], f"gnn.convs.{i}."
        g[pfx + "bias"] = ops.colsum2(dY)[0]
        out = torch.empty((n_own, H), dtype=torch.float32, device=dev)
        if kind == "gcn":
            g[pfx + "weight"] = ops.wgrad(s["a"], dY)
            dA = torch.empty((n_local, H), dtype=torch.float32, device=dev)
            ops.linear(dY, d(conv.weight), None, out=dA[:n_own])
            sh.halo_start(dA)
            _sum_launch(ops, sh.halo_finish, split, plan.rows_bwd, lambda rows: ops.node_neighbour_sum_bwd_part(
                dA, plan.lists, n_own, rscale=plan.din_rsqrt, oscale=plan.dout_rsqrt, both=both, y=s["y"], out=out, rows=rows))
        else:
            gW = ops.wgrad(dY, s["T"][:n_own])
            g[pfx + "fc_self.weight"], g[pfx + "fc_neigh.weight"] = gW[:, :H], gW[:, H:]
            dT = torch.empty((n_local, 2 * H), dtype=torch.float32, device=dev)
            ops.linear(dY, _conv_weight(conv, kind).t().contiguous(), None, out=dT[:n_own])
            sh.halo_start(dT[:, H:])
            _sum_launch(ops, sh.halo_finish, split, plan.rows_bwd, lambda rows: ops.node_neighbour_sum_bwd_part(
                dT[:, H:], plan.lists, n_own, rscale=plan.din_inv, both=both, add=dT[:, :H], mult=s["mask"],
                y=s["T"][:, :H] if i > 0 else None, out=out, rows=rows))
        dY = out
        kept["layers"][i] = s = None
    encoders_backward_on_shard(ops, model, sh, g, dY, de, x, e_raw)
    return g


def train_forward_on(model, shard, x_local, e_local, split=None):
    """The training step of GCNModel / SAGEModel over one rank's rows (dist.PartitionShard over the default partition): x_local / e_local
    are the input features of the shard's nodes (owned, then halo) and edges (local edge-id order).  Returns logits[E_global, 1], complete
    on every rank; after backward() every rank holds the whole graph's parameter gradients."""
    if getattr(model, "kind", None) not in KINDS:
        raise TypeError(f"engine_baselines.train_forward_on serves GCNModel and SAGEModel, not {type(model).__name__}")
    check_partition(model, shard.part)
    names, params = check_step_on(model, shard, x_local, e_local)
    split = PARTITION_SPLIT if split is None else bool(split)
    step = (draw_masks,   # (the shell hands the sequences shard.views; they read the shard itself)
            lambda ops, model, views, *rest: _part_step_forward(ops, model, shard, *rest, split),
            lambda ops, model, views, *rest: _part_step_backward(ops, model, shard, *rest, split))
    return _BaselineStep.apply(model, shard, x_local, e_local, names, step, *params)
