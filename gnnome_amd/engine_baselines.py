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


# ---------------------------------------------------------------------------------------------------
# train mode: one autograd.Function over the whole step
# ---------------------------------------------------------------------------------------------------

def _conv_weight(conv, kind):
    """The layer's product weight as ops.linear reads it, [H, K] (prepare_layer's layout) from the live parameters."""
    if kind == "gcn":
        return conv.weight.detach().t().contiguous()
    return torch.cat([conv.fc_self.weight.detach(), conv.fc_neigh.weight.detach()], 1)


def encoders_forward(ops, model, views, x, e_raw):
    """The two encoders on the live parameters -> (h [N,H], e [E,H] in sorted order: what the scorer reads).  Shared with engine_gat's step."""
    d = lambda t: t.detach().contiguous()  # noqa: E731
    ne, ee = model.node_encoder, model.edge_encoder
    h = engine.encode_nodes(ops, views, x, (d(ne.linear1.weight), d(ne.linear1.bias), d(ne.linear2.weight), d(ne.linear2.bias)))
    e = ops.encode(e_raw, d(ee.linear1.weight), d(ee.linear1.bias), d(ee.linear2.weight), d(ee.linear2.bias), gather=views.srt_eid,
                   rows=views.num_edges)
    return h, e


def score_forward(ops, model, views, h, e):
    """The scorer on the live parameters, keeping z1 -> (logits[E], what score_backward reads).  Shared with engine_gat's step."""
    d = lambda t: t.detach().contiguous()  # noqa: E731
    H = h.shape[1]
    pred = model.predictor
    hs = pred.W1.out_features
    W1 = d(pred.W1.weight)
    W_nodes = torch.cat([W1[:, :H], W1[:, H:2 * H]], 0).contiguous()
    b_nodes = torch.cat([torch.zeros_like(pred.W1.bias), pred.W1.bias]).detach().contiguous()
    PQ = ops.linear(h, W_nodes, b_nodes)
    z1 = torch.empty((views.num_edges, hs), dtype=torch.float32, device=h.device)
    logits = torch.empty(views.num_edges, dtype=torch.float32, device=h.device)
    ops.edge_score(e, PQ[:, :hs], PQ[:, hs:], views, W1[:, 2 * H:], d(pred.W2.weight), d(pred.W2.bias), d(pred.W3.weight.reshape(-1)),
                   d(pred.W3.bias.reshape(-1)), logits, z1_out=z1)
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


def _draw_masks(model, views, x):
    """One scaled keep-mask per layer, drawn once per step: a forward that is run again as bf16x6 drops the same elements."""
    from . import train
    masks = [None] * len(model.gnn.convs)
    if model.kind == "sage":
        H = model.node_encoder.linear2.out_features   # (train.dropout_mask is looked up here, at call time: tests substitute known masks)
        masks = [train.dropout_mask(views.num_nodes, H, conv.feat_drop.p, x.device) if conv.feat_drop.p > 0 else None
                 for conv in model.gnn.convs]
    return masks


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
    """One training step as ONE autograd node whose inputs are the model's parameters.  `step` = (masks, forward, backward): this
    module's for GCNModel / SAGEModel, engine_gat's for GATModel - the range fallback, the empty graph and the release of the kept
    activations are the same for all three."""

    @staticmethod
    def forward(ctx, model, views, x, e_raw, names, step, *params):
        ops = hip_ops
        draw, fwd, _ = step
        masks = draw(model, views, x)
        bf16x6 = ops._TUNING.get(10, 0) == 1
        logits, kept = fwd(ops, model, views, x, e_raw, masks)
        if not bf16x6 and getattr(model, "range_check", True) and not bool(torch.isfinite(logits).all()):
            bf16x6 = True   # fp16x3's operand range did not hold (forward_in_range): the step runs as bf16x6
            with ops.bf16x6_arithmetic():
                logits, kept = fwd(ops, model, views, x, e_raw, masks)
        ctx.model, ctx.views, ctx.names, ctx.step, ctx.kept, ctx.inputs, ctx.bf16x6 = model, views, names, step, kept, (x, e_raw), bf16x6
        return logits.unsqueeze(1)

    @staticmethod
    def backward(ctx, dlogits):
        if ctx.kept is None:
            raise RuntimeError("the activations of this training step were released by its first backward(); "
                               "retain_graph=True is not supported - run the forward again")
        model, views, bwd = ctx.model, ctx.views, ctx.step[2]
        if views.num_edges == 0:   # nothing was scored: no parameter has a gradient
            grads = [torch.zeros_like(p) for _, p in model.named_parameters()]
        else:
            if ctx.bf16x6:
                with hip_ops.bf16x6_arithmetic():
                    g = bwd(hip_ops, model, views, *ctx.inputs, ctx.kept, dlogits)
            else:
                g = bwd(hip_ops, model, views, *ctx.inputs, ctx.kept, dlogits)
            grads = [g[n].contiguous() for n in ctx.names]
        ctx.kept = None
        return (None, None, None, None, None, None) + tuple(grads)


_STEP = (_draw_masks, _step_forward, _step_backward)


def run_train_step(model, graph, x, e, step):
    """What train_forward and engine_gat.train_forward share: the refusals, the views, the inputs on the compute device, the step."""
    from .train import TRAIN_SCORE_HIDDEN
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
    out = _BaselineStep.apply(model, views, xd, ed, names, step, *params)
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
