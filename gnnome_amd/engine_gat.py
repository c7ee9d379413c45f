"""Host logic of the attention baseline, GATModel (models/full_graph.py:78-97, layers/processor.py:49-70): weight preparation and the
kernel sequence, beside engine_baselines.py, whose treatment of g', range fallback and call it shares.

The convolutions run on g' = add_self_loop(g) (directed=True) or add_self_loop(add_reverse_edges(g)) (directed=False), which is never
built (engine_baselines.py); the encoded e goes unchanged to the scorer, which scores the ORIGINAL graph.  Eval mode, per layer (N nodes,
H hidden, 3 heads):
    P  = h Wp^T                      [N, 3H + 64] = feat | el, pad | er, pad | zeros       gnnome_linear_planes_f32, one product
    A  = softmax-weighted sum + bias [N, 3H]                                               gnnome_node_attention_sum_f32 (csrc/node_attention.hip)
    h' = A linears[i]^T + bias       [N, H]                                                gnnome_linear_f32 (K = 3H)
a ReLU (gnnome_relu_rows_f32, in place) after every layer but the last, then the symmetric model's scorer.

THE FOLD.  DGL computes el[i,k] = sum_c feat[i,k,c] attn_l[k,c] from feat = h fc^T.  Here el[i,k] = h[i] . (attn_l[k] fc[kH:(k+1)H]) - the
row vector attn_l[k] fc_k is formed once per layer in fp64 and rounded to fp32 - and rides as row 3H + k of the projection weight (er: row
3H + 4 + k), so feat, el and er leave ONE product as 16-byte aligned column blocks of P and there is no score kernel.  The fold changes the
order of el's fp32 sum: about 1e-6 on O(1) values, far inside the model bar.  P and A are allocated once per forward.

Train mode: `model(graph, x, e)` keeps raising NotImplementedError (its tests pin that); the training step is the explicit entry
train_forward(model, graph, x, e), which trainer.train calls for this model - engine_baselines' autograd.Function (_BaselineStep: its
refusals, range fallback, empty graph and release of the kept activations) around this module's forward and backward.  Forward = the eval
sequence on the live parameters with Wp folded ON THE DEVICE every step (fp64 torch on parameter-sized tensors, rounded once: no host
sync), GATConv's feat_drop on each layer's INPUT (DGL drops h before fc; attn_drop is 0) - one scaled keep-mask per layer with p > 0
(train.dropout_mask), applied where the previous ReLU touches the row (gnnome_relu_mul_rows_f32; layer 0: no ReLU) - and the attention sum
in its training form, which leaves the softmax statistics.  Kept per layer: h_d (the dropped, post-ReLU input), P, A, stats, the mask, Wp.
Backward, per layer from the last (dY = the gradient of the head mix's output):
    d linears.weight, bias = wgrad(dY, A), column sums of dY;  dA = dY W                   gnnome_wgrad_f32, gnnome_colsum2_f32, gnnome_linear_f32
    d convs.bias = column sums of dA = (column sums of dY) W                             parameter-sized: fp64 torch on the device, rounded once
    dP = d feat | d el, 0 | d er, 0 | zeros                                                gnnome_node_attention_sum_bwd_f32 (csrc/node_attention_bwd.hip)
    dWp = wgrad(dP, h_d);  dh = dP Wp                                                      (M = K = 3H + 64: shapes the two products take)
    dY' = [h_d > 0] mask dh                                                                gnnome_relu_mul_rows_f32 (relu = 0), gnnome_relu_bwd_f32; no gate at layer 0
    THE UNFOLD, on parameter-sized tensors (torch on the device): d fc_k = dWp[kH:(k+1)H] + attn_l[k]^T dWp[3H+k] + attn_r[k]^T dWp[3H+4+k],
    d attn_l[k] = fc_k dWp[3H+k], d attn_r[k] = fc_k dWp[3H+4+k]
then the scorer's and the encoders' backward (engine_baselines.score_backward, encoders_backward).  No atomics anywhere: two steps from
equal state leave equal gradient bits.
"""
import torch

from . import engine
from . import engine_baselines as eb
from . import ops as hip_ops
from .engine_gated import in_edge_views

HEADS = 3
SCORE_COLUMNS = 64      # columns of P after feat: el at +0..2, er at +4..6, zeros - keeps Nout = 3H + 64 a shape of gnnome_linear_planes_f32


class GatLayer:
    """One convolution and its head mix as the kernels read them: Wp[3H + 64, H] and its fp16x3 planes (or None), the conv's bias[3H],
    its negative slope, the head mix W[H, 3H] and bias[H]."""
    __slots__ = ("Wp", "planes", "bias", "slope", "W", "b")


def projection_weight(conv):
    """Wp[3H + 64, H] on the host: rows 0..3H-1 fc.weight, row 3H + k attn_l[k] fc_k, row 3H + 4 + k attn_r[k] fc_k (fp64, rounded once)."""
    fc = conv.fc.weight.detach().to(device="cpu", dtype=torch.float64)
    hidden = fc.shape[1]
    if fc.shape[0] != HEADS * hidden:
        raise ValueError(f"GATConv.fc.weight is {tuple(fc.shape)}: built for {HEADS} heads of in == out features")
    Wp = torch.zeros(HEADS * hidden + SCORE_COLUMNS, hidden, dtype=torch.float64)
    Wp[:HEADS * hidden] = fc
    for off, attn in ((0, conv.attn_l), (4, conv.attn_r)):
        a = attn.detach().to(device="cpu", dtype=torch.float64).reshape(HEADS, hidden)
        for k in range(HEADS):
            Wp[HEADS * hidden + off + k] = a[k] @ fc[k * hidden:(k + 1) * hidden]
    return Wp.to(torch.float32)


def prepare_layer(conv, lin, device):
    def dev(t):
        return t.detach().to(device=device, dtype=torch.float32).contiguous()

    lw = GatLayer()
    lw.Wp = dev(projection_weight(conv))
    Nout, hidden = lw.Wp.shape
    eb.built_width(hidden)
    lw.planes = hip_ops.weight_planes(lw.Wp) if hip_ops.planes_supported(hidden, Nout) and lw.Wp.is_cuda else None
    lw.bias, lw.slope = dev(conv.bias), float(conv.negative_slope)
    lw.W, lw.b = dev(lin.weight), dev(lin.bias)
    if lw.W.shape != (hidden, HEADS * hidden):
        raise ValueError(f"GAT_processor.linears weight is {tuple(lw.W.shape)}, expected {(hidden, HEADS * hidden)}")
    return lw


class Prepared:
    """Device-resident, kernel-ready copies of a GATModel's parameters (eval semantics)."""

    def __init__(self, model, device):
        def dev(t):
            return t.detach().to(device=device, dtype=torch.float32).contiguous()

        self.device, self.kind = device, model.kind
        assert self.kind == "gat"
        self.hidden = eb.built_width(model.node_encoder.linear2.out_features)
        self.enc_node = tuple(dev(t) for t in (model.node_encoder.linear1.weight, model.node_encoder.linear1.bias,
                                               model.node_encoder.linear2.weight, model.node_encoder.linear2.bias))
        self.enc_edge = tuple(dev(t) for t in (model.edge_encoder.linear1.weight, model.edge_encoder.linear1.bias,
                                               model.edge_encoder.linear2.weight, model.edge_encoder.linear2.bias))
        self.layers = [prepare_layer(conv, lin, device) for conv, lin in zip(model.gnn.convs, model.gnn.linears)]
        self.predictor = engine.prepare_predictor(model.predictor, device)
        weights = [t for lw in self.layers for t in (lw.Wp, lw.W)] + [self.predictor["_W1"], self.predictor["W2"]]
        amax = max((float(t.abs().max()) if t.numel() else 0.0) for t in weights)
        self.force_bf16x6 = not (amax < engine.hip_ops_fp16_max())   # fp16x3's operand range, checked once for the weights
        self.range_verified = self.range_failed = None


def gat_stack(ops, layers, views, h, both):
    """processor.py:61-70 on g'.  P and A live for the whole stack."""
    if not layers:
        return h
    N, H = h.shape
    P = torch.empty((N, HEADS * H + SCORE_COLUMNS), dtype=torch.float32, device=h.device)
    A = torch.empty((N, HEADS * H), dtype=torch.float32, device=h.device)
    feat, el, er = P[:, :HEADS * H], P[:, HEADS * H:HEADS * H + 4], P[:, HEADS * H + 4:HEADS * H + 8]
    for i, lw in enumerate(layers):
        ops.linear(h, lw.Wp, None, out=P, planes=lw.planes)
        ops.node_attention_sum(feat, views, el, er, bias=lw.bias, negative_slope=lw.slope, both=both, out=A)
        h = ops.linear(A, lw.W, lw.b)
        if i + 1 < len(layers):
            ops.relu_rows(h)
    return h


def run_stack(ops, prep, views, x, e_raw, directed=True):
    """Encoders -> L convolutions on g' -> scorer on g; logits[E] at the original edge ids."""
    views = in_edge_views(views)
    h = engine.encode_nodes(ops, views, x, prep.enc_node)
    e = ops.encode(e_raw, *prep.enc_edge, gather=views.srt_eid, rows=views.num_edges)   # sorted order: what the scorer reads
    h = gat_stack(ops, prep.layers, views, h, not directed)
    logits = torch.empty(views.num_edges, dtype=torch.float32, device=h.device)
    engine.score_step(ops, prep.predictor, views, h, e, logits)
    return logits


def model_forward(model, graph, x, e):
    """models/full_graph.py:87-97 on the MI355X."""
    return eb.model_forward(model, graph, x, e, prepared=Prepared, stack=run_stack)


# ---------------------------------------------------------------------------------------------------
# train mode (the autograd.Function is engine_baselines._BaselineStep)
# ---------------------------------------------------------------------------------------------------

def fold_on_device(conv):
    """projection_weight without the host: Wp[3H + 64, H] from the live fc, attn_l and attn_r on their device, fp64, rounded once."""
    fc = conv.fc.weight.detach().double()
    hidden = fc.shape[1]
    if fc.shape[0] != HEADS * hidden:
        raise ValueError(f"GATConv.fc.weight is {tuple(fc.shape)}: built for {HEADS} heads of in == out features")
    W = HEADS * hidden
    Wp = torch.zeros((W + SCORE_COLUMNS, hidden), dtype=torch.float64, device=fc.device)
    Wp[:W] = fc
    fck = fc.view(HEADS, hidden, hidden)
    for off, attn in ((0, conv.attn_l), (4, conv.attn_r)):
        a = attn.detach().double().reshape(HEADS, 1, hidden)
        Wp[W + off:W + off + HEADS] = torch.bmm(a, fck)[:, 0]
    return Wp.float()


def unfold(conv, dWp):
    """The gradients of fc.weight [3H,H], attn_l and attn_r [1,3,H] from dWp [3H + 64, H] (the fold's transpose, fp32 on the device)."""
    fc = conv.fc.weight.detach()
    hidden = fc.shape[1]
    W = HEADS * hidden
    fck = fc.view(HEADS, hidden, hidden)
    dfc = dWp[:W].clone().view(HEADS, hidden, hidden)
    out = {}
    for off, name, attn in ((0, "attn_l", conv.attn_l), (4, "attn_r", conv.attn_r)):
        rows = dWp[W + off:W + off + HEADS]                                   # [3, H]: d (attn[k] fc_k)
        dfc += attn.detach().reshape(HEADS, hidden, 1) * rows[:, None, :]     # attn[k]^T rows[k]
        out[name] = torch.bmm(fck, rows[:, :, None])[:, :, 0].reshape(1, HEADS, hidden)
    out["fc.weight"] = dfc.view(W, hidden)
    return out


def _draw_masks(model, views, x):
    """One scaled keep-mask per layer with p > 0, drawn once per step: a forward that is run again as bf16x6 drops the same elements."""
    from . import train
    H = model.node_encoder.linear2.out_features   # (train.dropout_mask is looked up here, at call time: tests substitute known masks)
    return [train.dropout_mask(views.num_nodes, H, conv.feat_drop.p, x.device) if conv.feat_drop.p > 0 else None
            for conv in model.gnn.convs]


def _step_forward(ops, model, views, x, e_raw, masks):
    """The train-mode forward on sorted-order e -> (logits[E], what the backward reads)."""
    d = lambda t: t.detach().contiguous()  # noqa: E731
    both = not model.directed
    h, e = eb.encoders_forward(ops, model, views, x, e_raw)
    N, H = h.shape
    W = HEADS * H
    layers = []
    for i, (conv, lin) in enumerate(zip(model.gnn.convs, model.gnn.linears)):
        if masks[i] is not None:          # feat_drop on the layer's input, where the previous layer's ReLU touches the row
            ops.relu_mul_rows(h, masks[i], relu=i > 0)
        elif i > 0:
            ops.relu_rows(h)
        Wp = fold_on_device(conv)
        P = ops.linear(h, Wp, None)
        A, stats = ops.node_attention_sum_stats(P[:, :W], views, P[:, W:W + 4], P[:, W + 4:W + 8], bias=d(conv.bias),
                                                negative_slope=float(conv.negative_slope), both=both)
        layers.append(dict(h_d=h, P=P, A=A, stats=stats, mask=masks[i], Wp=Wp))
        h = ops.linear(A, d(lin.weight), d(lin.bias))
    logits, kept = eb.score_forward(ops, model, views, h, e)
    kept["layers"] = layers
    return logits, kept


def _step_backward(ops, model, views, x, e_raw, kept, dlogits):
    """-> {parameter name: gradient}."""
    d = lambda t: t.detach().contiguous()  # noqa: E731
    both = not model.directed
    N, H = kept["h"].shape
    W = HEADS * H
    g = {}
    dY, de = eb.score_backward(ops, model, views, kept, dlogits, g)
    dP = torch.empty((N, W + SCORE_COLUMNS), dtype=torch.float32, device=dY.device) if kept["layers"] else None
    for i in range(len(kept["layers"]) - 1, -1, -1):
        conv, lin, s = model.gnn.convs[i], model.gnn.linears[i], kept["layers"][i]
        g[f"gnn.linears.{i}.weight"] = ops.wgrad(dY, s["A"])
        g[f"gnn.linears.{i}.bias"] = sY = ops.colsum2(dY)[0]
        dA = ops.linear(dY, d(lin.weight).t().contiguous(), None)
        # the column sums of dA = dY W are (the column sums of dY) W: parameter-sized, fp64, rounded once (gnnome_colsum2_f32 sums rows of
        # 16..256 floats, not of 3H)
        g[f"gnn.convs.{i}.bias"] = (sY.double() @ lin.weight.detach().double()).float()
        P = s["P"]
        ops.node_attention_sum_bwd(dA, views, P[:, :W], P[:, W:W + 4], P[:, W + 4:W + 8], s["A"], s["stats"], bias=d(conv.bias),
                                   negative_slope=float(conv.negative_slope), both=both, dP=dP)
        for name, grad in unfold(conv, ops.wgrad(dP, s["h_d"])).items():
            g[f"gnn.convs.{i}.{name}"] = grad
        dY = ops.linear(dP, s["Wp"].t().contiguous(), None)
        if s["mask"] is not None:
            ops.relu_mul_rows(dY, s["mask"], relu=False)
        if i > 0:                          # h_d > 0 exactly where the ReLU passed and the mask kept
            dY = ops.relu_bwd(dY, s["h_d"])
        kept["layers"][i] = s = None
    eb.encoders_backward(ops, model, views, g, dY, de, x, e_raw)
    return g


_STEP = (_draw_masks, _step_forward, _step_backward)


def train_forward(model, graph, x, e):
    """The training step of GATModel (the reference's train.py:138-145 runs `model(g, x, e)` in train mode; here that call keeps raising
    and this is the explicit entry, as engine_baselines.train_forward is GCNModel's and SAGEModel's): logits [E,1] on the compute device,
    with autograd history to model.parameters().  `graph` as for the model's call; views of a reversed graph (GraphViews.reversed) are
    the model of the swapped edge list."""
    if getattr(model, "kind", None) != "gat":
        raise TypeError(f"engine_gat.train_forward serves GATModel, not {type(model).__name__}")
    return eb.run_train_step(model, graph, x, e, _STEP)
