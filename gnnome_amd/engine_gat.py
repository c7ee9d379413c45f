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

Several GPUs: the last section of this file - the same two sequences on one rank of a destination-range partition
(dist.GATPartitionedRunner), on gnnome_node_attention_sum_part_f32 / _stats_part_f32 / _bwd_dst_part_f32 / _bwd_src_part_f32.
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


_STEP = (eb.draw_masks, _step_forward, _step_backward)


def train_forward(model, graph, x, e):
    """The training step of GATModel (the reference's train.py:138-145 runs `model(g, x, e)` in train mode; here that call keeps raising
    and this is the explicit entry, as engine_baselines.train_forward is GCNModel's and SAGEModel's): logits [E,1] on the compute device,
    with autograd history to model.parameters().  `graph` as for the model's call; views of a reversed graph (GraphViews.reversed) are
    the model of the swapped edge list."""
    if getattr(model, "kind", None) != "gat":
        raise TypeError(f"engine_gat.train_forward serves GATModel, not {type(model).__name__}")
    return eb.run_train_step(model, graph, x, e, _STEP)


# ---------------------------------------------------------------------------------------------------
# destination-range partitions (gnnome_amd/dist.py, GATPartitionedRunner): one rank's rows of the same two sequences
# ---------------------------------------------------------------------------------------------------
# On the DEFAULT partition (every edge with an owned end) an owned node's in- and out-list are complete, so every softmax of an owned
# destination sees all of its terms: with feat | el of the halo rows at hand the part entries of csrc/node_attention.hip compute the owned
# rows with the whole graph's association - BIT-EQUAL to the single-rank kernel on equal tables.  The halo rows of P = h Wp^T are projected
# LOCALLY from the exchanged halo rows of h (H floats per row, the exchange GCNModel makes) rather than exchanged themselves (3H + 64
# floats per row, 3.25 times the bytes): redundant product rows against bytes on the link - which is cheaper is not measured.
# Backward, per layer: every edge's term of dfeat[j] / del[j] is computed by j's owner and its term of der[i] by i's owner, so the stack
# needs no halo transpose and no partial sums - but the source walk reads G = dA and the 64-byte work row (er | m | 1/den | D) of every
# destination j points at, and those are their owners': TWO forward-direction exchanges per layer, G's halo rows (3H floats each, in
# flight under the destination phase, which reads owned rows of G only) and work's (16 floats each) between the two phases.  Only the
# scorer's node gradient (halo_bwd) and the parameter gradients (sum_ranks, once, at the end) are summed across ranks.
# feat_drop: the OWNER applies ReLU and mask to its owned rows BEFORE the exchange, so halo rows arrive dropped and masks are drawn for
# owned rows only; with p > 0 layer 0's dropped input is exchanged too (a local copy made from x would lack the owner's mask).

def shard_lists(part):
    """The lists the part entries read (engine_baselines.ShardLists: the out-lists in the whole graph's order), made once per partition."""
    hit = part._baseline.get("lists")
    if hit is None:
        hit = part._baseline["lists"] = eb.ShardLists(part.views, part.node_gid)
    return hit


def check_partition(model, part):
    """The refusals of GATModel on a partition, before anything is allocated."""
    from .dist import check_shard
    if getattr(model, "kind", None) != "gat":
        raise TypeError(f"the GAT partition sequences serve GATModel, not {type(model).__name__}")
    if getattr(part, "in_edges_only", False):
        raise ValueError("GATModel runs on the default partition, not in_edges_only=True: its backward walks the owned nodes' out-lists "
                         "(and directed=False its forward too), which an in-edge-only partition does not hold")
    check_shard(part)
    eb.built_width(model.node_encoder.linear2.out_features)


def _project_part(ops, h, Wp, planes, n_own, finish):
    """P [n_local, 3H + 64] = h Wp^T of ALL local rows, the halo rows made locally once they have arrived (engine.project_rows)."""
    return engine.project_rows(lambda rows, out: ops.linear(rows, Wp, None, out=out, planes=planes), h, n_own, finish, Wp.shape[0])


def run_partitioned(ops, prep, part, x_local, e_local, group=None, directed=True):
    """run_stack on one rank: x_local [n_local,F] (owned, then halo), e_local [e_local,F] in local edge-id order -> logits[E_global].
    Per layer: the halo rows of the layer's input (layer 0's come straight from x), the projection of all local rows, the attention sum,
    the head mix and the ReLU on the owned rows; one more exchange of the last h, then the scorer on the owned in-edges."""
    from .dist import HaloExchange
    views, n_own, n_local, H = part.views, part.n_own, part.n_local, prep.hidden
    W = HEADS * H
    lists = shard_lists(part)
    xchg = HaloExchange(part, ops, group)
    h = ops.encode(x_local, *prep.enc_node)
    e = ops.encode(e_local, *prep.enc_edge, gather=views.srt_eid[:part.n_score], rows=part.n_score)   # the scored rows, sorted order
    L = len(prep.layers)
    A = torch.empty((n_own, W), dtype=torch.float32, device=h.device) if L else None
    for i, lw in enumerate(prep.layers):
        if i > 0:
            xchg.start(h)
        P = _project_part(ops, h, lw.Wp, lw.planes, n_own, xchg.finish)
        ops.node_attention_sum_part(P[:, :W], lists, n_own, P[:, W:W + 4], P[:n_own, W + 4:W + 8], bias=lw.bias, negative_slope=lw.slope,
                                    both=not directed, out=A)
        h = torch.empty((n_local, H), dtype=torch.float32, device=h.device)
        ops.linear(A, lw.W, lw.b, out=h[:n_own])
        if i + 1 < L:
            ops.relu_rows(h[:n_own])
    if L:
        xchg.start(h)
        xchg.finish()
    pw = prep.predictor
    return eb.score_part(ops, part, group, e, h, (pw["W_nodes"], pw["b_nodes"], pw.get("planes")), engine.tail_weights(pw))


def _part_step_forward(ops, model, sh, x, e_raw, masks):
    """_step_forward on a shard -> (logits[E_global], what the backward reads).  Kept per layer: h_d and P for the local rows; A, stats
    and the mask for the owned rows."""
    d = lambda t: t.detach().contiguous()  # noqa: E731
    part, views, n_own, n_local = sh.part, sh.views, sh.n_own, sh.n_local
    both = not model.directed
    lists = shard_lists(part)
    enc_node, enc_edge = eb.live_encoders(model)
    h = ops.encode(x, *enc_node)
    e = ops.encode(e_raw, *enc_edge, gather=views.srt_eid[:sh.e_own], rows=sh.e_own)
    H = h.shape[1]
    W = HEADS * H
    layers = []
    for i, (conv, lin) in enumerate(zip(model.gnn.convs, model.gnn.linears)):
        if masks[i] is not None:          # the owner drops its rows; the halo rows arrive dropped
            ops.relu_mul_rows(h[:n_own], masks[i], relu=i > 0)
        elif i > 0:
            ops.relu_rows(h[:n_own])
        if i > 0 or masks[0] is not None:   # (layer 0 without a mask: the halo rows are what x encodes to)
            sh.halo_start(h)
        Wp = fold_on_device(conv)
        P = _project_part(ops, h, Wp, None, n_own, sh.halo_finish)
        A, stats = ops.node_attention_sum_stats_part(P[:, :W], lists, n_own, P[:, W:W + 4], P[:n_own, W + 4:W + 8], bias=d(conv.bias),
                                                     negative_slope=float(conv.negative_slope), both=both)
        layers.append(dict(h_d=h, P=P, A=A, stats=stats, mask=masks[i], Wp=Wp))
        h = torch.empty((n_local, H), dtype=torch.float32, device=h.device)
        ops.linear(A, d(lin.weight), d(lin.bias), out=h[:n_own])
    if layers:
        sh.halo_start(h)
        sh.halo_finish()
    W1, W_nodes, b_nodes, tail = eb.live_predictor(model.predictor, H)
    z1 = torch.empty((sh.e_own, model.predictor.W1.out_features), dtype=torch.float32, device=h.device)
    logits = eb.score_part(ops, part, sh.group, e, h, (W_nodes, b_nodes, None), tail, z1_out=z1)
    return logits, dict(h=h, e=e, z1=z1, W1=W1, W_nodes=W_nodes, layers=layers)


def _part_step_backward(ops, model, sh, x, e_raw, kept, dlogits):
    """_step_backward on a shard -> {parameter name: this rank's share of the gradient}.  Per layer the head mix's backward on the owned
    rows, the exchange of G = dA's halo rows under the destination phase, the exchange of the halo work rows, the source phase, and dWp, dh
    from the owned rows of dP.  Only the scorer's node gradient returns partial rows to their owners (halo_bwd)."""
    from .train import score_backward_on_shard
    d = lambda t: t.detach().contiguous()  # noqa: E731
    n_own, n_local, e_own = sh.n_own, sh.n_local, sh.e_own
    both = not model.directed
    lists = shard_lists(sh.part)
    H = kept["h"].shape[1]
    W = HEADS * H
    dev = dlogits.device
    g = {}
    dh, de = score_backward_on_shard(ops, model.predictor, sh, g, dlogits, kept["z1"], kept["e"], kept["h"], kept["W1"], kept["W_nodes"], e_own)
    sh.halo_bwd(dh)
    dY = dh[:n_own]
    dP = None
    if kept["layers"]:
        dP = torch.empty((n_own, W + SCORE_COLUMNS), dtype=torch.float32, device=dev)
        dP[:, W + 8:].zero_()   # the 56 score columns no kernel writes: once per table
    for i in range(len(kept["layers"]) - 1, -1, -1):
        conv, lin, s = model.gnn.convs[i], model.gnn.linears[i], kept["layers"][i]
        g[f"gnn.linears.{i}.weight"] = ops.wgrad(dY, s["A"])
        g[f"gnn.linears.{i}.bias"] = sY = ops.colsum2(dY)[0]
        G = torch.empty((n_local, W), dtype=torch.float32, device=dev)
        ops.linear(dY, d(lin.weight).t().contiguous(), None, out=G[:n_own])
        sh.halo_start(G)                   # 3H floats per halo row, in flight under the destination phase (which reads owned rows of G)
        g[f"gnn.convs.{i}.bias"] = (sY.double() @ lin.weight.detach().double()).float()
        P = s["P"]
        work = torch.empty((n_local, 16), dtype=torch.float32, device=dev)
        ops.node_attention_sum_bwd_dst_part(G, lists, n_own, P[:, :W], P[:, W:W + 4], P[:n_own, W + 4:W + 8], s["A"], s["stats"],
                                            bias=d(conv.bias), negative_slope=float(conv.negative_slope), both=both,
                                            der=dP[:, W + 4:W + 8], work=work)
        sh.halo_finish()
        sh.halo_start(work)                # 16 floats per halo row
        sh.halo_finish()
        ops.node_attention_sum_bwd_src_part(G, lists, n_own, P[:n_own, :W], P[:n_own, W:W + 4], work,
                                            negative_slope=float(conv.negative_slope), both=both, dfeat=dP[:, :W], del_=dP[:, W:W + 4])
        h_d = s["h_d"][:n_own]
        for name, grad in unfold(conv, ops.wgrad(dP, h_d)).items():
            g[f"gnn.convs.{i}.{name}"] = grad
        dY = ops.linear(dP, s["Wp"].t().contiguous(), None)
        if s["mask"] is not None:
            ops.relu_mul_rows(dY, s["mask"], relu=False)
        if i > 0:                          # h_d > 0 exactly where the ReLU passed and the mask kept
            dY = ops.relu_bwd(dY, h_d)
        kept["layers"][i] = s = None
    eb.encoders_backward_on_shard(ops, model, sh, g, dY, de, x, e_raw)
    return g


def train_forward_on(model, shard, x_local, e_local):
    """The training step of GATModel over one rank's rows (dist.PartitionShard over the default partition): x_local / e_local are the input
    features of the shard's nodes (owned, then halo) and edges (local edge-id order).  Returns logits[E_global, 1], complete on every
    rank; after backward() every rank holds the whole graph's parameter gradients."""
    check_partition(model, shard.part)
    names, params = eb.check_step_on(model, shard, x_local, e_local)
    step = (eb.draw_masks,   # (the shell hands the sequences shard.views; they read the shard itself)
            lambda ops, model, views, *rest: _part_step_forward(ops, model, shard, *rest),
            lambda ops, model, views, *rest: _part_step_backward(ops, model, shard, *rest))
    return eb._BaselineStep.apply(model, shard, x_local, e_local, names, step, *params)
