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
Train mode is not built: the model raises NotImplementedError.
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
