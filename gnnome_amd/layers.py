"""Host-side mirrors of the reference's layer classes for the SymGatedGCN path.

Same class names, constructor arguments, parameter / buffer names and forward signatures as
layers/gated_gcn_full.py:8-42,82-142 (SymGatedGCN), layers/processor.py:9-19
(SymGatedGCN_processor) and layers/score_predictor.py:5-24 (ScorePredictor), so a reference
state_dict loads unchanged.  The modules only OWN parameters; all arithmetic is done by the HIP
kernels behind include/gnnome_hip.h (see engine.py).  The layer-level forwards accept and return
edge tensors in DGL edge-id order like the reference; the model-level forward keeps them in
destination-sorted order across the whole stack and never permutes an [E,H] tensor.
"""
import torch
import torch.nn as nn

from . import engine
from .graph import views_for


class SymGatedGCN(nn.Module):
    arithmetic = "auto"   # see SymGatedGCNModel.arithmetic (layer-level API)

    def __init__(self, in_channels, out_channels, normalization, dropout=None, residual=True):
        super().__init__()
        if in_channels != out_channels:
            raise ValueError("the SymGatedGCN path is only ever built with in_channels == out_channels "
                             "(layers/processor.py:12-14); unequal widths are not supported")
        if not residual:
            raise ValueError("residual=False is never used by the reference drivers and is not supported")
        # built widths: 64 (the reference's default, configs/hyperparameters.py:22), 128, 256; other widths up to 256 run zero-padded on the
        # next built one (engine.BUILT_HIDDEN; train mode: train._padded_step) - with LayerNorm the statistics run over the model's own channels
        engine.padded_width(in_channels)   # (raises above the largest built width)
        self.dropout = dropout if dropout else 0.0
        self.normalization = normalization
        self.residual = residual
        dtype = torch.float32
        self.A_1 = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.A_2 = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.A_3 = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.B_1 = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.B_2 = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.B_3 = nn.Linear(in_channels, out_channels, dtype=dtype)
        if normalization == "batch":
            self.bn_h = nn.BatchNorm1d(out_channels, track_running_stats=True)
            self.bn_e = nn.BatchNorm1d(out_channels, track_running_stats=True)
        elif normalization == "layer":
            self.bn_h = nn.LayerNorm(out_channels)
            self.bn_e = nn.LayerNorm(out_channels)
        else:
            # the reference calls self.bn_e unconditionally (gated_gcn_full.py:106), so 'none' raises
            # AttributeError there; refuse it up front instead.
            raise ValueError("normalization must be 'batch' or 'layer'")

    def forward(self, g, h, e):
        """(h[N,H], e[E,H] in edge-id order) -> (h', e') like gated_gcn_full.py:82-142."""
        return engine.layer_forward_edge_id_order(self, g, h, e)


class SymGatedGCN_processor(nn.Module):
    def __init__(self, num_layers, hidden_features, normalization, dropout=None):
        super().__init__()
        self.convs = nn.ModuleList([
            SymGatedGCN(hidden_features, hidden_features, normalization, dropout) for _ in range(num_layers)
        ])

    def forward(self, graph, h, e):
        for conv in self.convs:
            h, e = conv(graph, h, e)
        return h, e


class ScorePredictor(nn.Module):
    def __init__(self, in_features, hidden_edge_scores):
        super().__init__()
        # built: in_features in {64,128,256}, hidden_edge_scores in {32,64,128} (reference default 64, 64); anything below the largest
        # runs zero-padded on the next built width (engine.prepare_predictor), anything above is refused here
        engine.padded_width(in_features)
        engine.padded_width(hidden_edge_scores, engine.BUILT_SCORE_HIDDEN, "hidden_edge_scores")
        self.W1 = nn.Linear(3 * in_features, hidden_edge_scores)
        self.W2 = nn.Linear(hidden_edge_scores, 32)
        self.W3 = nn.Linear(32, 1)

    def forward(self, graph, x, e):
        """scores[E,1] in edge-id order from x[N,H], e[E,H] (edge-id order); score_predictor.py:19-24."""
        return engine.score_forward_edge_id_order(self, graph, x, e)


class NodeEncoder(nn.Module):
    """layers/node_encoder.py:5-34: linear1 -> relu -> linear2.  Owns the parameters; the arithmetic is gnnome_encode_f32."""

    def __init__(self, in_channels, hidden_channels, out_channels, bias=True):
        super().__init__()
        if not bias:
            raise ValueError("the encoder kernels add both biases (the reference builds its encoders with bias=True)")
        if not (1 <= in_channels <= 8 and 1 <= hidden_channels <= 64):
            raise ValueError("the encoder kernels take in_channels <= 8 and hidden_channels <= 64 (reference: 2, 16)")
        self.linear1 = nn.Linear(in_channels, hidden_channels, bias=bias)
        self.linear2 = nn.Linear(hidden_channels, out_channels, bias=bias)
        self.relu = nn.ReLU()

    def forward(self, x):
        """rows[., in_channels] -> rows[., out_channels] on the MI355X (eval semantics, no autograd history)."""
        from . import ops as hip_ops
        engine._refuse_training(self)
        out_device = x.device
        device = engine.compute_device(x)
        with torch.no_grad():
            w = [t.detach().to(device=device, dtype=torch.float32).contiguous()
                 for t in (self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias)]
            return hip_ops.encode(x.detach().to(device=device, dtype=torch.float32).contiguous(), *w).to(out_device)


class EdgeEncoder(NodeEncoder):
    """layers/edge_encoder.py:4-34: the same two-layer encoder for the edge features."""


class GatedGCN(nn.Module):
    """layers/gated_gcn_full.py:145-230: the one-direction gated layer - SymGatedGCN without A_3 and without the pass over
    dgl.reverse(g).  Same refusals as SymGatedGCN; runs at the built widths only (no zero-padding for this layer).
    Train mode goes through GatedGCNModel (engine_gated.py: the symmetric training step with a zero A_3, at its cost)."""
    arithmetic = "auto"   # "auto" | "fast": the matrix-core kernels; "reference" is not served for this layer

    def __init__(self, in_channels, out_channels, normalization, dropout=None, residual=True):
        super().__init__()
        from . import engine_gated
        if in_channels != out_channels:
            raise ValueError("the GatedGCN path is only ever built with in_channels == out_channels "
                             "(layers/processor.py:25-27); unequal widths are not supported")
        if not residual:
            raise ValueError("residual=False is never used by the reference drivers and is not supported")
        engine_gated.built_width(in_channels)
        self.dropout = dropout if dropout else 0.0
        self.normalization = normalization
        self.residual = residual
        dtype = torch.float32
        self.A_1 = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.A_2 = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.B_1 = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.B_2 = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.B_3 = nn.Linear(in_channels, out_channels, dtype=dtype)
        if normalization == "batch":
            self.bn_h = nn.BatchNorm1d(out_channels, track_running_stats=True)
            self.bn_e = nn.BatchNorm1d(out_channels, track_running_stats=True)
        elif normalization == "layer":
            self.bn_h = nn.LayerNorm(out_channels)
            self.bn_e = nn.LayerNorm(out_channels)
        else:
            # the reference calls self.bn_e unconditionally (gated_gcn_full.py:207), so 'none' raises AttributeError there
            raise ValueError("normalization must be 'batch' or 'layer'")

    def forward(self, g, h, e):
        """(h[N,H], e[E,H] in edge-id order) -> (h', e') like gated_gcn_full.py:182-230."""
        from . import engine_gated
        return engine_gated.layer_forward_edge_id_order(self, g, h, e)


class GatedGCN_processor(nn.Module):
    def __init__(self, num_layers, hidden_features, normalization, dropout=None):
        super().__init__()
        self.convs = nn.ModuleList([
            GatedGCN(hidden_features, hidden_features, normalization, dropout) for _ in range(num_layers)
        ])

    def forward(self, graph, h, e):
        for conv in self.convs:
            h, e = conv(graph, h, e)
        return h, e


def _model_level_only(module):
    raise NotImplementedError(f"{type(module).__name__} owns parameters only: the reference runs it on g' = add_self_loop(g), which is never "
                              "built here - call GCNModel / SAGEModel / GATModel, whose forward runs the whole stack "
                              "(gnnome_amd/engine_baselines.py, engine_gat.py)")


class GraphConv(nn.Module):
    """The parameters of DGL 0.8.1's GraphConv(in, out, norm='both', weight=True, bias=True) as layers/processor.py:39 builds it:
    `weight` [in, out] (NOT nn.Linear's layout; Xavier uniform) and `bias` [out] (zeros).  In eval mode GCNModel computes
    h' = (din'^-1/2 * sum_{j in N'(i)} dout'[j]^-1/2 h[j]) weight + bias with it."""

    def __init__(self, in_feats, out_feats, norm="both", weight=True, bias=True):
        super().__init__()
        from . import engine_baselines
        if in_feats != out_feats or norm != "both" or not weight or not bias:
            raise ValueError("GraphConv is built as layers/processor.py:39 builds it: in == out, norm='both', weight=True, bias=True")
        engine_baselines.built_width(in_feats)
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats))
        self.bias = nn.Parameter(torch.zeros(out_feats))
        nn.init.xavier_uniform_(self.weight)

    def forward(self, graph, feat):
        _model_level_only(self)


class SAGEConv(nn.Module):
    """The parameters of DGL 0.8.1's SAGEConv(in, out, 'mean', feat_drop) as layers/processor.py:77 builds it: `bias` [out] (zeros),
    `fc_self` and `fc_neigh` (nn.Linear without bias; Xavier uniform with the ReLU gain, as DGL initialises them).  In eval mode
    SAGEModel computes h' = h fc_self.weight^T + (1/din' * sum_{j in N'(i)} h[j]) fc_neigh.weight^T + bias with it; feat_drop is
    the identity there."""

    def __init__(self, in_feats, out_feats, aggregator_type="mean", feat_drop=0.0, bias=True):
        super().__init__()
        from . import engine_baselines
        if in_feats != out_feats or aggregator_type != "mean" or not bias:
            raise ValueError("SAGEConv is built as layers/processor.py:77 builds it: in == out, the 'mean' aggregator, bias=True")
        engine_baselines.built_width(in_feats)
        self.feat_drop = nn.Dropout(feat_drop)
        self.bias = nn.Parameter(torch.zeros(out_feats))
        self.fc_self = nn.Linear(in_feats, out_feats, bias=False)
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=False)
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)

    def forward(self, graph, feat):
        _model_level_only(self)


class GCN_processor(nn.Module):
    """layers/processor.py:35-46: num_layers GraphConv, a ReLU after every one but the last.  State-dict keys `convs.N.weight`, `convs.N.bias`."""

    def __init__(self, num_layers, hidden_features):
        super().__init__()
        self.convs = nn.ModuleList([GraphConv(hidden_features, hidden_features, weight=True, bias=True) for _ in range(num_layers)])

    def forward(self, graph, h, e):
        _model_level_only(self)


class SAGE_processor(nn.Module):
    """layers/processor.py:73-84: num_layers SAGEConv('mean'), a ReLU after every one but the last.  State-dict keys `convs.N.bias`,
    `convs.N.fc_self.weight`, `convs.N.fc_neigh.weight`.  dropout=None means 0.0 here (the reference hands None to nn.Dropout, which fails)."""

    def __init__(self, num_layers, hidden_features, dropout=None):
        super().__init__()
        drop = dropout if dropout else 0.0
        self.convs = nn.ModuleList([SAGEConv(hidden_features, hidden_features, "mean", feat_drop=drop) for _ in range(num_layers)])

    def forward(self, graph, h, e):
        _model_level_only(self)


class GATConv(nn.Module):
    """The parameters of DGL 0.8.1's GATConv(in, out, num_heads, feat_drop, attn_drop=0) as layers/processor.py:55 builds it
    (negative_slope=0.2, residual=False, activation=None, bias=True): `fc` (nn.Linear [heads*out, in] without bias), `attn_l` and `attn_r`
    [1, heads, out] (all three Xavier normal with the ReLU gain, as DGL initialises them) and `bias` [heads*out] (zeros).  In eval mode
    GATModel computes, per head k, feat = fc(h)[:, k], el = (feat * attn_l[k]).sum(-1), er = (feat * attn_r[k]).sum(-1) and
    rst[i, k] = sum_{p in N'(i)} softmax_p(leaky_relu(el[nbr_p] + er[i], 0.2)) feat[nbr_p] + bias[k] with it; feat_drop is the identity there."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2, residual=False, activation=None,
                 bias=True):
        super().__init__()
        from . import engine_baselines
        if in_feats != out_feats or attn_drop or residual or activation is not None or not bias:
            raise ValueError("GATConv is built as layers/processor.py:55 builds it: in == out, attn_drop=0, residual=False, activation=None, "
                             "bias=True")
        if num_heads != 3:
            raise ValueError(f"num_heads={num_heads}: the attention kernel is built for 3 heads (layers/processor.py:50)")
        engine_baselines.built_width(in_feats, what="hidden_features (GATConv)")
        self.num_heads, self.negative_slope = num_heads, float(negative_slope)
        self.feat_drop = nn.Dropout(feat_drop)
        self.fc = nn.Linear(in_feats, num_heads * out_feats, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.bias = nn.Parameter(torch.zeros(num_heads * out_feats))
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)

    def forward(self, graph, feat):
        _model_level_only(self)


class GAT_processor(nn.Module):
    """layers/processor.py:49-70: num_layers GATConv of 3 heads, each followed by nn.Linear(3H, H) on the concatenated heads, a ReLU after
    every layer but the last.  State-dict keys `convs.N.{attn_l, attn_r, bias, fc.weight}`, `linears.N.{weight, bias}`.  dropout=None means
    0.0 here (the reference hands None to nn.Dropout, which fails); the reference's print at construction is not reproduced."""

    def __init__(self, num_layers, hidden_features, dropout=0.0, num_heads=3):
        super().__init__()
        if num_heads != 3:
            raise ValueError(f"num_heads={num_heads}: the attention kernel is built for 3 heads (layers/processor.py:50)")
        self.num_heads = num_heads
        drop = dropout if dropout else 0.0
        self.convs = nn.ModuleList([GATConv(hidden_features, hidden_features, num_heads=num_heads, feat_drop=drop, attn_drop=0)
                                    for _ in range(num_layers)])
        self.linears = nn.ModuleList([nn.Linear(num_heads * hidden_features, hidden_features) for _ in range(num_layers)])

    def forward(self, graph, h, e):
        _model_level_only(self)


__all__ = ["SymGatedGCN", "SymGatedGCN_processor", "ScorePredictor", "NodeEncoder", "EdgeEncoder", "GatedGCN", "GatedGCN_processor",
           "GraphConv", "SAGEConv", "GCN_processor", "SAGE_processor", "GATConv", "GAT_processor", "views_for"]
