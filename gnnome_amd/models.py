"""`SymGatedGCNModel` - drop-in for the reference's models/full_graph.py:9-30.

    model = SymGatedGCNModel(node_features, edge_features, hidden_features, hidden_ne_features,
                             num_layers, hidden_edge_scores, normalization, dropout=None)
    logits = model(graph, x, e)          # [E,1] fp32 logits in DGL edge-id order

Same positional constructor (inference.py:435, train.py:248), same 190 state_dict keys as
weights/weights.pt, same call.  Differences, all deliberate:
  * `graph` may be a DGLGraph, any object with .edges()/.num_nodes(), a (src, dst, N) tuple or a
    prebuilt gnnome_amd.ops.GraphViews.
  * inputs may live on the CPU (inference.py:388 pins device='cpu'): they are staged to the current
    HIP device and the logits are returned on the inputs' device.  The compute always runs on the
    MI355X; without the HIP library or a GPU the call raises.
  * the stray `print(x.shape)` of models/full_graph.py:25 is not reproduced.
  * `model.arithmetic` ("auto" | "reference" | "fast", default "auto") chooses, per layer, between the bf16x6
    matrix-core kernels and kernels that evaluate the layer's dense products in the reference's own ORDER (bit for bit
    what torch's CPU nn.Linear computes); "auto" uses the latter for layers whose eval-BatchNorm gain magnifies fp32
    reorder noise (engine.REFERENCE_ORDER_GAIN; the shipped checkpoint's layer 0).  Eval mode only.
  * `model.node_order` ("auto" | "input" | "locality", default "auto"): graph_parser.py:174-181 numbers reads in S-line order, which need not be
    the layout's; a cached graph object whose mean edge span says so gets its nodes renumbered once (gnnome_amd/node_order.py) - callers
    never see it (x goes in and logits come out in their numbering).
  * `model.activation_storage` ("fp32" | "bf16", default "fp32"; train mode only): "bf16" keeps the pre-normalisation gate output
    and its gradient in HBM as bfloat16 between the kernels of the training step (gnnome_amd/train.py; arithmetic stays fp32).
"""
import torch.nn as nn

from . import engine
from .layers import (EdgeEncoder, GAT_processor, GatedGCN_processor, GCN_processor, NodeEncoder, SAGE_processor, ScorePredictor,
                     SymGatedGCN_processor)


class SymGatedGCNModel(nn.Module):
    arithmetic = "auto"
    activation_storage = "fp32"
    node_order = "auto"      # gnnome_amd.graph.views_for: renumber the nodes of a cached graph object whose ids do not follow the layout
    range_check = True       # engine.forward_in_range: a forward that left fp16x3's operand range is run again as bf16x6

    def __init__(self, node_features, edge_features, hidden_features, hidden_ne_features, num_layers,
                 hidden_edge_scores, normalization, dropout=None):
        super().__init__()
        if not (1 <= node_features <= 8 and 1 <= edge_features <= 8 and 1 <= hidden_ne_features <= 64):
            raise ValueError("the encoder kernels take node/edge features <= 8 and hidden_ne_features <= 64 "
                             "(reference: 2, 2, 16 - configs/hyperparameters.py:20-25)")
        self.linear1_node = nn.Linear(node_features, hidden_ne_features, bias=True)
        self.linear2_node = nn.Linear(hidden_ne_features, hidden_features, bias=True)
        self.linear1_edge = nn.Linear(edge_features, hidden_ne_features, bias=True)
        self.linear2_edge = nn.Linear(hidden_ne_features, hidden_features, bias=True)
        self.gnn = SymGatedGCN_processor(num_layers, hidden_features, normalization, dropout=dropout)
        self.predictor = ScorePredictor(hidden_features, hidden_edge_scores)
        self.relu = nn.ReLU()

    def forward(self, graph, x, e):
        return engine.model_forward(self, graph, x, e)


class GatedGCNModel(nn.Module):
    """Drop-in for the reference's models/full_graph.py:33-53 - the one-direction baseline the symmetric model is compared against:
    NodeEncoder and EdgeEncoder, GatedGCN_processor (layers/gated_gcn_full.py:145-230: no A_3, no pass over dgl.reverse(g)),
    ScorePredictor.  Same constructor and state_dict keys (`node_encoder.linear{1,2}.*`, `edge_encoder.linear{1,2}.*`,
    `gnn.convs.N.*`, `predictor.W{1,2,3}.*`), same call; `graph` and the inputs as for SymGatedGCNModel.

    Eval mode runs its own kernel sequence (gnnome_amd/engine_gated.py): a [N,4H] projection, the symmetric model's gate, the in-edge
    aggregation kernel gnnome_node_aggregate_in_f32, the symmetric model's scorer.  directed=False runs the stack on the doubled edge
    list and scores the original graph (full_graph.py:47-51).  Built widths only: hidden_features in {64, 128, 256},
    hidden_edge_scores in {32, 64, 128}; `arithmetic` "auto" / "fast" (the matrix-core kernels) - "reference" raises.

    Train mode, `training_step = "symmetric"` (the default; directed=True only): the SYMMETRIC model's training step with a zero A_3 per
    layer - zero tensors, not Parameters, never updated: exact for every parameter this model has, and it costs what the symmetric step
    costs (the out-edge pass and the fifth projection block run on zeros).  `training_step = "in_edge"` (set it on the instance or on a
    subclass): the one-direction step - a [N,4H] projection, gnnome_node_aggregate_in_raw_f32 and its backward
    gnnome_node_aggregate_in_bwd_f32 - for both `directed` values; fp32 storage, no recompute_gate.  Any other value raises ValueError.

    Multi-GPU (gnnome_amd/dist.py): eval mode and the "in_edge" step run on a destination-range partition built with
    PartitionedGraph.from_global(..., in_edges_only=True), directed=True only; "symmetric" raises NotImplementedError there."""
    arithmetic = "auto"
    activation_storage = "fp32"
    range_check = True
    training_step = "symmetric"

    def __init__(self, node_features, edge_features, hidden_features, hidden_ne_features, num_layers, hidden_edge_scores,
                 normalization, dropout=None, directed=True):
        super().__init__()
        from . import engine_gated
        engine_gated.built_width(hidden_features)
        engine_gated.built_width(hidden_edge_scores, engine.BUILT_SCORE_HIDDEN, "hidden_edge_scores")
        self.directed = directed
        self.node_encoder = NodeEncoder(node_features, hidden_ne_features, hidden_features)
        self.edge_encoder = EdgeEncoder(edge_features, hidden_ne_features, hidden_features)
        self.gnn = GatedGCN_processor(num_layers, hidden_features, normalization, dropout=dropout)
        self.predictor = ScorePredictor(hidden_features, hidden_edge_scores)

    def forward(self, graph, x, e):
        from . import engine_gated
        return engine_gated.model_forward(self, graph, x, e)


class _BaselineModel(nn.Module):
    """What GCNModel, SAGEModel and GATModel share: encoders, the scorer, the refusals and the call (gnnome_amd/engine_baselines.py)."""
    kind = None
    range_check = True

    def __init__(self, node_features, edge_features, hidden_features, hidden_ne_features, hidden_edge_scores, directed):
        super().__init__()
        from . import engine_baselines
        engine_baselines.built_width(hidden_features)
        engine_baselines.built_width(hidden_edge_scores, engine.BUILT_SCORE_HIDDEN, "hidden_edge_scores")
        self.directed = directed
        self.node_encoder = NodeEncoder(node_features, hidden_ne_features, hidden_features)
        self.edge_encoder = EdgeEncoder(edge_features, hidden_ne_features, hidden_features)

    def forward(self, graph, x, e):
        from . import engine_baselines
        return engine_baselines.model_forward(self, graph, x, e)


class GCNModel(_BaselineModel):
    """Drop-in for the reference's models/full_graph.py:56-75 - the GCN ablation baseline: NodeEncoder and EdgeEncoder, GCN_processor
    (layers/processor.py:35-46: DGL's GraphConv with norm='both', a ReLU between layers), ScorePredictor.  Same constructor and
    state_dict keys (`node_encoder.linear{1,2}.*`, `edge_encoder.linear{1,2}.*`, `gnn.convs.N.{weight,bias}`, `predictor.W{1,2,3}.*`),
    same call; `graph` and the inputs as for SymGatedGCNModel; logits [E,1] in edge-id order on the inputs' device.

    The convolutions run on g' = add_self_loop(g), or add_self_loop(add_reverse_edges(g)) with directed=False, which is never built:
    the degree-normalised neighbour sum is the kernel gnnome_node_neighbour_sum_f32 over the graph's own in- and out-lists.  The encoded
    e goes unchanged to the scorer, which scores the original graph.  `normalization` is accepted and unused, as in the reference.
    Built widths only: hidden_features in {64, 128, 256}, hidden_edge_scores in {32, 64, 128}.  The call serves eval mode only: in train
    mode it raises NotImplementedError.  The training step is the explicit entry engine_baselines.train_forward(model, graph, x, e)
    (logits with autograd history to the parameters; its backward runs on gnnome_node_neighbour_sum_bwd_f32), which
    trainer.train(model_class=GCNModel) calls.  On several GPUs: dist.PartitionedRunner over the default destination-range partition, eval
    mode (forward) and the training step (train_forward), on the partition forms of the two kernels; an in-edge-only partition and the
    captured forward are refused (DESIGN 7c "Partitions")."""
    kind = "gcn"

    def __init__(self, node_features, edge_features, hidden_features, hidden_ne_features, num_layers, hidden_edge_scores,
                 normalization, dropout=None, directed=True):
        super().__init__(node_features, edge_features, hidden_features, hidden_ne_features, hidden_edge_scores, directed)
        self.gnn = GCN_processor(num_layers, hidden_features)
        self.predictor = ScorePredictor(hidden_features, hidden_edge_scores)


class SAGEModel(_BaselineModel):
    """Drop-in for the reference's models/full_graph.py:100-119 - the GraphSAGE ablation baseline: NodeEncoder and EdgeEncoder,
    SAGE_processor (layers/processor.py:73-84: DGL's SAGEConv with the 'mean' aggregator, a ReLU between layers), ScorePredictor.
    Same constructor and state_dict keys (`gnn.convs.N.bias`, `gnn.convs.N.fc_self.weight`, `gnn.convs.N.fc_neigh.weight`, the
    encoders' and the predictor's as for GCNModel), same call; g', the scorer, `normalization`, the built widths and eval mode as for
    GCNModel.

    One divergence: the reference's default dropout=None reaches nn.Dropout(None) and fails at construction; here None means 0.0.
    feat_drop is the identity in eval mode; the training step (engine_baselines.train_forward, as for GCNModel - the call itself refuses
    train mode) draws one scaled keep-mask per layer through train.dropout_mask and applies it to the layer's input before both the self
    and the neighbour path, as DGL's SAGEConv does.  On a partition (dist.PartitionedRunner, as for GCNModel) the masks are drawn for the
    owned rows and the halo rows of every layer's input, layer 0's included, are the owners' dropped rows."""
    kind = "sage"

    def __init__(self, node_features, edge_features, hidden_features, hidden_ne_features, num_layers, hidden_edge_scores,
                 normalization, dropout=None, directed=True):
        super().__init__(node_features, edge_features, hidden_features, hidden_ne_features, hidden_edge_scores, directed)
        self.gnn = SAGE_processor(num_layers, hidden_features, dropout=dropout)
        self.predictor = ScorePredictor(hidden_features, hidden_edge_scores)


class GATModel(_BaselineModel):
    """Drop-in for the reference's models/full_graph.py:78-97 - the attention ablation baseline: NodeEncoder and EdgeEncoder,
    GAT_processor (layers/processor.py:49-70: DGL's GATConv with 3 heads, nn.Linear(3H, H) on the concatenated heads, a ReLU between
    layers), ScorePredictor.  Same constructor and state_dict keys (`gnn.convs.N.{attn_l, attn_r, bias, fc.weight}`,
    `gnn.linears.N.{weight, bias}`, the encoders' and the predictor's as for GCNModel), same call; g', the scorer, `normalization`, the
    built widths and eval mode as for GCNModel.  The call serves eval mode only, as GCNModel's; the training step is the explicit entry
    engine_gat.train_forward(model, graph, x, e) (its backward runs on gnnome_node_attention_sum_bwd_f32; feat_drop as one scaled keep-mask
    per layer on the layer's input), which trainer.train(model_class=GATModel) calls.  engine_baselines.train_forward refuses this model.

    Per layer (gnnome_amd/engine_gat.py): ONE projection on [fc.weight ; attn_l fc ; attn_r fc] gives feat, el and er as column blocks of
    a [N, 3H + 64] table, the edge softmax and the weighted sum are the kernel gnnome_node_attention_sum_f32 over the graph's own in- and
    out-lists, then the head mix.  As for SAGEModel, dropout=None means 0.0 (the reference fails on it), and the reference's print at
    construction is not reproduced.  On several GPUs: dist.GATPartitionedRunner over the default destination-range partition, eval mode
    and the training step, both `directed` values, on the partition forms of the attention kernels (DESIGN 7d "Partitions");
    dist.PartitionedRunner refuses this model and names that class."""
    kind = "gat"

    def __init__(self, node_features, edge_features, hidden_features, hidden_ne_features, num_layers, hidden_edge_scores,
                 normalization, dropout=None, directed=True):
        super().__init__(node_features, edge_features, hidden_features, hidden_ne_features, hidden_edge_scores, directed)
        self.gnn = GAT_processor(num_layers, hidden_features, dropout=dropout, num_heads=3)
        self.predictor = ScorePredictor(hidden_features, hidden_edge_scores)

    def forward(self, graph, x, e):
        from . import engine_gat
        return engine_gat.model_forward(self, graph, x, e)


__all__ = ["SymGatedGCNModel", "GatedGCNModel", "GCNModel", "SAGEModel", "GATModel"]
