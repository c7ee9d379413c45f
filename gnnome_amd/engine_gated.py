"""Host logic of the one-direction GatedGCN path (models/full_graph.py:33-53, layers/gated_gcn_full.py:145-230): weight
preparation and the kernel sequences of GatedGCNModel, beside engine.py (the symmetric model), which stays as it is.

Eval mode, per layer (N nodes, E edges, H hidden; e in DESTINATION-SORTED order across the whole stack):
    P    = h Wcat^T + bcat      [N,4H] = A1h|A2h|B1h|B2h, one GEMM         gnnome_linear_planes_f32 / gnnome_linear_f32
    e'   = relu(bn_e(B1h[src] + B2h[dst] + B_3 e)) + e                      the symmetric model's fused gate, unchanged
    h'   = relu(bn_h(A1h + fwd)) + h                                        gnnome_node_aggregate_in_f32 (csrc/node_aggregate_in.hip)
then the symmetric model's scorer.  There is no A_3 block in the projection and no out-edge half in the aggregation.
Only the matrix-core arithmetic is served: `arithmetic="reference"` raises.

directed=False (full_graph.py:47-51): the stack runs on the doubled edge list src|dst -> dst|src (the reverse copy of edge k
has id E + k), fed with the encoded e twice; the ORIGINAL graph is scored with the rows of the first E edge ids.  The doubled
views and the two row maps are kept with the graph's own cached views (GraphViews._derived; graph.views_for), so they are built once
per graph object.

Train mode goes through the symmetric model's training step (train._TrainStep): an adapter presents the model under the
symmetric model's attribute names, SHARING the Parameter objects, and gives every layer a zero A_3 (plain zero tensors, no
Parameters: never updated, absent from state_dict).  That is exact for every real parameter and for dh, because A3h = 0
makes bwd = +0, d bwd / d sigma = 0 and A_3^T dA3h = 0.  It COSTS WHAT THE SYMMETRIC STEP COSTS - the out-edge pass and the
fifth projection block are computed on zeros.  That is the default (`GatedGCNModel.training_step = "symmetric"`), for directed=True.

`training_step = "in_edge"` selects the step of this model's own (train_forward_in_edge, below): a [N,4H] projection, the train-form
gate, gnnome_node_aggregate_in_raw_f32 forward and gnnome_node_aggregate_in_bwd_f32 backward (csrc/node_aggregate_in_bwd.hip) - no
A_3, no out-edge half, no Tb / Ub tables - and directed=False on the doubled edge list.  The same step runs one rank's rows of an
in-edge-only destination-range partition (train_forward_in_edge_on over dist.PartitionShard) on the partition forms
gnnome_node_aggregate_in_raw_part_f32 / gnnome_node_aggregate_in_bwd_part_f32; eval mode on a partition is dist.run_partitioned.

directed=False on a partition: the doubled graph is again a one-direction problem, so its plan is the in-edge-only partition of the doubled
edge list (dist.PartitionedGraph.from_global(..., in_edges_only=True, doubled=True)); the partition forms above serve it unchanged.  The
plan's enc_rows / score_rows are the per-rank counterparts of doubled_row_maps' enc_gather / score_gather: the scorer gathers the
score_rows and runs under views of those edges alone, as run_stack does with score_gather on a whole graph.  Not served on a partition:
the captured forward, training_step = "symmetric", bf16 storage and recompute_gate.
"""
import torch
import torch.nn.functional as F

from . import engine
from . import ops as hip_ops
from .graph import views_for
from .ops import GraphViews

ARITHMETIC_MODES = ("auto", "fast")   # both: the matrix-core kernels; the reference-order route is not served for this model


def built_width(width, built=engine.BUILT_HIDDEN, what="hidden_features"):
    """GatedGCN runs at the built widths only (zero-padding is not served for this model)."""
    if width not in built:
        raise ValueError(f"{what}={width}: GatedGCN is built for {what} in {tuple(built)}")
    return width


def check_arithmetic(module):
    mode = getattr(module, "arithmetic", "auto")
    if mode not in ARITHMETIC_MODES:
        raise ValueError(f"arithmetic={mode!r}: GatedGCN serves {ARITHMETIC_MODES} (the matrix-core kernels); the reference-order "
                         "route is built for SymGatedGCN only")
    return mode


class GatedLayerWeights:
    """What engine.gate / the aggregation read of one layer (engine.LayerWeights' names; ref is always False here)."""
    __slots__ = ("Wcat", "bcat", "W3", "b3", "norm", "scale_e", "shift_e", "scale_h", "shift_h", "ref", "planes")


def prepare_layer(conv, device, arithmetic=None):
    def dev(t):
        return t.detach().to(device=device, dtype=torch.float32).contiguous()

    check_arithmetic(conv)
    hidden = built_width(conv.B_3.weight.shape[0])
    lw = GatedLayerWeights()
    lw.Wcat = dev(torch.cat([conv.A_1.weight, conv.A_2.weight, conv.B_1.weight, conv.B_2.weight], 0))
    # B_3's bias rides on the B2h rows: B1h[src] + (B2h[dst] + b3) + e*W3^T (as in engine.prepare_layer)
    lw.bcat = dev(torch.cat([conv.A_1.bias, conv.A_2.bias, conv.B_1.bias, conv.B_2.bias + conv.B_3.bias], 0))
    lw.W3, lw.b3 = dev(conv.B_3.weight), dev(conv.B_3.bias)
    lw.norm, lw.scale_e, lw.shift_e = engine._norm_affine(conv.bn_e, device)
    kind_h, lw.scale_h, lw.shift_h = engine._norm_affine(conv.bn_h, device)
    assert kind_h == lw.norm
    lw.ref = False
    lw.planes = hip_ops.weight_planes(lw.Wcat) if hip_ops.planes_supported(hidden, 4 * hidden) and lw.Wcat.is_cuda else None
    return lw


class Prepared:
    """Device-resident, kernel-ready copies of a GatedGCNModel's parameters (eval semantics)."""

    def __init__(self, model, device):
        def dev(t):
            return t.detach().to(device=device, dtype=torch.float32).contiguous()

        check_arithmetic(model)
        self.device = device
        self.directed = bool(getattr(model, "directed", True))   # (dist.run_partitioned: directed=False on a doubled plan only, checked up front)
        self.hidden = built_width(model.node_encoder.linear2.out_features)
        self.enc_node = tuple(dev(t) for t in (model.node_encoder.linear1.weight, model.node_encoder.linear1.bias,
                                               model.node_encoder.linear2.weight, model.node_encoder.linear2.bias))
        self.enc_edge = tuple(dev(t) for t in (model.edge_encoder.linear1.weight, model.edge_encoder.linear1.bias,
                                               model.edge_encoder.linear2.weight, model.edge_encoder.linear2.bias))
        self.layers = [prepare_layer(conv, device) for conv in model.gnn.convs]
        self.predictor = engine.prepare_predictor(model.predictor, device)
        weights = [t for lw in self.layers for t in (lw.Wcat, lw.W3)] + [self.predictor["_W1"], self.predictor["W2"]]
        amax = max((float(t.abs().max()) if t.numel() else 0.0) for t in weights) if weights else 0.0
        self.force_bf16x6 = not (amax < engine.hip_ops_fp16_max())   # fp16x3's operand range, checked once for the weights
        self.range_verified = self.range_failed = None


# ---------------------------------------------------------------------------------------------------
# graphs: true views of a reversed graph, and the doubled edge list of directed=False
# ---------------------------------------------------------------------------------------------------

def edge_list_of(views):
    """(src, dst) int32 in edge-id order, in the views' own node numbering."""
    src = torch.empty(views.num_edges, dtype=torch.int32, device=views.device)
    dst = torch.empty_like(src)
    eid = views.srt_eid.long()
    src[eid], dst[eid] = views.srt_src, views.srt_dst
    return (dst, src) if views.transposed else (src, dst)


def _carry_numbering(new, views):
    new.node_perm, new.node_gather = views.node_perm, views.node_gather   # (built from internal ids: the same renumbering applies)
    return new


def in_edge_views(views):
    """Views whose CONTIGUOUS runs are the in-edges of the graph `views` stands for.  The aggregation of this model reads
    in_ptr / srt_src only, so views of dgl.reverse(g) (GraphViews.reversed: the same arrays, roles exchanged by the caller)
    are rebuilt once over the swapped edge list - same edge ids - and kept with the views they came from (GraphViews._derived,
    which graph.views_for's cache keeps alive with the graph object)."""
    if not views.transposed:
        return views
    hit = views._derived.get("reversed")
    if hit is None:
        src, dst = edge_list_of(views)
        hit = views._derived["reversed"] = _carry_numbering(GraphViews(src, dst, views.num_nodes, validate=False), views)
    return hit


def doubled_edge_list(src, dst):
    """dgl.add_reverse_edges (full_graph.py:48): src|dst -> dst|src - edge k keeps its id, its reverse copy gets id E + k."""
    return torch.cat([src, dst]), torch.cat([dst, src])


def doubled_row_maps(srt_eid_doubled, srt_eid, num_edges):
    """The two row maps of directed=False, from the sorted edge ids of the doubled views and of the original ones (E = num_edges):
    enc_gather[p]   = the ORIGINAL edge whose encoded features row p of the doubled sorted order carries (e fed twice: id >= E -> id - E),
    score_gather[q] = the doubled sorted position of the edge at sorted position q of the original views - the rows of the first E ids,
                      e[:E], in the order the scorer reads them.  Both int32, on the inputs' device."""
    eid2, E = srt_eid_doubled, int(num_edges)
    enc_gather = torch.where(eid2 >= E, eid2 - E, eid2).to(torch.int32).contiguous()
    pos_of = torch.empty(2 * E, dtype=torch.int32, device=eid2.device)
    pos_of[eid2.long()] = torch.arange(2 * E, dtype=torch.int32, device=eid2.device)
    return enc_gather, pos_of[srt_eid.long()].contiguous()


class Doubled:
    """The doubled graph of directed=False: views over doubled_edge_list and the two maps of doubled_row_maps."""

    def __init__(self, views):
        src, dst = doubled_edge_list(*edge_list_of(views))
        self.views = _carry_numbering(GraphViews(src, dst, views.num_nodes, validate=False), views)
        self.enc_gather, self.score_gather = doubled_row_maps(self.views.srt_eid, views.srt_eid, views.num_edges)


def doubled_for(views):
    """(views: not transposed - run_stack hands in in_edge_views' result)"""
    hit = views._derived.get("doubled")
    if hit is None:
        hit = views._derived["doubled"] = Doubled(views)
    return hit


# ---------------------------------------------------------------------------------------------------
# kernel sequences (ops = gnnome_amd.ops)
# ---------------------------------------------------------------------------------------------------

def layer_step(ops, lw, views, h, e, raw_edges=None, scratch=None, n_out=None):
    """One GatedGCN layer on sorted-order e; returns (new h, e).  e = None with raw_edges = (e_raw, encoder weights): the edge
    encoder is folded into the gate (layer 0), as in the symmetric model."""
    H = h.shape[1]
    P = ops.linear(h, lw.Wcat, lw.bcat, planes=lw.planes)   # [N,4H] = A1h|A2h|B1h|B2h (gated_gcn_full.py:194-199)
    A1, A2, B1, B2 = (P[:, i * H:(i + 1) * H] for i in range(4))
    e = engine.gate(ops, lw, views, e, B1, B2, raw_edges, scratch)
    return ops.node_aggregate_in(e, A1, A2, views, h, lw.norm, lw.scale_h, lw.shift_h, num_nodes_out=n_out), e


def run_stack(ops, prep, views, x, e_raw, directed=True):
    """Encoders -> L layers -> scorer; logits[E] at the original edge ids."""
    score_views = views = in_edge_views(views)
    h = engine.encode_nodes(ops, views, x, prep.enc_node)
    if directed:
        e = engine.encode_edges(ops, prep, views, e_raw)   # None: layer 0's gate produces it on the fly
    else:
        dbl = doubled_for(views)
        views = dbl.views
        e = ops.encode(e_raw, *prep.enc_edge, gather=dbl.enc_gather, rows=views.num_edges)
    scratch = {}
    for lw in prep.layers:
        h, e = layer_step(ops, lw, views, h, e, raw_edges=(e_raw, prep.enc_edge), scratch=scratch)
    if e is None:   # a model without layers: the scorer reads the encoder's output
        e = ops.encode(e_raw, *prep.enc_edge, gather=views.srt_eid, rows=views.num_edges)
    if not directed:
        e = ops.gather_rows(e, dbl.score_gather)
    logits = torch.empty(score_views.num_edges, dtype=torch.float32, device=h.device)
    engine.score_step(ops, prep.predictor, score_views, h, e, logits)
    return logits


def forward_in_range(ops, prep, views, x, e, xd, ed, directed, check=True):
    """engine.forward_in_range for this stack: a forward whose logits are not all finite left fp16x3's operand range and is run
    again as bf16x6; checked once per set of inputs."""
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
# module entry points
# ---------------------------------------------------------------------------------------------------

TRAINING_STEPS = ("symmetric", "in_edge")


def training_step_of(model):
    kind = getattr(model, "training_step", "symmetric")
    if kind not in TRAINING_STEPS:
        raise ValueError(f"training_step={kind!r} not in {TRAINING_STEPS}")
    return kind


def model_forward(model, graph, x, e):
    """models/full_graph.py:42-53 on the MI355X."""
    if model.training:
        step = train_forward_in_edge if training_step_of(model) == "in_edge" else train_forward
        return step(model, graph, x, e).to(x.device)
    out_device = x.device
    device = engine.compute_device(x, e)
    prep = engine.prepared_for(model, device, Prepared)
    views = views_for(graph, device, node_order="input")
    if x.shape[0] != views.num_nodes or e.shape[0] != views.num_edges:
        raise ValueError(f"x has {x.shape[0]} rows for {views.num_nodes} nodes, e has {e.shape[0]} rows for {views.num_edges} edges")
    with torch.no_grad():
        xd = x.detach().to(device=device, dtype=torch.float32).contiguous()
        ed = e.detach().to(device=device, dtype=torch.float32).contiguous()
        logits = forward_in_range(hip_ops, prep, views, x, e, xd, ed, bool(model.directed), check=getattr(model, "range_check", True))
    views.check_range()   # a fresh graph's deferred endpoint check, after the whole forward has been enqueued
    return logits.unsqueeze(1).to(out_device)


def layer_forward_edge_id_order(conv, g, h, e):
    """gated_gcn_full.py:182-230 with e given and returned in edge-id order."""
    engine._refuse_training(conv)
    out_device = h.device
    device = engine.compute_device(h, e)
    lw = engine.prepared_for(conv, device, prepare_layer)
    views = in_edge_views(views_for(g, device))
    with torch.no_grad():
        hd = h.detach().to(device=device, dtype=torch.float32).contiguous()
        ed = e.detach().to(device=device, dtype=torch.float32).contiguous()
        es = hip_ops.gather_rows(ed, views.srt_eid)
        if views.node_gather is not None:   # views over renumbered nodes: rows in, rows out in the caller's numbering
            hd = hip_ops.gather_rows(hd, views.node_gather)
        h_new, es = layer_step(hip_ops, lw, views, hd, es)
        if views.node_perm is not None:
            h_new = h_new.index_select(0, views.node_perm)
        e_new = torch.empty_like(es)
        e_new[views.srt_eid.long()] = es
        h_new = F.dropout(h_new, conv.dropout, training=conv.training)
    views.check_range()
    return h_new.to(out_device), e_new.to(out_device)


# ---------------------------------------------------------------------------------------------------
# train mode: the symmetric training step on an adapter with a zero A_3
# ---------------------------------------------------------------------------------------------------

class _ZeroLinear:
    """A_3 as the symmetric step sees it for this model: zero weight and bias - tensors, not Parameters."""

    def __init__(self, like):
        self.weight = torch.zeros_like(like.weight, requires_grad=False)
        self.bias = torch.zeros_like(like.bias, requires_grad=False)


class _SymLayer:
    bn_e_updates = 1   # gated_gcn_full.py:207 applies bn_e once per layer (the symmetric layer twice): one momentum update per step

    def __init__(self, conv):
        self.conv = conv
        self.A_1, self.A_2, self.B_1, self.B_2, self.B_3 = conv.A_1, conv.A_2, conv.B_1, conv.B_2, conv.B_3
        self.bn_h, self.bn_e = conv.bn_h, conv.bn_e
        self.A_3 = _ZeroLinear(conv.A_2)

    @property
    def dropout(self):
        return self.conv.dropout


class _Convs:
    def __init__(self, convs):
        self.convs = convs


class SymAdapter:
    """GatedGCNModel under the attribute names train._TrainStep reads of a SymGatedGCNModel; every Parameter is the model's own."""

    def __init__(self, model):
        self.linear1_node, self.linear2_node = model.node_encoder.linear1, model.node_encoder.linear2
        self.linear1_edge, self.linear2_edge = model.edge_encoder.linear1, model.edge_encoder.linear2
        self.gnn = _Convs([_SymLayer(conv) for conv in model.gnn.convs])
        self.predictor = model.predictor
        self.device = next(model.parameters()).device
        self.layers = len(model.gnn.convs)
        # the step returns its gradients under the symmetric model's names, in the order of the model's own named_parameters()
        own = [n for n, _ in model.named_parameters()]
        self.names = [_sym_name(n) for n in own]
        self.activation_storage = getattr(model, "activation_storage", "fp32")
        self.recompute_gate = getattr(model, "recompute_gate", False)


def _sym_name(name):
    for enc, kind in (("node_encoder.", "_node"), ("edge_encoder.", "_edge")):
        if name.startswith(enc):
            layer, leaf = name[len(enc):].split(".")      # linear1.weight -> linear1_node.weight
            return f"{layer}{kind}.{leaf}"
    return name


def train_forward(model, graph, x, e):
    """`model(graph, x, e)` in train mode with autograd support, through train._TrainStep (see the module docstring)."""
    from .train import TRAIN_SCORE_HIDDEN, WholeGraph, _TrainStep
    check_arithmetic(model)
    if not model.directed:
        raise NotImplementedError("train mode of GatedGCNModel is built for directed=True; directed=False is served in eval mode")
    device = engine.compute_device(x, e)
    params = [p for _, p in model.named_parameters()]
    if any(p.device != device for p in params):
        raise RuntimeError("training needs the model on the compute device: call model.to(device) first")
    built_width(model.node_encoder.linear2.out_features)
    built_width(model.predictor.W1.out_features, TRAIN_SCORE_HIDDEN, "hidden_edge_scores")
    adapter = model.__dict__.get("_gnnome_sym_adapter")
    if adapter is None or adapter.device != device or adapter.layers != len(model.gnn.convs):
        adapter = model.__dict__["_gnnome_sym_adapter"] = SymAdapter(model)
    adapter.activation_storage = getattr(model, "activation_storage", "fp32")
    adapter.recompute_gate = getattr(model, "recompute_gate", False)
    views = views_for(graph, device, node_order="input")
    xd = x.detach().to(device=device, dtype=torch.float32).contiguous()
    ed = e.detach().to(device=device, dtype=torch.float32).contiguous()
    out = _TrainStep.apply(adapter, WholeGraph(views), xd, ed, adapter.names, *params)
    views.check_range()
    return out


# ---------------------------------------------------------------------------------------------------
# train mode, training_step = "in_edge": the one-direction step
# ---------------------------------------------------------------------------------------------------

def _cat4(conv):
    """(Wcat [4H,H], bcat [4H]) = A_1 | A_2 | B_1 | B_2 of one layer; B_3's bias rides on the B2h rows (prepare_layer)."""
    Wcat = torch.cat([conv.A_1.weight, conv.A_2.weight, conv.B_1.weight, conv.B_2.weight], 0).detach().contiguous()
    bcat = torch.cat([conv.A_1.bias, conv.A_2.bias, conv.B_1.bias, conv.B_2.bias + conv.B_3.bias], 0).detach().contiguous()
    return Wcat, bcat


class _StepGraph:
    """Where one in-edge step runs: `sh` (train.WholeGraph) over the views the STACK runs on - the graph's in-edge views, or the doubled
    ones of directed=False - `enc_gather`, the original edge id each of the stack's sorted rows encodes, and the views and rows that are
    scored (`score_gather` = None: every row of the stack, as it lies)."""

    def __init__(self, views, directed, doubled=doubled_for, ops=hip_ops):
        """doubled, ops: the builder of the doubled graph and the backend (the tests run the step's host logic on a torch backend)."""
        from .train import WholeGraph
        self.score_views = self.seg_views = views   # seg_views: whose in- / out-lists the scorer's node gathers are transposed over
        self.num_scored = self.num_logits = views.num_edges   # (num_logits: the length of the complete logits)
        if directed:
            self.sh, self.enc_gather, self.score_gather = WholeGraph(views, ops), views.srt_eid, None
        else:
            dbl = doubled(views)
            self.sh, self.enc_gather, self.score_gather = WholeGraph(dbl.views, ops), dbl.enc_gather, dbl.score_gather

    @classmethod
    def on_shard(cls, shard):
        """One rank's rows of an in-edge-only destination-range partition (dist.PartitionShard): the stack runs on the local views, every
        local edge is an owned in-edge.  directed=True: each is scored here, into this rank's piece of the logits.  directed=False (a doubled
        plan): the local rows are this rank's share of the 2E doubled ones, e_local already carries every row's original features
        (PartitionedGraph.enc_rows), and the scorer reads the shard's score_rows - the copies with ids below E, possibly none - under the
        views of those edges alone."""
        self = object.__new__(cls)
        self.sh, self.enc_gather, self.score_gather = shard, shard.views.srt_eid, shard.score_rows
        self.score_views, self.seg_views, self.num_scored = shard.score_views, shard.seg_views, shard.e_scored
        self.num_logits = shard.part.scored.total
        return self


class _InEdgeStep(torch.autograd.Function):
    """One training step of GatedGCNModel (gated_gcn_full.py:182-230 in train mode, full_graph.py:42-53) as ONE autograd node whose inputs
    are the model's parameters - train._TrainStep's shape on the one-direction kernels.  fp32 storage.  A single process (train.WholeGraph),
    or one rank of an in-edge-only destination-range partition (dist.PartitionShard; directed=False: of the doubled list): n_own owned rows first, halo rows of h
    refreshed before every projection, BatchNorm statistics over the owned rows merged across ranks, the halo rows of dh - which carry this
    rank's PARTIAL gradients, as do the halo rows of dA2h / dB1h - returned to their owners once per layer, parameter gradients summed over ranks.
    The single-process case issues exactly the calls it issued before shards were served."""

    @staticmethod
    def forward(ctx, model, sg, x, e_raw, names, *params):
        from . import train
        sh = sg.sh
        ops, views = sh.ops, sh.views
        convs = model.gnn.convs
        layer_norm = len(convs) > 0 and isinstance(convs[0].bn_e, torch.nn.LayerNorm)
        H = model.node_encoder.linear2.out_features
        n, E2 = views.num_nodes, views.num_edges
        n_own = sh.n_own
        whole = sh.alone and n_own == n   # the single-process case; otherwise a shard: rows [n_own, n) are halo rows
        d = lambda t: t.detach().contiguous()  # noqa: E731
        ne, ee = model.node_encoder, model.edge_encoder
        node_gather = getattr(views, "node_gather", None)   # views over renumbered nodes read x (caller's numbering) through it
        h = ops.encode(x, d(ne.linear1.weight), d(ne.linear1.bias), d(ne.linear2.weight), d(ne.linear2.bias),
                       **({} if node_gather is None else dict(gather=node_gather, rows=n)))   # (a shard's halo rows of layer 0 come from x)
        # directed=False: the encoded e fed twice - row p of the doubled sorted order encodes original edge enc_gather[p]
        e = ops.encode(e_raw, d(ee.linear1.weight), d(ee.linear1.bias), d(ee.linear2.weight), d(ee.linear2.bias), gather=sg.enc_gather, rows=E2)
        saved = []
        for li, conv in enumerate(convs):
            Wcat, bcat = _cat4(conv)
            if whole:
                P = ops.linear(h, Wcat, bcat)   # [N,4H] = A1h|A2h|B1h|B2h (gated_gcn_full.py:194-199)
            else:
                if li > 0:
                    sh.halo_start(h)
                P = engine.project_rows(lambda rows, out: ops.linear(rows, Wcat, bcat, out=out), h, n_own, sh.halo_finish, 4 * H)
            A1, A2, B1, B2 = (P[:, i * H:(i + 1) * H] for i in range(4))
            mean_e = rstd_e = sc_e = sh_e = mean_h = rstd_h = sc_h = sh_h = None
            path, xe, stats = train._raw_gate(sh, conv, e, B1, B2, layer_norm, torch.float32)
            if layer_norm:
                e_new = ops.ln_relu_res(xe, d(conv.bn_e.weight), d(conv.bn_e.bias), e)
            else:   # bn_e is applied ONCE per layer (gated_gcn_full.py:207): one momentum update; directed=False: statistics over all 2E rows
                if path == "moments":
                    mean_e, rstd_e, sc_e, sh_e = train._bn_train_fused(sh, conv.bn_e, stats, updates=1)
                else:
                    # (a shard: every local edge is an owned in-edge, each edge of the graph on exactly one rank)
                    mean_e, rstd_e, sc_e, sh_e = train._bn_train(sh, conv.bn_e, stats[0], stats[1], sh.e_own, sh.e_global, updates=1)
                e_new = ops.bn_relu_res(xe, sc_e, sh_e, e)
            # v, hf, rdf: the owned rows
            v, hf, rdf = ops.node_aggregate_in_raw(e_new, A1, A2, views) if whole else ops.node_aggregate_in_raw_part(e_new, A1, A2, views, n_own)
            # a shard keeps n rows of h: the owned ones are written here, the halo rows by the next exchange
            h_rows = None if whole else torch.empty((n, H), dtype=torch.float32, device=x.device)
            into = {} if whole else dict(out=h_rows[:n_own])
            if layer_norm:
                h_next = ops.ln_relu_res(v, d(conv.bn_h.weight), d(conv.bn_h.bias), h[:n_own], **into)
            else:
                if train._can_fuse_bn(sh, conv.bn_h):
                    mean_h, rstd_h, sc_h, sh_h = train._bn_train_fused(sh, conv.bn_h, ops.batch_moments(v), updates=1)
                else:
                    m_h, v_h = ops.batch_stats(v)
                    mean_h, rstd_h, sc_h, sh_h = train._bn_train(sh, conv.bn_h, m_h, v_h, n_own, sh.n_global, updates=1)
                h_next = ops.bn_relu_res(v, sc_h, sh_h, h[:n_own], **into)
            mask = None
            if conv.dropout > 0.0:
                mask = train.dropout_mask(n_own, H, conv.dropout, x.device)
                if whole:
                    h_next = ops.mul23(h_next, mask, mask)[0]
                else:
                    h_rows[:n_own].copy_(ops.mul23(h_rows[:n_own], mask, mask)[0])
            if not whole:
                h_next = h_rows
            saved.append(dict(h=h, P=P, e=e, xe=xe, e_new=e_new, v=v, hf=hf, rdf=rdf, mask=mask, Wcat=Wcat, mean_e=mean_e, rstd_e=rstd_e,
                              sc_e=sc_e, sh_e=sh_e, mean_h=mean_h, rstd_h=rstd_h, sc_h=sc_h, sh_h=sh_h))
            h, e = h_next, e_new

        pred = model.predictor
        hs = pred.W1.out_features
        W1 = d(pred.W1.weight)
        W_nodes = torch.cat([W1[:, :H], W1[:, H:2 * H]], 0).contiguous()
        b_nodes = torch.cat([torch.zeros_like(pred.W1.bias), pred.W1.bias]).detach().contiguous()
        if not whole:
            sh.halo_start(h)
            sh.halo_finish()
        PQ = ops.linear(h, W_nodes, b_nodes)
        # directed=False: the ORIGINAL graph is scored with the rows of the first E edge ids (full_graph.py:51)
        E = sg.num_scored   # (0 on a rank of a doubled plan whose in-edges are all reverse copies: it scores nothing and gathers with the others)
        e_sc = engine.scored_rows(ops, e, sg.score_gather, E)
        z1 = torch.empty((E, hs), dtype=torch.float32, device=h.device)
        w_tail = (W1[:, 2 * H:], d(pred.W2.weight), d(pred.W2.bias), d(pred.W3.weight.reshape(-1)), d(pred.W3.bias.reshape(-1)))
        logits = engine.score_tail(ops, e_sc, PQ[:, :hs], PQ[:, hs:], w_tail, sg.score_views, E, sg.num_logits, z1_out=z1, **sh.logits_finish)
        ctx.model, ctx.sg, ctx.names, ctx.saved = model, sg, names, saved
        ctx.tail = dict(h=h, e_sc=e_sc, z1=z1, W1=W1, W_nodes=W_nodes, x=x, e_raw=e_raw)
        return logits.unsqueeze(1)

    @staticmethod
    def backward(ctx, dlogits):
        from . import train
        model, sg, saved, tail = ctx.model, ctx.sg, ctx.saved, ctx.tail
        if saved is None:
            raise RuntimeError("the activations of this training step were released by its first backward(); "
                               "retain_graph=True is not supported - run the forward again")
        sh = sg.sh
        ops, views, sv = sh.ops, sh.views, sg.score_views
        H = model.node_encoder.linear2.out_features
        n, E2 = views.num_nodes, views.num_edges
        n_own = sh.n_own
        whole = sh.alone and n_own == n
        d = lambda t: t.detach().contiguous()  # noqa: E731
        dev = dlogits.device
        g = {}
        # A shard: rows that also live on another rank (halo nodes) carry PARTIAL gradients here.  Everything below is linear in the incoming
        # gradient, so the per-rank parameter gradients sum to the whole graph's (sum_ranks at the end), and the halo rows of dh go back to
        # their owners once per layer (halo_bwd_start / halo_bwd_finish), which add them in ascending rank order.

        # ---- scorer (score_predictor.py:12-17), over the scored views
        pred = model.predictor
        hs = pred.W1.out_features
        dl = dlogits.reshape(-1).contiguous().float()
        if sg.num_scored == 0:
            # a rank of a doubled plan that scored nothing: its share of the predictor's gradients, of de and of dh is zero; the layers
            # below still run, for the gradients that reach its rows through the peers' halo rows of dh
            for k, p in pred.named_parameters():
                g["predictor." + k] = torch.zeros_like(p)
            de = torch.zeros((E2, H), dtype=torch.float32, device=dev)
            dh = torch.zeros((n, H), dtype=torch.float32, device=dev)
        else:
            dz1, dz2, u = ops.score_tail_bwd(tail["z1"], dl, sv, d(pred.W2.weight), d(pred.W2.bias), d(pred.W3.weight.reshape(-1)))
            g["predictor.W2.weight"] = ops.wgrad(dz2, tail["z1"])
            g["predictor.W2.bias"] = ops.colsum2(dz2)[0]
            g["predictor.W3.weight"] = ops.colsum2(u)[0].reshape(1, 32)
            g["predictor.W3.bias"] = (dl if sh.alone else dl[sv.srt_eid.long()]).sum().reshape(1)   # (a shard: the edges scored here)
            W1 = tail["W1"]
            de = ops.linear(dz1, W1[:, 2 * H:].t().contiguous(), None)       # d e_final of the scored rows
            gW1e = ops.wgrad(dz1, tail["e_sc"])
            seg = sg.seg_views
            d_ps = ops.segment_sum(dz1, seg.out_ptr, seg.out_pos, n)         # gathered by srt_src in the forward
            d_qd = ops.segment_sum(dz1, seg.in_ptr, None, n)                 # gathered by srt_dst
            dPQ = torch.cat([d_ps, d_qd], 1)
            g["predictor.W1.bias"] = ops.colsum2(d_qd)[0]
            gWn = ops.wgrad(dPQ, tail["h"])                                  # [2hs, H]
            g["predictor.W1.weight"] = torch.cat([gWn[:hs], gWn[hs:], gW1e], 1)
            dh = ops.linear(dPQ, tail["W_nodes"].t().contiguous(), None)     # [N,H]
            if sg.score_gather is not None:   # directed=False: the scorer's de goes back to the rows it read, the reverse copies get none
                de = ops.scatter_add_rows(de, sg.score_gather, torch.zeros((E2, H), dtype=torch.float32, device=dev))

        # ---- layers, last to first (gated_gcn_full.py:182-230)
        if saved:
            sh.halo_bwd_start(dh)   # the halo rows travel under the kernels that do not read dh (the scorer's weight gradients above are done)
        for li in range(len(saved) - 1, -1, -1):
            s, conv, pfx = saved[li], model.gnn.convs[li], f"gnn.convs.{li}."
            A2, W3t = s["P"][:, H:2 * H], d(conv.B_3.weight).t().contiguous()
            sh.halo_bwd_finish(dh)
            if s["mask"] is not None:
                if whole:
                    dh = ops.mul23(dh, s["mask"], s["mask"])[0]
                else:
                    dh[:n_own].copy_(ops.mul23(dh[:n_own], s["mask"], s["mask"])[0])
            # h' = relu(norm_h(v)) + h_in      (owned rows; a halo row's dv is zero)
            dv = (torch.empty if n == n_own else torch.zeros)((n, H), dtype=torch.float32, device=dev)
            if s["sc_h"] is None:
                _, g[pfx + "bn_h.weight"], g[pfx + "bn_h.bias"] = ops.ln_bwd(dh[:n_own], s["v"], d(conv.bn_h.weight), d(conv.bn_h.bias), out=dv[:n_own])
            else:
                g[pfx + "bn_h.weight"], g[pfx + "bn_h.bias"] = train._bn_bwd(sh, dh[:n_own], s["v"], s["sc_h"], s["sh_h"], s["mean_h"], s["rstd_h"],
                                                                             sh.n_global, n_own, dv[:n_own])
            # v = A1h + fwd: the two node tables, then de += ... over the in-lists and dA2h over the out-lists
            Tf, Uf = ops.mul23(dv[:n_own], s["rdf"], s["hf"])
            if whole:
                dA2 = ops.node_aggregate_in_bwd(s["e_new"], Tf, Uf, A2, views, de)
            else:   # [n, H]: a halo source's row is this rank's partial sum over the local edges
                dA2 = ops.node_aggregate_in_bwd_part(s["e_new"], Tf, Uf, A2, views, de, n_own)
            # e' = relu(norm_e(xe)) + e_in ;  xe = B1h[src] + B2h[dst] + e_in W3^T
            amax_dxe = None
            if s["sc_e"] is None:
                dxe = torch.empty_like(de)
                _, g[pfx + "bn_e.weight"], g[pfx + "bn_e.bias"] = ops.ln_bwd(de, s["xe"], d(conv.bn_e.weight), d(conv.bn_e.bias), out=dxe)
            elif ops.can_fuse_bn_bwd_dgrad(de, W3t, s["xe"]):
                # BatchNorm backward and d e_in = d e' + dxe W3 in one pass over the edges, as in the symmetric step
                g[pfx + "bn_e.weight"], g[pfx + "bn_e.bias"], c1, c2 = train._bn_bwd(sh, de, s["xe"], s["sc_e"], s["sh_e"], s["mean_e"], s["rstd_e"],
                                                                                     sh.e_global, sh.e_own, None, apply=False)
                if train.SCALED_WGRAD and hasattr(ops, "can_dgrad_amax") and ops.can_dgrad_amax(de, s["xe"]):
                    amax_dxe = torch.empty(1, dtype=torch.int32, device=dev)
                dxe = ops.bn_bwd_dgrad(de, s["xe"], s["sc_e"], s["sh_e"], s["sc_e"], c1, c2, s["mean_e"], s["rstd_e"], W3t, rows_once=sh.e_own,
                                       **({"amax": amax_dxe} if amax_dxe is not None else {}))
                W3t = None
            else:
                dxe = torch.empty_like(de)
                g[pfx + "bn_e.weight"], g[pfx + "bn_e.bias"] = train._bn_bwd(sh, de, s["xe"], s["sc_e"], s["sh_e"], s["mean_e"], s["rstd_e"],
                                                                             sh.e_global, sh.e_own, dxe)
            if W3t is not None:
                ops.linear(dxe, W3t, None, out=de, accumulate=True)   # d e_in = d e' + dxe W3
            dB2, dB1 = ops.segment_sum2(dxe, views, n)   # B2h was gathered by srt_dst (the in-lists), B1h by srt_src (the out-lists): one launch
            parts = [dv, dA2, dB1, dB2]
            names = ("A_1", "A_2", "B_1", "B_2")
            WcatT = s["Wcat"].t().contiguous()
            if ops.can_use_blocks(parts):   # the four [N,H] gradients stay where their kernels left them
                dh = ops.linear_blocks(parts, WcatT, dh, accumulate=True)
                if li > 0:
                    sh.halo_bwd_start(dh)   # (layer 0's halo rows of h came from x: their dh stays here, for the node encoder's gradients)
                gWcat, gbcat = ops.wgrad_blocks(parts, s["h"])            # [4H, H], [4H]
                for k, name in enumerate(names):
                    g[pfx + name + ".bias"] = gbcat[k * H:(k + 1) * H]
            else:
                dP = torch.cat(parts, 1)
                dh = ops.linear(dP, WcatT, None, out=dh, accumulate=True)
                if li > 0:
                    sh.halo_bwd_start(dh)
                for k, name in enumerate(names):
                    g[pfx + name + ".bias"] = ops.colsum2(parts[k])[0]
                gWcat = ops.wgrad(dP, s["h"])
            for k, name in enumerate(names):
                g[pfx + name + ".weight"] = gWcat[k * H:(k + 1) * H]
            g[pfx + "B_3.weight"] = ops.wgrad(dxe, s["e"], amax=amax_dxe) if amax_dxe is not None else ops.wgrad(dxe, s["e"])
            g[pfx + "B_3.bias"] = g[pfx + "B_2.bias"].clone()   # every edge has exactly one destination: sum_p dxe[p] = sum_i dB2[i]
            saved[li] = s = None

        # ---- encoders (full_graph.py:44-45); directed=False: the 2E rows of de reach each original edge's features twice, summed by the products
        train.encoder_bwd(ops, g, dh, tail["x"], getattr(views, "node_gather", None), n, model.node_encoder.linear1, model.node_encoder.linear2,
                          "node_encoder.linear1", "node_encoder.linear2")
        train.encoder_bwd(ops, g, de, tail["e_raw"], sg.enc_gather, E2, model.edge_encoder.linear1, model.edge_encoder.linear2,
                          "edge_encoder.linear1", "edge_encoder.linear2")
        ctx.saved = ctx.tail = None
        return (None, None, None, None, None) + tuple(sh.sum_ranks([g[name].contiguous() for name in ctx.names]))


def train_forward_in_edge(model, graph, x, e):
    """`model(graph, x, e)` in train mode through the one-direction step (`GatedGCNModel.training_step = "in_edge"`), both `directed`
    values; logits [E,1] on the compute device, differentiable with respect to the model's parameters.  Served: fp32 storage, both
    norms, the built widths; a single process (one rank of a partition: train_forward_in_edge_on)."""
    _check_in_edge_step(model)
    device = engine.compute_device(x, e)
    names, params = zip(*model.named_parameters())
    if any(p.device != device for p in params):
        raise RuntimeError("training needs the model on the compute device: call model.to(device) first")
    views = views_for(graph, device, node_order="input")
    if x.shape[0] != views.num_nodes or e.shape[0] != views.num_edges:
        raise ValueError(f"x has {x.shape[0]} rows for {views.num_nodes} nodes, e has {e.shape[0]} rows for {views.num_edges} edges")
    xd = x.detach().to(device=device, dtype=torch.float32).contiguous()
    ed = e.detach().to(device=device, dtype=torch.float32).contiguous()
    out = _InEdgeStep.apply(model, _StepGraph(in_edge_views(views), bool(model.directed)), xd, ed, list(names), *params)
    views.check_range()
    return out


def train_forward_in_edge_on(model, shard, x_local, e_local):
    """The one-direction step over one rank's rows of an in-edge-only destination-range partition (dist.PartitionShard over
    PartitionedGraph.from_global(..., in_edges_only=True)); x_local / e_local: the input features of the shard's nodes (owned, then halo)
    and edges (local edge-id order).  Returns logits[E_global, 1], complete on every rank; after backward() every rank holds the whole
    graph's parameter gradients.  training_step="in_edge" only (dist.PartitionedRunner.train_forward checks it).  directed=False runs on a
    doubled plan (PartitionedGraph.from_global(..., in_edges_only=True, doubled=True)): the logits are [E, 1] over the ORIGINAL edge ids,
    e_local the plan's local_edge_rows of the original features; bn_e's statistics run over the 2E rows (the ranks' local rows sum to
    them through combine_stats), one momentum update per layer; the edge encoder's weight gradient sums both copies' de, each copy on
    the rank that owns it (sum_ranks)."""
    from .dist import check_doubled
    _check_in_edge_step(model)
    check_doubled(True, bool(model.directed), shard.part, None)
    if not getattr(shard.part, "in_edges_only", False):
        raise ValueError("GatedGCNModel runs on an in-edge-only partition: build it with PartitionedGraph.from_global(..., in_edges_only=True)")
    names, params = zip(*model.named_parameters())
    if any(p.device != x_local.device for p in params):
        raise RuntimeError("training needs the model on the compute device: call model.to(device) first")
    if x_local.shape[0] != shard.n_local or e_local.shape[0] != shard.e_local:
        raise ValueError(f"x has {x_local.shape[0]} rows for {shard.n_local} local nodes, e has {e_local.shape[0]} rows for {shard.e_local} local edges")
    return _InEdgeStep.apply(model, _StepGraph.on_shard(shard), x_local, e_local, list(names), *params)


def _check_in_edge_step(model):
    from .train import TRAIN_SCORE_HIDDEN
    check_arithmetic(model)
    if getattr(model, "activation_storage", "fp32") != "fp32":
        raise ValueError(f'training_step="in_edge" keeps activations as "fp32"; activation_storage={model.activation_storage!r} is served by '
                         'training_step="symmetric"')
    if getattr(model, "recompute_gate", False):
        raise ValueError('training_step="in_edge" keeps the gate output; recompute_gate is served by training_step="symmetric"')
    built_width(model.node_encoder.linear2.out_features)
    built_width(model.predictor.W1.out_features, TRAIN_SCORE_HIDDEN, "hidden_edge_scores")
