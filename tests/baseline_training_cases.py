"""Helper of the GCNModel / SAGEModel training tests (tests/test_baseline_training_statement.py, test_baseline_training.py): a plain-torch,
differentiable restatement of both models in TRAIN mode.  It is baseline_graphs.baseline_model plus SAGEConv's feat_drop: one scaled
keep-mask per layer (Bernoulli(1 - p) / (1 - p)), applied to the layer's input before both the self and the neighbour path (DGL 0.8.1's
SAGEConv: feat_src = feat_dst = feat_drop(feat)).  GraphConv has no dropout.  Written from the formulas, as baseline_graphs.py is."""
import torch
import torch.nn.functional as F

import baseline_graphs as bg


def seeded_masks(n, hidden, p, count, seed):
    """`count` scaled keep-masks [n, hidden] of F.dropout(., p, training=True) from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, hidden, generator=g) >= p).float() / (1.0 - p) for _ in range(count)]


def baseline_model_train(kind, sd, src, dst, n, x, e, num_layers, directed=True, masks=None):
    """Logits [E,1] of GCNModel / SAGEModel in train mode from a state dict (leaves that require grad are differentiated through);
    masks: per layer a [n, H] tensor or None (SAGE only; None everywhere = no dropout)."""
    src, dst = src.long(), dst.long()
    enc = lambda p, t: F.linear(torch.relu(F.linear(t, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])), sd[p + ".linear2.weight"],  # noqa: E731
                                sd[p + ".linear2.bias"])
    h, ee = enc("node_encoder", x), enc("edge_encoder", e)
    layer = bg.gcn_layer if kind == "gcn" else bg.sage_layer
    for i in range(num_layers):
        if kind == "sage" and masks is not None and masks[i] is not None:
            h = h * masks[i]
        h = layer(sd, f"gnn.convs.{i}.", src, dst, n, h, directed)
        if i + 1 < num_layers:
            h = torch.relu(h)
    z = torch.relu(F.linear(torch.cat([h[src], h[dst], ee], 1), sd["predictor.W1.weight"], sd["predictor.W1.bias"]))
    z = torch.relu(F.linear(z, sd["predictor.W2.weight"], sd["predictor.W2.bias"]))
    return F.linear(z, sd["predictor.W3.weight"], sd["predictor.W3.bias"])


class MaskFeed:
    """Stands in for gnnome_amd.train.dropout_mask: hands out the given masks in order, on the asked device."""

    def __init__(self, masks):
        self.masks, self.calls = list(masks), 0

    def __call__(self, rows, cols, p, device):
        m = self.masks[self.calls]
        self.calls += 1
        assert m.shape == (rows, cols)
        return m.to(device).contiguous()
