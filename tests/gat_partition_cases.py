"""Helpers of the partitioned GATModel tests (test_dist_gat_gloo.py, test_hip_gat_partition.py): the model, the configurations every
(graph, world) pair runs, and a counter of a shard's exchange calls.  The graphs, the full shard of a rank and the handed masks are those
of baseline_partition_graphs (read, not changed)."""
import baseline_graphs as bg
from baseline_partition_graphs import HIDDEN, LAYERS, SCORE_HIDDEN, HandedMasks, known_masks  # noqa: F401

DROPOUT = 0.25
# (directed, dropout): both `directed` values without dropout, and once with feat_drop masks handed to both runs
CONFIGS = [(True, 0.0), (False, 0.0), (True, DROPOUT)]


def model(directed=True, dropout=0.0, seed=8):
    from gnnome_amd.models import GATModel
    m = GATModel(2, 2, HIDDEN, 16, LAYERS, SCORE_HIDDEN, "batch", dropout=dropout, directed=directed)
    m.load_state_dict(bg.random_state_dict(m, seed=seed))
    return m


class CountedExchanges:
    """Wraps the exchange calls of dist.HaloExchange while it is active: `starts` = the width of every forward-direction exchange
    started, in order; `transposes` = how many halo transposes."""

    def __init__(self):
        self.starts, self.transposes = [], 0

    def __enter__(self):
        from gnnome_amd import dist as gdist
        self._cls, self._start, self._tstart = gdist.HaloExchange, gdist.HaloExchange.start, gdist.HaloExchange.transpose_start
        counter = self

        def start(xchg, h):
            counter.starts.append(int(h.shape[1]))
            return counter._start(xchg, h)

        def transpose_start(xchg, dh):
            counter.transposes += 1
            return counter._tstart(xchg, dh)

        self._cls.start, self._cls.transpose_start = start, transpose_start
        return self

    def __exit__(self, *exc):
        self._cls.start, self._cls.transpose_start = self._start, self._tstart
        return False
