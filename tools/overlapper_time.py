"""Times gnnome_amd.overlapper on synthetic reads: a random genome read at 20x by error-free reads of one length on both strands
(default 10 000 reads x 15 000 bases).  Every figure is a host clock around a call that ends in a device synchronise, after a warm-up
call of the same shapes; the median of --repeats calls is reported.

    python tools/overlapper_time.py [--reads 10000 --length 15000 --k 19 --w 10 --repeats 5 --statement-reads 200]

Sketch: input bytes per second of the whole sketch_reads call, and the share of the HBM figure the project uses (8 TB/s) that the
kernel's own traffic - every base twice, once per launch - amounts to.  A further pass with stats= takes device-event times of every
stage (the median over the repeats): for the sketch the count stage (count launch, scan, size read-back) and the write launch alone - the
write launch's bytes per second is the one figure that is a single kernel's; for find_overlaps the record kernel and the chain kernel
as records per second, and torch's sorts beside them; for simplify.simplify_graph on the graph of these overlaps the edge and node
counts before and after and its stages (mates check, the sort and the mark kernel of the transitive rule, the lists and the two launches
of the tips, the compaction); for unitigs.compact_unitigs on the simplified graph its stages (checks and degrees, the link kernel, the
ranking with its round count, the numbering, the scatter kernel, the edge gathers, the spelling, the host name tables) and, beside the
ranking, the same pointer jumping written as torch gathers (torch_pointer_jumping below: one record per node, one jump per round, the
same count read back per round), whose ranks must equal the kernel's; with --bubbles SITES the reads come from two haplotypes that differ
at SITES places and bubbles.pop_bubbles on the simplified graph is timed as well (its stages added up over the rounds, the arms, what is
removed, the share of the ranking in the stage times) - without the flag nothing changes.  The only baseline is the NumPy / Python statement
(tests/overlap_graph_statement.py) on the first --statement-reads reads of the same input, a host wall time labelled as such.
Prints one JSON line."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8e12
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def make_reads(n, length, coverage, seed, sites=0, site_length=2000):
    """sites > 0: a second haplotype that differs from the first in `sites` evenly spaced stretches of site_length random bases - longer
    than max_hang, so reads of different haplotypes do not dovetail across a site - and a haplotype bit per read, drawn after everything
    else."""
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, max(n * length // coverage, 2 * length))]
    start = rng.integers(0, len(genome) - length + 1, n)
    flip = rng.integers(0, 2, n).astype(bool)
    haplotypes, hap = [genome], np.zeros(n, dtype=np.int64)
    if sites:
        other = genome.copy()
        for at in np.linspace(0, len(genome) - site_length, sites + 2)[1:-1].astype(np.int64).tolist():
            other[at:at + site_length] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, site_length)]
        haplotypes.append(other)
        hap = rng.integers(0, 2, n)
    data = np.empty(n * length, dtype=np.uint8)
    for i, (s, f) in enumerate(zip(start.tolist(), flip.tolist())):
        piece = haplotypes[hap[i]][s:s + length]
        data[i * length:(i + 1) * length] = _COMP[piece[::-1]] if f else piece
    return torch.from_numpy(data), torch.arange(n + 1, dtype=torch.int64) * length


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times), out


def torch_pointer_jumping(pred, weight):
    """The ranking of csrc/unitigs.hip as torch gathers, for comparison: pred int64[N] (-1: a head), weight int64[N] (the p of a node's
    out-link) -> (head, rank, offset, rounds).  Paths only: a cycle leaves unfinished nodes and raises."""
    node = torch.arange(pred.numel(), device=pred.device)
    has = pred >= 0
    anc = torch.where(has, pred, node)
    hops = has.long()
    bases = torch.where(has, weight[anc], torch.zeros_like(weight))
    done = pred[anc] < 0
    left, rounds = int((~done).sum()), 0
    while left:
        hops = torch.where(done, hops, hops + hops[anc])
        bases = torch.where(done, bases, bases + bases[anc])
        anc = torch.where(done, anc, anc[anc])
        done = pred[anc] < 0
        before, left, rounds = left, int((~done).sum()), rounds + 1
        if left >= before:
            raise SystemExit("torch_pointer_jumping: the count of unfinished nodes stopped falling: the graph has a cycle")
    return anc, hops, bases, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--length", type=int, default=15000)
    ap.add_argument("--coverage", type=int, default=20)
    ap.add_argument("--k", type=int, default=19)
    ap.add_argument("--w", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--statement-reads", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--bubbles", type=int, default=0, metavar="SITES",
                    help="read a diploid genome whose haplotypes differ at SITES places and time the bubble stages too (0: off)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlapper_time: no GPU - nothing is measured without one")
    from gnnome_amd import overlapper
    dev = torch.device("cuda", 0)
    data, off = make_reads(a.reads, a.length, a.coverage, a.seed, a.bubbles)
    reads = (data.to(dev), off.to(dev))
    nbytes = int(data.numel())
    sk_t, sk_lo, sk_hi, sk = timed(lambda: overlapper.sketch_reads(reads, a.k, a.w), a.repeats)
    ov_t, ov_lo, ov_hi, ov = timed(lambda: overlapper.find_overlaps(reads, sk), a.repeats)
    P, kept = int(ov.records[0].numel()), len(ov)
    sk_stats, ov_stats = [], []
    for _ in range(a.repeats):
        sk_stats.append({})
        ov_stats.append({})
        overlapper.find_overlaps(reads, overlapper.sketch_reads(reads, a.k, a.w, stats=sk_stats[-1]), stats=ov_stats[-1])
    stage = lambda runs: {key: statistics.median(r[key] for r in runs) for key in runs[0] if key.endswith("_ms")}   # noqa: E731
    sk_ms, ov_ms = stage(sk_stats), stage(ov_stats)
    from gnnome_amd import _lib
    with open(_lib.LIB_PATH, "rb") as f:
        so_sha16 = hashlib.sha256(f.read()).hexdigest()[:16]
    out = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip(),
           "so_sha16": so_sha16,
           "reads": a.reads, "length": a.length, "k": a.k, "w": a.w, "input_bytes": nbytes, "minimizers": len(sk), "seed_pairs": P,
           "overlaps_kept": kept,
           "sketch_call_s": sk_t, "sketch_call_s_min_max": [sk_lo, sk_hi], "sketch_input_bytes_per_s": nbytes / sk_t,
           "sketch_share_of_hbm_2_reads_per_base": 2 * nbytes / sk_t / HBM_BYTES_PER_S,
           "sketch_stage_ms": sk_ms, "sketch_write_launch_bytes_per_s": nbytes / (sk_ms["write_ms"] * 1e-3),
           "sketch_write_launch_share_of_hbm": nbytes / (sk_ms["write_ms"] * 1e-3) / HBM_BYTES_PER_S,
           "find_overlaps_stage_ms": ov_ms, "groups": ov_stats[0]["groups"],
           "pair_kernel_records_per_s": P / (ov_ms["pairs_write_ms"] * 1e-3), "chain_kernel_records_per_s": P / (ov_ms["chain_ms"] * 1e-3),
           "find_overlaps_call_s": ov_t, "find_overlaps_call_s_min_max": [ov_lo, ov_hi], "find_overlaps_records_per_s": P / ov_t}
    del ov
    # the graph of these overlaps and simplify.simplify_graph on it: its stages by device events, the whole call by the host clock
    from gnnome_amd import simplify
    g = overlapper.overlap_graph(reads, sk, similarity=False)
    del sk
    g.pop("overlaps")
    sg_t, sg_lo, sg_hi, sg = timed(lambda: simplify.simplify_graph(g), a.repeats)
    sg_stats = []
    for _ in range(a.repeats):
        sg_stats.append({})
        simplify.simplify_graph(g, stats=sg_stats[-1])
    out.update(graph_edges=int(g["src"].numel()), graph_nodes=int(g["num_nodes"]), graph_max_out_degree=int(torch.bincount(g["src"]).max()),
               simplified_edges=int(sg["src"].numel()), simplified_nodes=int(sg["num_nodes"]), simplify_removed=sg["removed"],
               simplified_max_out_degree=int(torch.bincount(sg["src"]).max()) if sg["src"].numel() else 0,
               simplify_stage_ms=stage(sg_stats), simplify_call_s=sg_t, simplify_call_s_min_max=[sg_lo, sg_hi])
    # unitigs.compact_unitigs on the simplified graph, and the ranking once more as torch gathers
    from gnnome_amd import unitigs
    ug_t, ug_lo, ug_hi, ug = timed(lambda: unitigs.compact_unitigs(sg), a.repeats)
    ug_stats = []
    for _ in range(a.repeats):
        ug_stats.append({})
        unitigs.compact_unitigs(sg, stats=ug_stats[-1])
    src, dst, p, N = sg["src"], sg["dst"], sg["prefix_length"], sg["num_nodes"]
    link = (torch.bincount(src, minlength=N)[src] == 1) & (torch.bincount(dst, minlength=N)[dst] == 1) & ((src >> 1) != (dst >> 1))
    pred, weight = torch.full((N,), -1, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)
    pred[dst[link]] = src[link]
    weight[src[link]] = p[link]
    tj_t, tj_lo, tj_hi, (_, tj_rank, tj_offset, tj_rounds) = timed(lambda: torch_pointer_jumping(pred, weight), a.repeats)
    chains = unitigs.unitig_chains(sg)
    sizes = chains["chain_off"][1:] - chains["chain_off"][:-1]
    out.update(unitig_nodes=int(ug["num_nodes"]), unitig_edges=int(ug["src"].numel()), unitig_links=int(chains["link"].sum()),
               unitig_longest_chain=int(sizes.max()) if sizes.numel() else 0, unitig_circular=int(ug["circular"].sum()),
               unitig_rank_rounds=ug_stats[0]["rank_rounds"], unitig_stage_ms=stage(ug_stats), unitig_call_s=ug_t,
               unitig_call_s_min_max=[ug_lo, ug_hi], torch_rank_wall_ms=tj_t * 1e3, torch_rank_wall_ms_min_max=[tj_lo * 1e3, tj_hi * 1e3],
               torch_rank_rounds=tj_rounds,
               torch_rank_matches=bool(torch.equal(tj_rank.int(), chains["rank"]) and torch.equal(tj_offset, chains["offset"])))
    if a.bubbles:
        # bubbles.pop_bubbles on the simplified graph: its stages by device events, added up over the rounds, and the ranking's share
        from gnnome_amd import bubbles
        bb_t, bb_lo, bb_hi, bb = timed(lambda: bubbles.pop_bubbles(sg), a.repeats)
        bb_stats = []
        for _ in range(a.repeats):
            bb_stats.append({})
            bubbles.pop_bubbles(sg, stats=bb_stats[-1])
        bb_ms = stage(bb_stats)
        arms = bubbles.bubble_arms(sg)
        out.update(bubble_sites=a.bubbles, bubble_arms=int(arms["first"].numel()), bubble_longest_arm=int(arms["nodes"].max()) if arms["first"].numel() else 0,
                   bubble_removed=bb["removed"], bubble_edges_left=int(bb["src"].numel()),
                   bubble_max_out_degree_left=int(torch.bincount(bb["src"]).max()) if bb["src"].numel() else 0,
                   bubble_rank_rounds=bb_stats[0]["rank_rounds"], bubble_stage_ms=bb_ms, bubble_call_s=bb_t, bubble_call_s_min_max=[bb_lo, bb_hi],
                   bubble_ranking_share=sum(v for k, v in bb_ms.items() if k.startswith("unitig_")) / sum(bb_ms.values()))
        del bb
    del g, sg, ug
    if a.statement_reads:
        import overlap_graph_statement as st
        n = min(a.statement_reads, a.reads)
        host = data[:n * a.length].numpy().tobytes()
        sub = [host[i * a.length:(i + 1) * a.length] for i in range(n)]
        t0 = time.perf_counter()
        st.sketch(sub, a.k, a.w)
        t1 = time.perf_counter()
        st.overlaps(sub, k=a.k, w=a.w)
        t2 = time.perf_counter()
        out.update(statement_reads=n, statement_sketch_wall_s=t1 - t0, statement_overlaps_wall_s=t2 - t1,
                   statement_sketch_bytes_per_s=n * a.length / (t1 - t0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
