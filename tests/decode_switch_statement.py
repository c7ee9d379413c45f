"""Plain-Python statement of the greedy decode WITH the reference's two switches (inference.py:26-28): `early_stopping` /
`p_threshold` (:98-100, :142-145) and `RANDOM` (:59-61, :102-104, :147-149, :432).  TEST INFRASTRUCTURE ONLY: the checker of
gnnome_greedy_walks_opts (csrc/decode.hip) and of the keywords of gnnome_amd/decode.py.

Dicts, sets and torch's CPU kernels, like the reference and like oracle/decode_oracle.py, which supplies the unchanged parts
(neighbor_dicts, contig_length, sample_edges).  With both switches off every function here returns what the oracle returns.

Early stopping is the reference's own expression, `(neighbor_p < math.log(p_threshold)).all()`: an fp32 tensor against a Python
double, which torch compares in fp32 after rounding the double to fp32 (tests/test_decode_switches_host.py pins that), so a
log-probability EQUAL to the rounded threshold is not below it.  It is reached only in the ranked branch: a successor list of
length 2 or more with at least one admissible successor.  tests/golden/g19_decode_switches.pt holds walks of the reference's own
functions with early_stopping = True; the statement is held to them exactly.

Random mode cannot be the reference's: it draws torch.randint from the CPU generator once per step, one candidate after the
other.  The statement's draw - and the kernel's - is a pure function of (seed, candidate index, half, step):

    key  = candidate << 32 | half << 31 | step          half: 0 forward, 1 backward; step: the iteration of the walk loop,
                                                        i.e. the position of the current node in the half's walk
    u    = the (key + 1)-th output of splitmix64 seeded with `seed`: mix64(seed + (key + 1) * 0x9E3779B97F4A7C15 mod 2^64)
    j    = ((u >> 32) * n) >> 32                        multiply-shift of the top 32 bits onto [0, n)

and the walk takes the j-th of the n admissible successors in list order, adding that successor's own log-probability.
"""
import math

import torch

from oracle import decode_oracle as oracle

M64 = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15


def mix64(z):
    """The finaliser of splitmix64 (Steele, Lea, Flood 2014), on Python integers."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, candidate, half, step, n):
    assert 0 <= candidate < 2 ** 31 and half in (0, 1) and 0 <= step < 2 ** 31 and 0 < n < 2 ** 31
    key = (candidate << 32) | (half << 31) | step
    u = mix64((seed & M64) + (key + 1) * GOLDEN_GAMMA)
    return ((u >> 32) * n) >> 32


def launch_seed(seed, iteration):
    """The kernel seed of outer iteration `iteration` (= the number of contigs found so far, the reference's idx_contig):
    the (iteration + 1)-th output of splitmix64 seeded with `seed`."""
    return mix64((seed & M64) + (iteration + 1) * GOLDEN_GAMMA)


class Switches:
    def __init__(self, early_stopping=False, p_threshold=0.06, random_walks=False, seed=0):
        self.early_stopping, self.p_threshold, self.random_walks, self.seed = early_stopping, p_threshold, random_walks, seed


def _walk(start, logProbs, neighbors, edges, visited_old, sw, candidate, half, events=None):
    """inference.py:72-111 / :116-156 with the switches read from `sw`.  events: a list that receives one word per ranked step
    ('stop', 'rank', 'random') and 'single' per single-successor step taken, with the list length and the admissible count."""
    current = start
    walk = []
    visited = set()
    sumLogProb = torch.tensor([0.0])
    step = -1
    while True:
        step += 1
        walk.append(current)
        visited.add(current)
        visited.add(current ^ 1)
        neighs_current = neighbors[current]
        if len(neighs_current) == 0:
            break
        if len(neighs_current) == 1:
            neighbor = neighs_current[0]
            if neighbor in visited_old or neighbor in visited:
                break
            sumLogProb += logProbs[edges[current, neighbor]]
            if events is not None:
                events.append(("single", 1, 1, float(logProbs[edges[current, neighbor]])))
            current = neighbor
            continue
        masked_neighbors = [n for n in neighs_current if not (n in visited_old or n in visited)]
        neighbor_edges = [edges[current, n] for n in masked_neighbors]
        if not neighbor_edges:
            break
        neighbor_p = logProbs[neighbor_edges]
        if sw.early_stopping:
            if (neighbor_p < math.log(sw.p_threshold)).all().item():
                if events is not None:
                    events.append(("stop", len(neighs_current), len(masked_neighbors), float(neighbor_p.max())))
                return walk, visited, sumLogProb
        if sw.random_walks:
            index = draw(sw.seed, candidate, half, step, neighbor_p.shape[0])
            logProb = neighbor_p[index:index + 1]
        else:
            logProb, index = torch.topk(neighbor_p, k=1, dim=0)
        if events is not None:
            events.append(("random" if sw.random_walks else "rank", len(neighs_current), len(masked_neighbors), float(neighbor_p.max())))
        sumLogProb += logProb
        current = masked_neighbors[index]
    return walk, visited, sumLogProb


def run_greedy_both_ways(src, dst, logProbs, succs, preds, edges, visited, sw=None, candidate=0, events=None):
    """inference.py:160-164.  events: {'f': [...], 'b': [...]} to be filled, or None."""
    sw = sw or Switches()
    tmp_visited = visited | {src, src ^ 1, dst, dst ^ 1}
    walk_f, visited_f, sum_f = _walk(dst, logProbs, succs, edges, tmp_visited, sw, candidate, 0, None if events is None else events["f"])
    walk_b, visited_b, sum_b = _walk(src ^ 1, logProbs, succs, edges, tmp_visited | visited_f, sw, candidate, 1,
                                     None if events is None else events["b"])
    walk_b = list(reversed([w ^ 1 for w in walk_b]))
    return walk_f, walk_b, visited_f, visited_b, sum_f, sum_b


def sample_edges_uniform(prob_edges, nb_paths):
    """inference.py:56-61 with RANDOM = True: the 2^24 cut, then torch.randint from the CPU generator."""
    if prob_edges.shape[0] > 2 ** 24:
        prob_edges = prob_edges[:2 ** 24]
    return torch.randint(0, prob_edges.shape[0], (nb_paths,))


def candidate_figures(src, dst, len_walk, len_contig, sum_f, sum_b):
    """What the reference prints per candidate (inference.py:267-296): Python doubles from the fp32 sums' .item()s.
    -> (len_walk, len_contig, sumLogProb, meanLogProb, meanLogProb_scaled).  A contig length that is not positive gives
    scaled 0 (the reference's `except ValueError` branch; for 0 it would divide by zero)."""
    sumLogProb = float(sum_f) + float(sum_b)
    if src == dst:
        len_walk = 1
    if len_walk > 2:
        mean = sumLogProb / (len_walk - 2)
        scaled = mean / math.sqrt(len_contig) if len_contig > 0 else 0.0
    elif len_walk == 2:
        mean = 0.0
        scaled = mean / math.sqrt(len_contig) if len_contig > 0 else 0.0
    else:
        len_contig, sumLogProb, mean, scaled = 0, 0.0, 0.0, 0.0
    return len_walk, len_contig, sumLogProb, mean, scaled


def get_contigs_greedy(src, dst, num_nodes, scores, prefix_length, read_length, len_threshold, nb_paths=50, sampler=None,
                       trace=None, sw=None):
    """oracle.get_contigs_greedy (inference.py:193-359) with the switches.  random_walks: start edges by sample_edges_uniform
    unless a sampler is given, candidate e of outer iteration i walks with launch_seed(sw.seed, i) and candidate index e; as in
    the reference, `results` is a dict keyed by (src, dst): a later candidate on the same start edge replaces the earlier one's
    walks and keeps its place."""
    sw = sw or Switches()
    sampler = sampler or (sample_edges_uniform if sw.random_walks else oracle.sample_edges)
    succs, preds, edges = oracle.neighbor_dicts(src, dst, num_nodes)
    logProbs = torch.log(torch.sigmoid(scores.float()))
    src_l, dst_l = src.tolist(), dst.tolist()
    all_contigs, visited = [], set()
    iteration = -1
    while True:
        iteration += 1
        remaining = [k for k in range(len(src_l)) if src_l[k] not in visited and dst_l[k] not in visited]
        if not remaining:
            break
        idx_edges = sampler(torch.sigmoid(scores.float()[remaining]), nb_paths)
        it_sw = Switches(sw.early_stopping, sw.p_threshold, sw.random_walks, launch_seed(sw.seed, iteration))
        results = {}
        for e, idx in enumerate(torch.as_tensor(idx_edges).tolist()):
            s, d = src_l[remaining[idx]], dst_l[remaining[idx]]
            results[(s, d)] = run_greedy_both_ways(s, d, logProbs, succs, preds, edges, visited, it_sw, candidate=e)
        all_walks, all_visited_iter, all_contig_lens = [], [], []
        for k, (walk_f, walk_b, visited_f, visited_b, _, _) in results.items():
            walk_it = walk_b + walk_f
            len_contig_it = oracle.contig_length(walk_it, edges, prefix_length, read_length)
            if k[0] == k[1]:
                len_contig_it = 0
            all_walks.append(walk_it)
            all_visited_iter.append(visited_f | visited_b)
            all_contig_lens.append(len_contig_it)
        best = max(all_contig_lens)
        idxx = all_contig_lens.index(best)
        best_walk, best_visited = all_walks[idxx], all_visited_iter[idxx]
        trans = set()
        for ss, dd in zip(best_walk[:-1], best_walk[1:]):
            t1 = set(succs[ss]) & set(preds[dd])
            trans = trans | t1 | {t ^ 1 for t in t1}
        best_visited = best_visited | trans
        if trace is not None:
            trace.append({"contig_len": best, "walk_len": len(best_walk), "candidates": len(results)})
        if best < len_threshold:
            break
        all_contigs.append(best_walk)
        visited |= best_visited
    return all_contigs
