"""The edge-label contract (utils/labels.py) restated in plain Python / numpy, in linear time: the statement the device labels
(gnnome_amd/labels.py, csrc/edge_labels.hip) are checked against, itself anchored to the reference's recorded labels
(tests/golden/g14_labels.pt).

Per (chromosome, strand) problem, over its class edges G and their endpoints V, with hk = end (strand +1) or -start (strand -1):
    final = argmax_V hk ; reached = min_V hk ; alive = V
    while alive:
        a = the first alive node in cursor order (start ascending for +1, end descending for -1)
        F = nodes reachable from a in G[alive] ; h = argmax_F hk ; C = nodes that reach h in G[F]
        if |C| >= 2 and hk[h] >= reached: reached = hk[h], the class edges inside C get 1, stop if h == final
        alive -= F
Every argmin / argmax takes the smallest node id among equal keys.  CSR adjacency, a deque per traversal and a cursor that only moves
forward keep it O(N + E)."""
from collections import deque

import numpy as np


def class_edges(src, dst, strand, start, end, chrom):
    """bool[E] class-edge mask and int8[E] strand of the problem each class edge belongs to."""
    su, sv = strand[src], strand[dst]
    same = (chrom[src] == chrom[dst]) & (su == sv)
    pos = same & (su == 1) & (start[src] < start[dst]) & (start[dst] < end[src])
    neg = same & (su == -1) & (start[dst] < start[src]) & (start[src] < end[dst])
    return pos | neg


def _csr(a, b, n):
    order = np.argsort(a, kind="stable")
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(a, minlength=n), out=ptr[1:])
    return ptr, b[order]


def statement_labels(src, dst, num_nodes, strand, start, end, chrom, stats=None):
    """-> float32[E].  stats: a list that receives one dict per problem (chr, strand, nodes, class_edges, passes, accepted), in the
    order chromosome code ascending, strand -1 before +1."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    strand, chrom = np.asarray(strand, dtype=np.int64), np.asarray(chrom, dtype=np.int64)
    start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    n, E = int(num_nodes), src.size
    y = np.zeros(E, dtype=np.float32)
    cls = class_edges(src, dst, strand, start, end, chrom) if E else np.zeros(0, dtype=bool)
    cs, cd = src[cls], dst[cls]
    out_ptr, out_adj = _csr(cs, cd, n)
    in_ptr, in_adj = _csr(cd, cs, n)
    member = np.zeros(n, dtype=bool)
    member[cs] = member[cd] = True
    nodes = np.nonzero(member)[0]
    pkey = chrom[nodes] * 2 + (strand[nodes] > 0)
    hkey = np.where(strand > 0, end, -start)                  # maximised by the loop
    ckey = np.where(strand > 0, start, -end)                  # cursor order, ascending
    order = nodes[np.lexsort((nodes, ckey[nodes], pkey))]     # problem, cursor key, node id
    okey = chrom[order] * 2 + (strand[order] > 0)
    bounds = np.flatnonzero(np.diff(okey)) + 1
    fstamp = np.full(n, -1, dtype=np.int64)
    bstamp = np.full(n, -1, dtype=np.int64)
    comp = np.full(n, -1, dtype=np.int64)
    hk = hkey.tolist()
    for seg in np.split(order, bounds) if order.size else []:
        V = seg.tolist()
        final = min(V, key=lambda u: (-hk[u], u))
        reached = min(hk[u] for u in V)
        cursor, passes, accepted = 0, 0, 0
        while cursor < len(V):
            a = V[cursor]
            fstamp[a] = passes
            F, q = [a], deque([a])
            while q:
                u = q.popleft()
                for v in out_adj[out_ptr[u]:out_ptr[u + 1]].tolist():
                    if fstamp[v] == -1:
                        fstamp[v] = passes
                        F.append(v)
                        q.append(v)
            h = min(F, key=lambda u: (-hk[u], u))
            stop = False
            if not hk[h] < reached:
                bstamp[h] = passes
                C, q = [h], deque([h])
                while q:
                    u = q.popleft()
                    for v in in_adj[in_ptr[u]:in_ptr[u + 1]].tolist():
                        if fstamp[v] == passes and bstamp[v] == -1:
                            bstamp[v] = passes
                            C.append(v)
                            q.append(v)
                if len(C) >= 2:
                    reached = hk[h]
                    accepted += 1
                    comp[C] = passes
                    stop = h == final
            passes += 1
            if stop:
                break
            while cursor < len(V) and fstamp[V[cursor]] != -1:
                cursor += 1
        if stats is not None:
            u0 = V[0]
            stats.append({"chr": int(chrom[u0]), "strand": int(strand[u0]), "nodes": len(V),
                          "class_edges": int((out_ptr[seg + 1] - out_ptr[seg]).sum()), "passes": passes, "accepted": accepted})
    if E:
        cu, cv = comp[src], comp[dst]
        y[cls & (cu != -1) & (cu == cv)] = 1.0
    return y


def positioned_read_graph(num_reads, num_chr=2, seed=0, read_len=(8000, 16000), coverage=12, transitive=3, false_links=0.01,
                          gaps=100, contained=0.02, chain=False):
    """A synthetic graph of reads sampled at positions on `num_chr` chromosomes (codes 1.., and X = -1 for the last when
    num_chr > 2), both genome strands, as read_gfa numbers it: read k is node 2k with its strand and 2k+1 with the opposite, both
    with the read's start and end.  Links: each read to its next `transitive` overlapping successors along the genome, in both
    orientations (the mate of every link is written: u -> v and v^ -> u^), `false_links` of the links between random reads,
    `gaps` coverage gaps per chromosome (reads near a gap are dropped, so components end there), and `contained` reads lying
    inside another one.  chain=True: one chromosome, one strand, each read linked to the next only (the deepest traversal).
    -> dict(src, dst int64, num_nodes, read_strand, read_start, read_end, read_chr int64[N])."""
    rng = np.random.default_rng(seed)
    if chain:
        L = np.full(num_reads, 1000, dtype=np.int64)
        start = np.arange(num_reads, dtype=np.int64) * 500
        fasta_strand = np.ones(num_reads, dtype=np.int64)
        chrom = np.ones(num_reads, dtype=np.int64)
        a = np.arange(num_reads - 1)
        links = (a, a + 1)
    else:
        per = num_reads // num_chr
        starts, chroms = [], []
        for c in range(num_chr):
            glen = per * (read_len[0] + read_len[1]) // (2 * coverage)
            s = np.sort(rng.integers(0, glen, size=per))
            cuts = rng.integers(0, glen, size=gaps)
            keep = np.ones(per, dtype=bool)
            for x in cuts:                                    # no read starts within one read length before a cut
                keep &= ~((s > x - read_len[1]) & (s <= x))
            s = s[keep]
            starts.append(s)
            code = c + 1 if not (num_chr > 2 and c == num_chr - 1) else -1
            chroms.append(np.full(s.size, code, dtype=np.int64))
        start = np.concatenate(starts)
        chrom = np.concatenate(chroms)
        R = start.size
        L = rng.integers(read_len[0], read_len[1], size=R)
        inner = rng.random(R) < contained                    # contained reads: shorter, inside their predecessor
        L[inner] = read_len[0] // 4
        fasta_strand = np.where(rng.random(R) < 0.5, 1, -1)
        num_reads = R
        src_l, dst_l = [], []
        end = start + L
        for k in range(1, transitive + 1):
            a = np.arange(R - k)
            b = a + k
            ok = (chrom[a] == chrom[b]) & (start[b] < end[a]) & (start[a] < start[b])
            src_l.append(a[ok])
            dst_l.append(b[ok])
        a, b = np.concatenate(src_l), np.concatenate(dst_l)
        nf = int(false_links * a.size)
        fa, fb = rng.integers(0, R, size=nf), rng.integers(0, R, size=nf)
        ok = fa != fb
        links = (np.concatenate([a, fa[ok]]), np.concatenate([b, fb[ok]]))
        perm = rng.permutation(R)                             # read ids in no genome order
        inv = np.empty(R, dtype=np.int64)
        inv[perm] = np.arange(R)
        start, L, fasta_strand, chrom = start[perm], L[perm], fasta_strand[perm], chrom[perm]
        links = (inv[links[0]], inv[links[1]])
    end = start + L
    R = num_reads
    a, b = links
    # a genome-order link a -> b: the read-forward edge on the genome's + strand is (a, b) in the orientation each read has there:
    # node 2r carries the read's FASTA strand, so the + strand copy of read r is 2r when its strand is +1, else 2r+1
    pa = 2 * a + (fasta_strand[a] < 0)
    pb = 2 * b + (fasta_strand[b] < 0)
    src = np.concatenate([pa, pb ^ 1])
    dst = np.concatenate([pb, pa ^ 1])
    node_strand = np.empty(2 * R, dtype=np.int64)
    node_strand[0::2], node_strand[1::2] = fasta_strand, -fasta_strand
    pair = np.unique(np.stack([src, dst], 1), axis=0)
    pair = pair[pair[:, 0] != pair[:, 1]]
    return {"src": pair[:, 0].copy(), "dst": pair[:, 1].copy(), "num_nodes": 2 * R, "read_strand": node_strand,
            "read_start": np.repeat(start, 2), "read_end": np.repeat(end, 2), "read_chr": np.repeat(chrom, 2)}
