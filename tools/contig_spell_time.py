"""Time contig spelling (gnnome_amd/contigs.py, csrc/contig_spell.hip) on a synthetic assembly with >= 1 GB of FASTA output.

    python tools/contig_spell_time.py [--gbytes 1.2] [--reps 10] [--out-dir DIR]

Reports, as one JSON line: the copy kernel's time from device events (gnnome_contig_spell, line_width 60) and of the checked piece
pass (gnnome_contig_pieces: two kernels and one stream synchronise), the bytes the copy moves (output written + bytes read from the
read store + per-step metadata: node id, piece offset, two read offsets) and that figure as a fraction of 8 TB/s, then - measured
separately - the device-to-host copy of the file image and the file write.  Needs the MI355X; there is no CPU path."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnome_amd import contigs  # noqa: E402
from gnnome_amd.decode import DecodeGraph  # noqa: E402

HBM_BYTES_PER_S = 8e12


def build(gbytes, seed=0):
    """64 reads of 1 MiB (both strands used), every node linked to three others with prefixes of 0.5-1 MiB, walks long enough
    for `gbytes` of sequence; a few hundred short walks as well, so that contig lengths span orders of magnitude."""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed)
    R, L = 64, 1 << 20
    data = torch.from_numpy(rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=R * L)).to(dev)
    store = contigs.ReadStore(data, (torch.arange(R + 1, dtype=torch.int64) * L).to(dev))
    n = 2 * R
    src = [u for u in range(n) for d in (2, 4, 7)]
    dst = [(u + d) % n for u in range(n) for d in (2, 4, 7)]
    prefix = rng.integers(L // 2, L, size=len(src))
    dg = DecodeGraph(src, dst, n, prefix, [L] * n, device=dev)
    succ = [[] for _ in range(n)]
    for u, v in zip(src, dst):
        succ[u].append(v)
    walks, total = [], 0
    for k in range(400):                                     # short contigs: 1 to 3 reads
        w = [int(rng.integers(n))]
        for _ in range(k % 3):
            w.append(int(rng.choice(succ[w[-1]])))
        walks.append(w)
    while total < gbytes * 1e9:                              # long contigs of ~100 Mbp each
        w = [int(rng.integers(n))]
        for _ in range(130):
            w.append(int(rng.choice(succ[w[-1]])))
        walks.append(w)
        total += 130 * 0.75 * L
    return dg, walks, store


def events_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbytes", type=float, default=1.2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out-dir", default=None, help="where the FASTA file is written (default: a temporary directory)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X")
    dg, walks, store = build(args.gbytes)
    c = contigs.spell_contigs(dg, walks, store, line_width=60)        # warm-up: pieces, scan, headers, copy
    fasta = c.respell(60)
    torch.cuda.synchronize()
    plan = c._plan
    W, S = len(c), int(plan["nodes"].numel())
    unwrapped = int(c.offsets[-1])
    image = int(fasta.data.numel())
    body_off = torch.from_numpy(fasta.body_off).to(dg.device)
    from gnnome_amd import _lib
    from gnnome_amd.ops import _ptr, _stream
    lib = _lib.load()

    def spell():
        _lib.check(lib.gnnome_contig_spell(_ptr(plan["nodes"]), S, _ptr(plan["walk_off"]), W, _ptr(plan["piece_off"]), _ptr(store.data),
                                           _ptr(store.off), store.num_reads, _ptr(body_off), 60, _ptr(fasta.data), image,
                                           _stream(dg.device)), "contig_spell")

    spell()
    kernel = events_ms(spell, args.reps)
    pieces = events_ms(lambda: _pieces_only(lib, dg, plan, store), max(3, args.reps // 2))
    moved = image + unwrapped + S * (4 + 8 + 16) + W * 16
    t = time.perf_counter()
    host = fasta.fasta_bytes()
    d2h = time.perf_counter() - t
    with tempfile.TemporaryDirectory(dir=args.out_dir) as d:
        path = os.path.join(d, "assembly.fasta")
        t = time.perf_counter()
        with open(path, "wb") as f:
            host.tofile(f)
            f.flush()
            os.fsync(f.fileno())
        write = time.perf_counter() - t
    kmed = float(np.median(kernel))
    print(json.dumps({
        "what": "contig_spell", "walks": W, "steps": S, "unwrapped_bytes": unwrapped, "fasta_bytes": image,
        "spell_kernel_ms_median": round(kmed, 3), "spell_kernel_ms_min": round(min(kernel), 3),
        "bytes_moved": moved, "achieved_GBps": round(moved / kmed / 1e6, 1), "fraction_of_8TBps": round(moved / (kmed * 1e-3) / HBM_BYTES_PER_S, 4),
        "pieces_ms_median": round(float(np.median(pieces)), 3),
        "d2h_s": round(d2h, 3), "d2h_GBps": round(image / d2h / 1e9, 2), "file_write_s": round(write, 3),
        "file_write_GBps": round(image / write / 1e9, 2)}))


def _pieces_only(lib, dg, plan, store):
    """gnnome_contig_pieces alone (its checks synchronise the stream)."""
    import ctypes
    from gnnome_amd import _lib
    from gnnome_amd.ops import _ptr, _stream
    nodes, walk_off = plan["nodes"], plan["walk_off"]
    W, S = int(walk_off.numel()) - 1, int(nodes.numel())
    need = ctypes.c_size_t(0)
    _lib.check(lib.gnnome_contig_pieces_workspace_bytes(W, S, ctypes.byref(need)), "workspace")
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=dg.device)
    piece_len = torch.empty(S, dtype=torch.int64, device=dg.device)
    _lib.check(lib.gnnome_contig_pieces(_ptr(nodes), S, _ptr(walk_off), W, _ptr(dg.succ_ptr), _ptr(dg.succ_nbr), _ptr(dg.succ_eid),
                                        _ptr(dg.prefix_length), dg.num_nodes, _ptr(store.off), store.num_reads, _ptr(piece_len), _ptr(ws),
                                        ws.numel(), _stream(dg.device)), "contig_pieces")


if __name__ == "__main__":
    main()
