"""Overlap edit distances beyond one wavefront (overlap.edit_distances(long_overlaps=True), csrc/overlap_similarity.hip k_overlap_strips):
wall time per call with the device drained, RUNS runs after one warm-up call per shape.

    python tools/overlap_long_time.py [--out profiles/overlap_long_time.txt] [--default-only] [--root TREE]

Two seeded inputs:
  mixed   ~2 000 overlaps of 0.4-0.9 kb between reads laid out on one genome (2 % divergence) with three overlaps of 67-70 kb rows
          against ~1.2 kb targets interleaved at 1/4, 1/2 and 3/4 of the list
  square  one overlap of 66 000 x ~66 000 at 1 % divergence (the band gives up, two strips, the carry at full length)
Rows: the long entry on `mixed` and on `square`, and the DEFAULT entry on the short overlaps of `mixed` alone.  --default-only times
that last row only and never names the keyword, so the same file runs against another commit's build: --root TREE imports
gnnome_amd from TREE (its own lib/), which is how the default entry is compared before and after the strip pass was added."""
import argparse
import json
import os
import random
import sys
import time


def _random(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def _mutate(rng, s, rate):
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice("ACGT"))
            continue
        if r < rate:
            out.append(rng.choice("ACGT"))
        out.append(ch)
    return "".join(out)


def mixed(seed=61, short_reads=1001):
    rng = random.Random(seed)
    genome = _random(rng, 300 * short_reads + 2000)
    reads, pos = [], 0
    for _ in range(short_reads):
        ln = rng.randrange(400, 900)
        reads.append(_mutate(rng, genome[pos:pos + ln], 0.02))
        pos += ln // 3
    src, dst, ol = [], [], []
    for r in range(short_reads - 2):
        for t in (1, 2):
            flip = rng.random() < 0.3
            src.append(2 * r + (rng.randrange(2) if flip else 0)), dst.append(2 * (r + t) + (rng.randrange(2) if flip else 0))
            ol.append(rng.randrange(200, min(len(reads[r]), len(reads[r + t]))))
    big = _random(rng, 70_000)
    f = len(reads)
    reads += [big, _mutate(rng, big[66_000 - 900:66_000 + 300], 0.05), _mutate(rng, big[3_000:4_100], 0.05)]
    longs = [(2 * f, 2 * f + 2, 67_000), (2 * f + 1, 2 * f + 4, 69_999), (2 * f, 2 * f + 5, 70_000)]
    for k, (u, v, L) in enumerate(longs):
        at = (k + 1) * len(src) // 4
        src.insert(at, u), dst.insert(at, v), ol.insert(at, L)
    short = [i for i, L in enumerate(ol) if L <= 65_536]
    return reads, src, dst, ol, short


def square(seed=21):
    rng = random.Random(seed)
    shared = _random(rng, 66_000)
    return [_random(rng, 4_000) + shared, _mutate(rng, shared, 0.01) + _random(rng, 4_000)], [0], [2], [66_000]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "overlap_long_time.txt"))
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from gnnome_amd import overlap
    dev = torch.device("cuda", 0)
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    def timed(fn):
        fn()                                   # warm-up: code objects, allocator
        out = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            out.append(round((time.perf_counter() - t0) * 1e3, 3))
        return out, res

    emit(device=torch.cuda.get_device_name(0), runs=args.runs, label=args.label, package=os.path.dirname(os.path.abspath(overlap.__file__)),
         note="milliseconds per edit_distances call (packed reads already on the device), wall, device drained before and after")
    reads, src, dst, ol, short = mixed()
    packed = tuple(t.to(dev) for t in overlap.pack_reads(reads))
    s_src, s_dst, s_ol = ([x[i] for i in short] for x in (src, dst, ol))
    ms, (d_short, _) = timed(lambda: overlap.edit_distances(packed, s_src, s_dst, s_ol, device=dev, with_similarity=False))
    emit(case="mixed, short overlaps only, default entry", overlaps=len(short), ms=ms, checksum=int(d_short.sum()))
    if not args.default_only:
        st = {}
        ms, (d_all, _) = timed(lambda: overlap.edit_distances(packed, src, dst, ol, device=dev, with_similarity=False, stats=st, long_overlaps=True))
        same = d_all.cpu()[torch.tensor(short)].tolist() == d_short.cpu().tolist()
        emit(case="mixed, long entry", overlaps=len(src), ms=ms, strips=st["strips"], banded=st["banded"], short_equal_default=bool(same),
             long_distances=[int(d_all[i]) for i in range(len(src)) if ol[i] > 65_536])
        reads2, src2, dst2, ol2 = square()
        packed2 = tuple(t.to(dev) for t in overlap.pack_reads(reads2))
        st = {}
        ms, (d2, _) = timed(lambda: overlap.edit_distances(packed2, src2, dst2, ol2, device=dev, with_similarity=False, stats=st, long_overlaps=True))
        block_steps = 2 * (len(reads2[1][:66_000]) + 63) * 32      # ceil(m / (B * 2048)) strips of (n + 63) * B block steps
        emit(case="square 66 000 x 66 000, long entry", ms=ms, strips=st["strips"], distance=int(d2[0]), block_steps_per_wave=block_steps,
             ns_per_block_step=round(min(ms) * 1e6 / block_steps, 2))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
