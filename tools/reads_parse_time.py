"""Reads files: the host readers (contigs._records' per-line loop and gfa._node_annotations' regex per read, the code path every
earlier commit has) against the device reader (gnnome_amd/reads.py, csrc/reads_parse.hip) on the same box, three runs each, wall time
with the device drained.

    python tools/reads_parse_time.py [--out profiles/reads_parse_time.txt] [--dir /tmp/reads_parse_time]

Three synthetic files with a fixed seed:
  fastq   20 000 reads x 15 kb, four-line FASTQ, ~600 MB
  fasta   the same reads as a 60-column FASTA, ~305 MB
  short   500 000 records of 60-140 bases with strand= / start= / end= / chr= titles (the training path), FASTA, ~85 MB
Timed on each: ReadStore.from_reads_file with keep=None and with a 5 % keep, and read_gfa(training=True, labels=False) on a GFA that
names every read with '*' sequences - parser / reads_parser "host" against "device".  "host" runs exactly the code the parent commit
runs (those function bodies are untouched), so its rows are the baseline; the device rows are never compared to themselves."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnome_amd import contigs, gfa, reads  # noqa: E402

RUNS = 3


def _title(r, rng):
    start = int(rng.integers(0, 10 ** 8))
    return b"read%d strand=%s start=%d end=%d chr=%d" % (r, b"+-"[r & 1:(r & 1) + 1], start, start + 15000, 1 + r % 22)


def write_long(fastq_path, fasta_path, num_reads=20_000, length=15_000, seed=2):
    rng = np.random.default_rng(seed)
    step = 3000
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=num_reads * step + length)]
    quality = np.frombuffer(b"FFFF:,F#", dtype=np.uint8)[rng.integers(0, 8, size=length + 64)]
    rows = -(-length // 60)
    with open(fastq_path, "wb") as fq, open(fasta_path, "wb") as fa:
        for r in range(num_reads):
            title, seq = _title(r, rng), genome[r * step:r * step + length]
            fq.write(b"@" + title + b"\n" + seq.tobytes() + b"\n+\n" + quality[r % 64:r % 64 + length].tobytes() + b"\n")
            body = np.full(rows * 60, 10, dtype=np.uint8)
            body[:length] = seq
            wrapped = np.full((rows, 61), 10, dtype=np.uint8)
            wrapped[:, :60] = body.reshape(rows, 60)
            fa.write(b">" + title + b"\n" + wrapped.tobytes())
    return num_reads


def write_short(path, num_reads=500_000, seed=3):
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=1 << 20)].tobytes()
    length = rng.integers(60, 141, size=num_reads)
    at = rng.integers(0, (1 << 20) - 200, size=num_reads)
    with open(path, "wb") as f:
        for r in range(num_reads):
            f.write(b">" + _title(r, rng) + b"\n" + pool[at[r]:at[r] + length[r]] + b"\n")
    return num_reads


def write_gfa(path, num_reads):
    with open(path, "w") as f:
        f.writelines(f"S\tread{r}\t*\tLN:i:100\n" for r in range(num_reads))
        f.writelines(f"L\tread{r}\t+\tread{r + 1}\t+\t30M\n" for r in range(0, num_reads - 1, 7))


def timed(fn):
    out = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(round(time.perf_counter() - t0, 4))
    return out, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "reads_parse_time.txt"))
    ap.add_argument("--dir", default="/tmp/reads_parse_time")
    ap.add_argument("--files", default="fastq,fasta,short")
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dev = torch.device("cuda", 0)
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)

    emit(device=torch.cuda.get_device_name(0), runs=RUNS, note="seconds, wall, device drained before and after each run; host = the parent commit's code path")
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
    reads.read_reads_device(os.path.join(golden, "g14_single.fasta"), ["x"], device=dev, titles=True)   # load the library, warm the allocator
    paths = {k: os.path.join(args.dir, f"{k}.{'fastq' if k == 'fastq' else 'fasta'}") for k in ("fastq", "fasta", "short")}
    counts = {}
    wanted = args.files.split(",")
    if "fastq" in wanted or "fasta" in wanted:
        counts["fastq"] = counts["fasta"] = write_long(paths["fastq"], paths["fasta"])
    if "short" in wanted:
        counts["short"] = write_short(paths["short"])
    for name in wanted:
        path, R = paths[name], counts[name]
        gfa_path = os.path.join(args.dir, f"{name}.gfa")
        write_gfa(gfa_path, R)
        g = gfa.read_gfa(gfa_path, similarity=None)
        keep = np.random.default_rng(4).random(R) < 0.05
        for label, k in (("keep_none", None), ("keep_5_percent", keep)):
            res = {}
            for parser in ("host", "device"):
                secs, store = timed(lambda parser=parser, k=k: contigs.ReadStore.from_reads_file(path, g["node_to_read"], g["num_nodes"], keep=k,
                                                                                                 device=dev, parser=parser))
                res[parser] = (secs, store)
            same = torch.equal(res["host"][1].data, res["device"][1].data) and torch.equal(res["host"][1].off, res["device"][1].off)
            emit(file=name, bytes=os.path.getsize(path), reads=R, what=f"from_reads_file_{label}", host_s=res["host"][0], device_s=res["device"][0],
                 equal=bool(same))
            del res, store
        res = {}
        for rp in ("host", "device"):
            secs, out = timed(lambda rp=rp: gfa.read_gfa(gfa_path, similarity=None, training=True, reads_path=path, labels=False, reads_parser=rp))
            res[rp] = (secs, out)
        same = all(torch.equal(res["host"][1][k], res["device"][1][k]) for k in ("read_strand", "read_start", "read_end", "read_chr"))
        emit(file=name, bytes=os.path.getsize(path), reads=R, what="read_gfa_training_labels_false", host_s=res["host"][0], device_s=res["device"][0],
             equal=bool(same))
        # the share of the reads file in read_gfa(training=True): the same call without it
        secs, _ = timed(lambda: gfa.read_gfa(gfa_path, similarity=None))
        emit(file=name, what="read_gfa_without_training_host_parser", seconds=secs)


if __name__ == "__main__":
    main()
