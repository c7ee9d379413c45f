"""GFA ingestion: the host parser (gfa.read_gfa's Python loop, the code path every earlier commit has) against the device parser
(gfa.read_gfa_device, csrc/gfa_parse.hip) on the same box, three runs each, wall time with the device drained.

    python tools/gfa_parse_time.py [--out profiles/gfa_parse_time.txt] [--dir /tmp/gfa_parse_time]

Two synthetic files with a fixed seed:
  noseq   50 000 S lines ('*'), 500 000 eight-field L lines (hifiasm 'noseq' style), ~26 MB
  seqs    20 000 reads x 15 kb WITH sequences, layout links with SI:f: tags, ~300 MB
Timed: read_gfa(parser="host", similarity=None) against read_gfa_device(similarity=None) on both files, then
pipeline.assemble_to_fasta with fixed scores= for both parsers on the second.  parser="host" runs exactly the code the parent
commit runs (the function's body is untouched), so its rows are the baseline; the device rows are never compared to themselves."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnome_amd import decode, gfa, pipeline  # noqa: E402

RUNS = 3


def write_noseq(path, segments=50_000, links=500_000, seed=1):
    rng = np.random.default_rng(seed)
    length = rng.integers(9000, 25000, size=segments)
    a = rng.integers(0, segments, size=links)
    b = (a + rng.integers(1, 40, size=links)) % segments
    o = rng.integers(0, 2, size=(links, 2))
    ol = rng.integers(500, 9000, size=links)
    with open(path, "w") as f:
        f.writelines(f"S\tutg{k:06d}l\t*\tLN:i:{length[k]}\trd:i:12\n" for k in range(segments))
        f.writelines(f"L\tutg{a[k]:06d}l\t{'+-'[o[k, 0]]}\tutg{b[k]:06d}l\t{'+-'[o[k, 1]]}\t{ol[k]}M\tL1:i:{length[a[k]] - ol[k]}\tL2:i:{length[b[k]] - ol[k]}\n"
                     for k in range(links))


def write_seqs(path, reads=20_000, length=15_000, seed=2):
    rng = np.random.default_rng(seed)
    step = 3000
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=reads * step + length)]
    with open(path, "wb") as f:
        for r in range(reads):
            f.write(b"S\tread%d\t" % r)
            f.write(genome[r * step:r * step + length].tobytes())
            f.write(b"\tLN:i:%d\n" % length)
        for r in range(reads):
            for t in range(r + 1, min(r + 5, reads)):
                f.write(b"L\tread%d\t+\tread%d\t+\t%dM\tSI:f:%.6f\n" % (r, t, length - (t - r) * step, 1.0 - 0.002 * rng.random()))


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
    ap.add_argument("--out", default=os.path.join("profiles", "gfa_parse_time.txt"))
    ap.add_argument("--dir", default="/tmp/gfa_parse_time")
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dev = torch.device("cuda", 0)
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    emit(device=torch.cuda.get_device_name(0), runs=RUNS, note="seconds, wall, device drained before and after each run")
    gfa.read_gfa_device(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "g10_raven6.gfa"), similarity=None)   # load
    files = {"noseq": write_noseq, "seqs": write_seqs}
    for name, make in files.items():
        path = os.path.join(args.dir, f"{name}.gfa")
        make(path)
        host_s, h = timed(lambda: gfa.read_gfa(path, similarity=None, parser="host"))
        dev_s, d = timed(lambda: gfa.read_gfa_device(path, similarity=None, device=dev))
        nonames_s, _ = timed(lambda: gfa.read_gfa_device(path, similarity=None, device=dev, keep_names=False))
        same = all(torch.equal(d[k].cpu(), h[k]) for k in ("src", "dst", "overlap_length", "prefix_length", "read_length"))
        emit(file=name, bytes=os.path.getsize(path), nodes=h["num_nodes"], edges=int(h["src"].numel()), read_gfa_host_s=host_s,
             read_gfa_device_s=dev_s, read_gfa_device_keep_names_false_s=nonames_s, equal=bool(same and d["read_to_node"] == h["read_to_node"]))
        if name == "seqs":
            src, dst = h["src"], h["dst"]
            hop = torch.where(src % 2 == 0, (dst - src) // 2, (src - dst) // 2).float()
            scores = (10.0 - 2.0 * hop).to(dev)
            res = {}
            for parser in ("host", "device"):
                fasta = os.path.join(args.dir, f"{parser}.fasta")

                def run(parser=parser, fasta=fasta):
                    torch.manual_seed(1)
                    return pipeline.assemble_to_fasta(path, None, fasta, 10, scores=scores, sampler=decode.sample_edges_device, nb_paths=20,
                                                      device=dev, parser=parser)
                secs, (walks, _, stats) = timed(run)
                res[parser] = (walks, open(fasta, "rb").read(), stats)
                emit(file=name, assemble_to_fasta_parser=parser, seconds=secs, contigs=stats["num_contigs"], total_length=stats["total_length"])
            emit(file=name, assemble_to_fasta_equal=bool(res["host"] == res["device"]))
    with open(args.out, "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
