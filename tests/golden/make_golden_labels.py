"""Generate tests/golden/g14_labels.pt (+ g14_*.gfa and g14_*.fasta / .fastq.gz inputs) from the REFERENCE's own training-mode parser
and labelling.  Build container only:

    python tests/golden/make_golden_labels.py        # needs the reference checkout at REF (make_golden_gfa.py)

graph_parser.only_from_gfa (:120-581) and every function of utils/labels.py are compiled from their files' syntax trees (as in
make_golden_gfa.py) and run with the real networkx, the Seq / edlib / dgl.from_networkx stand-ins of make_golden_gfa.py, and
  * `SeqIO.parse(handle_or_path, "fasta" | "fastq")`: records with .id (the title's first token), .description (the whole title)
    and .seq - what Biopython's FASTA and FASTQ iterators give;
  * `utils.labels`: the compiled reference module.  With several chromosomes only_from_gfa calls process_graph_combo, which calls
    .item() on the chromosome codes that only_from_gfa itself stored as Python ints and so raises AttributeError; for that case the
    codes are turned into numpy integers on the networkx graph first, and then the reference's process_graph_combo runs unchanged;
  * `dgl.load_graphs` for interval_union: the graph only_from_gfa just returned.
The reference's text runs; none of it is stored.  Starts and ends never tie within one (chromosome, strand), so every argmin / argmax
is decided by its key and the labels do not depend on the reference's set iteration order."""
import gzip
import os
import re
import sys
import types
from collections import Counter, namedtuple
from datetime import datetime

import networkx as nx
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_gfa import REF, Seq, _Dgl, _Edlib, reference_functions  # noqa: E402


class _Record:
    def __init__(self, title, seq):
        self.description = title
        self.id = title.split(None, 1)[0] if title.strip() else ""
        self.seq = Seq(seq)


class _SeqIO:
    @staticmethod
    def parse(handle, kind):
        f = open(handle) if isinstance(handle, str) else handle
        lines = [ln.rstrip("\n") for ln in f]
        recs, i = [], 0
        if kind == "fasta":
            while i < len(lines):
                if lines[i].startswith(">"):
                    title, seq, i = lines[i][1:].rstrip(), [], i + 1
                    while i < len(lines) and not lines[i].startswith(">"):
                        seq.append(lines[i].strip())
                        i += 1
                    recs.append(_Record(title, "".join(seq)))
                else:
                    i += 1
        else:
            while i < len(lines):
                if not lines[i].strip():
                    i += 1
                    continue
                recs.append(_Record(lines[i][1:].rstrip(), lines[i + 1].strip()))
                i += 4
        return iter(recs)


def write_reads(path, reads, fastq=False):
    """reads: (id, title fields, sequence)."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "wt") as f:
        for rid, fields, seq in reads:
            if fastq:
                f.write(f"@{rid} {fields}\n{seq}\n+\n{'I' * len(seq)}\n")
            else:
                f.write(f">{rid} {fields}\n{seq[:len(seq) // 2]}\n{seq[len(seq) // 2:]}\n")


def layout(rng, chroms, reads_per_chr, gaps):
    """Reads at distinct positions per chromosome: (chr code, start, end, strand), genome-sorted per chromosome."""
    out = []
    for c in chroms:
        starts = np.sort(rng.choice(np.arange(0, 60 * reads_per_chr, 3), size=reads_per_chr, replace=False)) * 14   # even
        ends = starts + rng.choice(np.arange(900, 2000), size=reads_per_chr, replace=False) * 2 + 1                  # odd
        for g in gaps:   # a coverage gap: reads after it start beyond every end before it
            shift = int(ends[:g].max()) - int(starts[g]) + 1001 if g < reads_per_chr else 0
            starts[g:] += shift + (shift & 1)
            ends[g:] += shift + (shift & 1)
        assert len(set(ends.tolist())) == reads_per_chr, "tied ends: choose another seed"
        for s, e in zip(starts.tolist(), ends.tolist()):
            out.append((c, s, e, "+" if rng.random() < 0.5 else "-"))
    return out


def case_files(name, rng, reads, extra_links=(), utg=None, fastq=False, chr_field=None, isolated=()):
    """Write the GFA (6-field L lines) and the reads file; a link joins each read to its next 1-3 genome successors that it
    overlaps, in the orientation the reads have on the genome's + strand; extra_links: (a, b, same_orientation) links outside that
    rule (false ones, or the only links of the `isolated` reads)."""
    ids = [f"read{k}" for k in range(len(reads))]
    seqs = ["".join(rng.choice(list("ACGT"), size=16)) for _ in reads]
    code = chr_field or (lambda c: {-1: "X", -2: "Y", -3: "M"}.get(c, str(c)))
    records = []
    for k, (c, s, e, st) in enumerate(reads):
        fields = [f"strand={st}", f"start={s}", f"end={e}", f"chr={code(c)}"]
        rng.shuffle(fields)
        records.append((ids[k], " ".join(fields) + " depth=1", seqs[k]))
    records.insert(1, (ids[1], "strand=+ start=1 end=2 chr=1", seqs[1]))   # a repeated id: the last record wins
    gfa_lines, done = [], set()
    if utg is not None:   # unitig utg000001l stands for the reads in `utg`: (read index, A-line orientation)
        members = {k for k, _ in utg}
    else:
        members = set()
    seg = {}
    for k in range(len(reads)):
        if k in members:
            continue
        seg[k] = ids[k]
        gfa_lines.append(f"S\t{ids[k]}\t{seqs[k]}\tLN:i:{reads[k][2] - reads[k][1]}")
    if utg is not None:
        head = min(k for k, _ in utg)
        gfa_lines.append(f"S\tutg000001l\t{seqs[head]}\tLN:i:5000")
        for k, o in utg:
            gfa_lines.append(f"A\tutg000001l\t0\t{o}\t{ids[k]}\t0\t{reads[k][2] - reads[k][1]}\tid:i:{k}")
            seg[k] = "utg000001l"
    utg_strand = 1
    if utg is not None:
        utg_strand = 1 if sum((1 if reads[k][3] == "+" else -1) * (1 if o == "+" else -1) for k, o in utg) >= 0 else -1
    orient = lambda k: ("+" if utg_strand > 0 else "-") if k in members else ("+" if reads[k][3] == "+" else "-")   # noqa: E731
    for a in range(len(reads)):
        for b in range(a + 1, min(a + 4, len(reads))):
            if a in isolated or b in isolated or reads[b][0] != reads[a][0] or reads[b][1] >= reads[a][2] or seg[a] == seg[b] or (seg[a], seg[b]) in done:
                continue
            done.add((seg[a], seg[b]))
            gfa_lines.append(f"L\t{seg[a]}\t{orient(a)}\t{seg[b]}\t{orient(b)}\t{int(rng.integers(100, 500))}M")
    for a, b, same in extra_links:
        gfa_lines.append(f"L\t{seg[a]}\t{orient(a)}\t{seg[b]}\t{orient(b) if same else '+-'[orient(b) == '+']}\t77M")
    gfa = os.path.join(HERE, f"g14_{name}.gfa")
    with open(gfa, "w") as f:
        f.write("\n".join(gfa_lines) + "\n")
    rpath = os.path.join(HERE, f"g14_{name}.fastq.gz" if fastq else f"g14_{name}.fasta")
    write_reads(rpath, records, fastq)
    return gfa, rpath


def main():
    scope = {"nx": nx, "Seq": Seq, "dgl": _Dgl, "edlib": _Edlib, "tqdm": lambda x, **k: x, "datetime": datetime, "re": re, "gzip": gzip,
             "Counter": Counter, "namedtuple": namedtuple, "SeqIO": _SeqIO, "print": lambda *a, **k: None}
    lab_scope = {"nx": nx, "print": lambda *a, **k: None}
    names = ["interval_union", "get_gt_for_single_strand", "create_correct_graphs", "create_correct_graphs_combo", "process_graph",
             "process_graph_combo"]
    interval_union, _, _, _, process_graph, process_graph_combo = reference_functions(os.path.join(REF, "utils", "labels.py"), names, lab_scope)
    calls = []

    def combo_numpy_chr(graph):   # see the module docstring: the codes as numpy integers, then the reference's own function
        calls.append("combo")
        nx.set_node_attributes(graph, {u: np.int64(c) for u, c in nx.get_node_attributes(graph, "read_chr").items()}, "read_chr")
        return process_graph_combo(graph)

    def single(graph):
        calls.append("single")
        return process_graph(graph)

    scope["utils"] = types.SimpleNamespace(labels=types.SimpleNamespace(process_graph=single, process_graph_combo=combo_numpy_chr))
    (only_from_gfa,) = reference_functions(os.path.join(REF, "graph_parser.py"),
                                           ["get_neighbors", "get_predecessors", "get_edges", "calculate_similarities", "only_from_gfa"], scope)[-1:]
    rng = np.random.default_rng(14)
    specs = []
    # one chromosome, both genome strands, three gaps (several components), a rejected component (a short pair inside the first
    # component's span that is linked only to itself) and false links across strands
    r = layout(rng, [1], 40, gaps=[12, 25, 33])
    r.append((1, r[2][1] + 10, r[2][1] + 400, "+"))
    r.append((1, r[2][1] + 200, r[2][1] + 700, "-"))
    r.sort(key=lambda t: t[1])
    iso = [k for k, t in enumerate(r) if t[1] in (r[2][1] + 10, r[2][1] + 200) and (t[2] - t[1]) in (390, 500)]
    specs.append(("single", r, [(5, 30, True), (7, 8, False), (iso[0], iso[1], True)], None, False, set(iso)))
    # a unitig whose reads disagree on strand, one chromosome (X), the reads as gzipped FASTQ
    r = layout(rng, [-1], 30, gaps=[17])
    specs.append(("utg_x", r, [], [(3, "+"), (4, "-"), (5, "+")], True, set()))
    # several chromosomes, X / Y / M among them: the process_graph_combo path
    r = layout(rng, [1, 2, -1, -2, -3], 14, gaps=[8])
    specs.append(("multi", r, [(1, 20, True), (30, 31, False)], None, False, set()))
    cases = []
    for name, reads, extra, utg, fastq, iso in specs:
        for c in {t[0] for t in reads}:
            ss, ee = [t[1] for t in reads if t[0] == c], [t[2] for t in reads if t[0] == c]
            assert len(set(ss)) == len(ss) and len(set(ee)) == len(ee), f"{name}: tied positions"
        gfa, rpath = case_files(name, rng, reads, extra, utg, fastq, isolated=iso)
        calls.clear()
        g, aux = only_from_gfa(gfa, training=True, reads_path=rpath, get_similarities=False)
        src, dst = g.edges()
        scope_dgl = types.SimpleNamespace(load_graphs=lambda path: ([g], None))
        lab_scope["dgl"] = scope_dgl
        union = interval_union(name, HERE)
        nd = g.ndata
        cases.append({"name": name, "gfa": os.path.basename(gfa), "reads": os.path.basename(rpath), "path": calls[0],
                      "src": src, "dst": dst, "num_nodes": g.num_nodes(), "read_strand": nd["read_strand"], "read_start": nd["read_start"],
                      "read_end": nd["read_end"], "read_chr": nd["read_chr"], "y": g.edata["y"].to(torch.float32),
                      "interval_union": union})
        print(name, calls[0], "N =", g.num_nodes(), "E =", src.numel(), "labelled =", int(g.edata["y"].sum()))
    torch.save({"cases": cases, "made_with": "tests/golden/make_golden_labels.py (graph_parser.only_from_gfa(training=True) and "
                "utils/labels.py via ast, networkx " + nx.__version__ + ")"}, os.path.join(HERE, "g14_labels.pt"))


if __name__ == "__main__":
    main()
