"""From a GFA to contig walks on one MI355X - the sequence of inference.py:411-467 with every step on this package's side
of the boundary (GFA reader, feature preparation, the SymGatedGCN scorer, greedy decode), and assemble_to_fasta goes on to
inference.py:475-489 (walks -> contigs -> FASTA, gnnome_amd/contigs.py) with N50 / NG50.  The evaluation with minigraph /
paftools (evaluate.py:139-197) is not here.

    model = gnnome_amd.SymGatedGCNModel(2, 2, 64, 16, 8, 64, 'batch'); model.load_state_dict(torch.load('weights/weights.pt')); model.eval()
    walks, scores, g = assemble('asm.gfa', model, len_threshold=10, nb_paths=100)
    walks, contigs, stats = assemble_to_fasta('asm.gfa', model, '0_assembly.fasta', len_threshold=10, reads='reads.fastq.gz')
"""
import os

import torch

from . import contigs as contigs_mod
from . import analyze, decode, features, gfa, labels, metrics
from .graph import views_for


def score_graph(g, model, device=None):
    """inference.py:411-441: degree features (z-scored, :416-420), edge features (utils/data_utils.py:31-41), eval-mode model
    call -> logits[E] in edge-id order, on the device.  `g`: the dict read_gfa returns (overlap_similarity required - the
    shipped model was trained with it, hyperparameters.py:17)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    if g["overlap_similarity"] is None:
        raise ValueError("the graph carries no overlap similarities (see gnnome_amd.gfa: SI:f: tags, a similarity callable, or edlib)")
    views = views_for((g["src"], g["dst"], g["num_nodes"]), device)
    x = features.degree_features(views)
    e = features.edge_features(g["overlap_length"].to(device), g["overlap_similarity"].to(device))
    model = model.to(device).eval()
    with torch.no_grad():
        return model(views, x, e).squeeze(1)


def _read(path, similarity, parser, device, long_overlaps=False):
    """The graph dict of a GFA by `parser`: "host" = gfa.read_gfa; "device" = gfa.read_gfa_device, tensors and packed reads left on the
    device; "auto" = the device parser, and the host parser whenever that one reports anything.  long_overlaps goes to the reader's
    device similarity call (gfa.read_gfa)."""
    if parser not in ("host", "device", "auto"):
        raise ValueError(f"parser={parser!r}: expected 'host', 'device' or 'auto'")
    if parser == "device" or (parser == "auto" and not callable(similarity) and torch.cuda.is_available()):
        try:
            return gfa.read_gfa_device(path, similarity=similarity, device=device, long_overlaps=long_overlaps)
        except Exception:   # noqa: BLE001
            if parser == "device":
                raise
    return gfa.read_gfa(path, similarity=similarity, long_overlaps=long_overlaps)


def _simplified(g, simplify, device, renumber=True):
    """g through simplify.simplify_graph when `simplify` is True or a dict of its keywords; None leaves g alone.  renumber=False: the
    read sequences come from a source that knows the reads by their old numbers, so the reads keep them (compact=False; asking for
    compact=True there is refused)."""
    if simplify is None:
        return g
    if simplify is not True and not isinstance(simplify, dict):
        raise ValueError(f"simplify={simplify!r}: expected None, True or a dict of simplify_graph's keywords")
    from .simplify import simplify_graph
    kw = dict(simplify) if isinstance(simplify, dict) else {}
    if not renumber:
        if kw.get("compact"):
            raise ValueError("simplify: compact=True renumbers the reads, and the sequences of this call (the GFA file's S lines, or a "
                             "ReadStore) go by the old numbers; pass compact=False")
        kw["compact"] = False
    return simplify_graph(g, device=device, **kw)


def assemble(gfa_or_graph, model, len_threshold, nb_paths=100, similarity="auto", device=None, scores=None, sampler=None, parser="host",
             long_overlaps=False, early_stopping=False, p_threshold=0.06, random_walks=False, seed=None, simplify=None, isolated=False):
    """-> (walks, scores, graph dict).  `scores` overrides the model (inference.py:426-432: saved predictions / labels).
    parser: how a GFA path is read (gfa.read_gfa's parser=; with "device" the graph's tensors stay on the device).
    long_overlaps: gfa.read_gfa's keyword - True lets a GFA with overlaps beyond 65 536 bases (ultra-long ONT reads) through.
    early_stopping, p_threshold, random_walks, seed: decode.decode_contigs' keywords (the reference's decoder switches,
    inference.py:26-28); the ablation's constant scores are scores=decode.constant_scores(g).
    simplify: True or a dict of simplify.simplify_graph's keywords - the graph is simplified (transitive edges, tips, the reads left
    without an edge) before it is scored; the returned dict, and `scores` if given, are of the simplified graph.
    isolated: for a unitig graph - the decoder starts its walks from edges, so a segment that no walk reaches (one without edges above
    all) is never a contig; True appends a one-node walk for every even node of at least len_threshold bases that the walks leave
    untouched on both strands, in node order."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    g = gfa_or_graph if isinstance(gfa_or_graph, dict) else _read(gfa_or_graph, similarity, parser, device, long_overlaps)
    g = _simplified(g, simplify, device)
    if scores is None and isolated and int(torch.as_tensor(g["src"]).numel()) == 0:
        scores = torch.zeros(0)
    if scores is None:
        scores = score_graph(g, model, device)
    prefix = g["prefix_length"].masked_fill(g["prefix_length"] < 0, 0)      # inference.py:461
    dg = decode.DecodeGraph(g["src"], g["dst"], g["num_nodes"], prefix, g["read_length"], device=device).set_scores(scores)
    walks = decode.decode_contigs(dg, len_threshold, nb_paths=nb_paths, sampler=sampler, early_stopping=early_stopping,
                                  p_threshold=p_threshold, random_walks=random_walks, seed=seed)
    if isolated:
        free = torch.ones(int(g["num_nodes"]), dtype=torch.bool)
        free[torch.tensor([v ^ s for w in walks for v in w for s in (0, 1)], dtype=torch.long)] = False
        long_enough = torch.as_tensor(g["read_length"]).reshape(-1).cpu() >= len_threshold
        walks = walks + [[v] for v in torch.nonzero(free & long_enough).squeeze(1).tolist() if v % 2 == 0]
    return walks, scores, g


def assemble_to_fasta(gfa_or_graph, model, out_path, len_threshold, reads=None, nb_paths=100, similarity="auto", device=None, scores=None,
                      sampler=None, line_width=contigs_mod.FASTA_WRAP, ref_length=None, parser="host", reads_parser="host",
                      long_overlaps=False, early_stopping=False, p_threshold=0.06, random_walks=False, seed=None, simplify=None,
                      isolated=False):
    """GFA -> scores -> greedy walks -> contigs spelled on the device -> FASTA at out_path (inference.py:411-489).
    -> (walks, contigs, stats); stats = quick_evaluation's figures as a dict (ref_length from the caller: NG50 and the
    reconstructed fraction are -1 without it).  Sequences: the GFA's S lines if it carries them, else `reads` (a FASTA / FASTQ
    path, plain or .gz, or a ReadStore); with neither this raises before any scoring.  Only the reads the walks touch are
    uploaded.  The prefixes are masked as pipeline.assemble masks them (inference.py:461).  parser="device" / "auto": the GFA is read
    once, by gfa.read_gfa_device, and its sequences are the packed reads that parse left on the device, restricted to the touched ones.
    reads_parser: how a `reads` file is read (ReadStore.from_reads_file's parser=).  long_overlaps, early_stopping, p_threshold,
    random_walks, seed, simplify, isolated: as in assemble; where the sequences come from the GFA file's S lines (parser="host") or from a
    ReadStore the reads keep their numbers (compact=False)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    gfa_path = None if isinstance(gfa_or_graph, dict) else gfa_or_graph
    if gfa_path is not None and parser != "host":
        gfa_or_graph = _read(gfa_path, similarity, parser, device, long_overlaps)
        if "reads" in gfa_or_graph:     # device-parsed: nothing below opens the GFA again
            gfa_path = None
    elif parser not in ("host", "device", "auto"):
        raise ValueError(f"parser={parser!r}: expected 'host', 'device' or 'auto'")
    if isinstance(reads, contigs_mod.ReadStore):
        source = "store"
    elif isinstance(gfa_or_graph, dict) and gfa_or_graph.get("reads") is not None:
        source = "packed"
    elif gfa_path is not None and contigs_mod.gfa_sequences(gfa_path) is not None:
        source = "gfa"
    elif reads is not None:
        if not os.path.isfile(reads):
            raise FileNotFoundError(f"reads file {reads} not found")
        contigs_mod.reads_file_type(reads)
        source = "file"
    elif isinstance(gfa_or_graph, dict) and gfa_or_graph.get("read_seqs"):
        source = "dict"
    else:
        raise ValueError("no read sequences: the GFA's S lines say '*' (or a graph dict was passed) and no `reads` was given")
    g = gfa_or_graph if isinstance(gfa_or_graph, dict) else gfa.read_gfa(gfa_or_graph, similarity=similarity, long_overlaps=long_overlaps)
    g = _simplified(g, simplify, device, renumber=source not in ("store", "gfa"))
    walks, scores, g = assemble(g, model, len_threshold, nb_paths=nb_paths, similarity=similarity, device=device, scores=scores,
                                sampler=sampler, early_stopping=early_stopping, p_threshold=p_threshold, random_walks=random_walks, seed=seed,
                                isolated=isolated)
    touched = sorted({v >> 1 for w in walks for v in w})
    if source == "store":
        store = reads
    elif source == "packed":
        store = contigs_mod.ReadStore.from_packed(*g["reads"], keep=touched)
    elif source == "gfa":
        store = contigs_mod.ReadStore.from_gfa(gfa_path, keep=touched, device=device)
    elif source == "file":
        store = contigs_mod.ReadStore.from_reads_file(reads, g["node_to_read"], g["num_nodes"], keep=touched, device=device,
                                                      parser=reads_parser)
    else:
        store = contigs_mod.ReadStore.from_sequences([g["read_seqs"][2 * r] for r in range(g["num_nodes"] // 2)], keep=touched, device=device)
    prefix = g["prefix_length"].masked_fill(g["prefix_length"] < 0, 0)
    dg = decode.DecodeGraph(g["src"], g["dst"], g["num_nodes"], prefix, g["read_length"], device=device)
    contigs = contigs_mod.spell_contigs(dg, walks, store, line_width=line_width)
    contigs_mod.write_fasta(contigs, out_path, line_width=line_width)
    stats = {"num_contigs": len(contigs), "total_length": int(sum(contigs.lengths_host())) if len(contigs) else 0}
    if len(contigs):
        n, longest, rec, n50, ng50 = contigs_mod.quick_evaluation(contigs, ref_length)
        stats.update(longest_contig=longest, reconstructed=rec, n50=n50, ng50=ng50)
    else:
        stats.update(longest_contig=0, reconstructed=-1, n50=-1, ng50=-1)
    return walks, contigs, stats


def assemble_reads_to_fasta(reads_path, model, out_path, len_threshold, nb_paths=100, device=None, scores=None, use_labels=False,
                            sampler=None, line_width=contigs_mod.FASTA_WRAP, ref_length=None, long_overlaps=False, unitigs=False, **overlap_kw):
    """Reads -> overlap graph -> scores -> greedy walks -> contigs -> FASTA at out_path, with no assembler's GFA in between:
    reads.read_reads_device (every record of the FASTA / FASTQ file, in file order; a repeated id keeps its last record) ->
    overlapper.overlap_graph (overlap_kw: its k, w, max_occ, band, min_seeds, min_overlap, max_hang, max_pairs, drop_contained, simplify;
    with simplify's compact the names follow the dict's kept_reads) ->
    assemble_to_fasta on that dict.  -> (walks, contigs, stats, graph dict).  scores: one logit per edge instead of the model.
    use_labels: the titles carry strand=, start=, end= and chr= (the simulator's), the dict gets the four read_* columns and y, and the
    labels are the scores (+20 / -20 as logits: the reference's use_labels, whose floor is 1e-9).
    unitigs: True, or a dict of unitigs.compact_unitigs' keywords - the graph (named and, with use_labels, labelled as a read graph
    first) is compacted, and the decoder walks the unitig graph with the unitig sequences as the read store; `scores`, if given, are per
    edge of the unitig graph; unitigs that no walk reaches become contigs of their own (assemble's isolated=True).  The returned dict is
    the unitig graph."""
    if unitigs is not False and unitigs is not True and not isinstance(unitigs, dict):
        raise ValueError(f"unitigs={unitigs!r}: expected False, True or a dict of compact_unitigs' keywords")
    from . import overlapper
    from .reads import read_reads_device
    device = device or torch.device("cuda", torch.cuda.current_device())
    names = list(dict.fromkeys(contigs_mod.read_titles(reads_path)))
    res = read_reads_device(reads_path, names, device=device, sequences=True, titles=use_labels)
    annotations = None
    if use_labels:
        if bool((res.missing != 0).any()):
            raise ValueError(f"{reads_path}: use_labels needs strand=, start=, end= and chr= in every title")
        cols = torch.repeat_interleave(res.ann, 2, dim=0)
        cols[1::2, 0] = -cols[1::2, 0]
        annotations = [cols[:, j].contiguous() for j in range(4)]
    g = overlapper.overlap_graph((res.data, res.off), annotations=annotations, device=device, long_overlaps=long_overlaps, **overlap_kw)
    kept = g["kept_reads"].tolist() if "kept_reads" in g else range(len(names))
    g["node_to_read"] = {2 * i + s: names[r] for i, r in enumerate(kept) for s in (0, 1)}
    if use_labels:
        g["y"] = labels.process_graph(g, device=device)[1]
    if unitigs is not False:
        from .unitigs import compact_unitigs
        g = compact_unitigs(g, device=device, **(unitigs if isinstance(unitigs, dict) else {}))
    if use_labels:
        scores = (g["y"] * 2 - 1) * 20
    walks, contigs, stats = assemble_to_fasta(g, model, out_path, len_threshold, nb_paths=nb_paths, device=device, scores=scores,
                                              sampler=sampler, line_width=line_width, ref_length=ref_length, isolated=unitigs is not False)
    return walks, contigs, stats, g


def edge_report(g, model=None, scores=None, device=None):
    """The quality figures of a scorer on a labelled graph (a dict with `y`, e.g. read_gfa(training=True)): the confusion counts at
    0.5, the eight figures utils/metrics.py:15-46 derives from them and the two average precisions (:67-80).  `scores` (logits, one
    per edge) overrides the model, as in assemble."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    if g.get("y") is None:
        raise ValueError("edge_report: the graph carries no labels y (read_gfa(training=True), or labels.process_graph)")
    if scores is None:
        if model is None:
            raise ValueError("edge_report: neither a model nor scores")
        scores = score_graph(g, model, device)
    scores = torch.as_tensor(scores).detach().reshape(-1).float().to(device)
    y = torch.as_tensor(g["y"]).reshape(-1).float().to(device)
    TP, TN, FP, FN = metrics.calculate_tfpn(scores, y)
    acc, precision, recall, f1 = metrics.calculate_metrics(TP, TN, FP, FN)
    acc_inv, precision_inv, recall_inv, f1_inv = metrics.calculate_metrics_inverse(TP, TN, FP, FN)
    return {"TP": TP, "TN": TN, "FP": FP, "FN": FN, "acc": acc, "precision": precision, "recall": recall, "f1": f1,
            "acc_inv": acc_inv, "precision_inv": precision_inv, "recall_inv": recall_inv, "f1_inv": f1_inv,
            "aps": metrics.get_aps(scores, y, device=device), "aps_inverse": metrics.get_aps_inverse(scores, y, device=device)}


def walk_report(g, walks, device=None):
    """The walk checks of utils/analyze.py:1-38 summed over `walks` on a graph with read positions (read_gfa(training=True)): per kind -
    strand, chromosome, overlap - the number of findings and the number of walks with at least one, copied to the host once.
    analyze.audit_walks has the findings themselves."""
    audit = analyze.audit_walks(g, walks, device=device)
    counts = audit.counts.long()
    totals = torch.cat([counts.sum(0), (counts > 0).sum(0)]).tolist()
    kinds = ("strand", "chromosome", "overlap")
    report = {"walks": len(audit)}
    report.update({k: totals[i] for i, k in enumerate(kinds)})
    report.update({"walks_with_" + k: totals[3 + i] for i, k in enumerate(kinds)})
    return report


def coverage_report(g, ref_length=None, device=None):
    """How much of the reference the simulated reads of a graph with read positions (read_gfa(training=True)) can reconstruct at all:
    labels.reference_coverage - per chromosome and in total the covered bases, the number of islands and the longest island, and the
    covered fraction when ref_length (an int, or a dict by chromosome code) is given.  The covered total is the honest ref_length for
    contigs.calculate_NG50 / quick_evaluation; the island count is a lower bound on the contigs of a perfect assembly."""
    return labels.reference_coverage(g, ref_length=ref_length, device=device)
