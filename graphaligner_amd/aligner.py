"""Host-side mirror of the reference's driver around the hot path:
`alignReads` / `runComponentMappings` (Aligner.cpp:107-205, 230-322) and the flags of AlignerMain.cpp.

What is kept: read loading by file extension (fastqloader.cpp), seeds grouped by read name in file
order (Aligner.cpp:246-271), graph loading by extension (Aligner.cpp:207-228), the per-read messages,
failed / poor-score handling (Aligner.cpp:153-171), the digraph-id -> original-id rewrite (:83-91), the
combined GAM (:301-314) and the per-read `alignment_<t>_<name>.gam` / `trace_<t>_<name>.trace`
files (:177-201).  What differs: the reference's `-t N` threads each pop one read at a time and call
AlignOneWay; here the whole read set is one batch on the GPU (`-t` is accepted and only names the
"thread" in messages and file names: everything is thread 0).  Reads are popped from the BACK of the
list by the reference (:113-117), so with `-t 1` its output order is the reverse of the input order;
that order is kept.  `-i` (no seeds) and `-A` (augmented graph) are not part of the hot path and
are refused.  An addition of this project: `--find-seeds` (with `--seed-k K`, `--seed-max N`) stands in
for `-s`: the seeds come from the library's k-mer index of the graph (binding.Graph.find_seeds).  `--seed-walks N`
(1..256; 0, the default: k-mers inside nodes only) builds the walk index, which a graph of nodes shorter than k needs.  `--seed-loci`
groups a read's hits into loci first and gives one seed per locus (binding.Graph.find_seeds(loci=True)), so that a long read is not
extended twice from the same place.  `--seed-coord file|topology` chooses the linear coordinate the hits are ranked and grouped by: the
order of the graph file (the default) or the coordinate built from the edges (binding.Graph.set_seed_coordinate), which a graph
file that is not in path order needs.

    python -m graphaligner_amd.aligner -g graph.gfa -f reads.fastq -s seeds.gam -a out.gam -t 1 -b 35
    python -m graphaligner_amd.aligner -g graph.gfa -f reads.fastq --find-seeds -a out.gam -t 1 -b 35
"""
import getopt
import gzip
import os
import sys

import numpy as np

from . import binding


class Read:
    def __init__(self, seq_id, sequence):
        self.seq_id = seq_id
        self.sequence = sequence


def load_reads(path):
    """fastqloader.cpp:6-76: format by extension; fastq = 4-line records starting with '@'"""
    def lines():
        with open(path, "r") as f:
            for line in f:
                line = line.rstrip("\n")
                yield line[:-1] if line.endswith("\r") else line
    reads = []
    if path.endswith(".fastq") or path.endswith(".fq"):
        it = lines()
        for line in it:
            if not line.startswith("@"):
                continue
            seq = next(it, "")
            next(it, "")
            next(it, "")
            reads.append(Read(line[1:], seq))
    elif path.endswith(".fasta") or path.endswith(".fa"):
        cur = None
        for line in lines():
            if line.startswith(">"):
                cur = Read(line[1:], "")
                reads.append(cur)
            elif cur is not None:
                cur.sequence += line
    return reads


def load_graph(path, device=0, lib_path=None):
    """Aligner.cpp:207-228"""
    if not os.path.exists(path):
        sys.stderr.write("No graph file exists\n")
        raise SystemExit(0)
    sys.stdout.write("load graph from %s\n" % path)
    if path.endswith(".vg"):
        return binding.Graph(vg=open(path, "rb").read(), device=device, lib_path=lib_path)
    if path.endswith(".gfa"):
        return binding.Graph(gfa=open(path, "rb").read(), device=device, lib_path=lib_path)
    sys.stderr.write("Unknown graph type (%s)\n" % path)
    raise SystemExit(0)


# ---- a second, independent GAM writer (the C one is ga_results_encode_gam) for the per-read files ----
def _varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _int_field(f, v):
    return b"" if v == 0 else _varint(f << 3) + _varint(v)          # proto3: zero is not written


def _bytes_field(f, b):
    return b"" if len(b) == 0 else _varint((f << 3) | 2) + _varint(len(b)) + b


def _message(f, b):
    return _varint((f << 3) | 2) + _varint(len(b)) + b


def encode_alignment(name, sequence, result, halve_node_ids=True):
    """vg.Alignment{1:sequence, 2:Path{2:Mapping{1:Position{1:node_id,2:offset,4:is_reverse}, 2:Edit{1:from_length,2:to_length,3:sequence}, 5:rank}},
    3:name, 6:score, 7:query_position} (vg.pb.h field numbers)"""
    path = b""
    for node_id, is_reverse, offset, rank, from_length, to_length, seq in result["mappings"]:
        pos = _int_field(1, node_id // 2 if halve_node_ids else node_id) + _int_field(2, offset) + _int_field(4, int(is_reverse))
        edit = _int_field(1, from_length) + _int_field(2, to_length) + _bytes_field(3, seq.encode())
        path += _message(2, _message(1, pos) + _message(2, edit) + _int_field(5, rank))
    return (_bytes_field(1, sequence.encode()) + _message(2, path) + _bytes_field(3, name.encode())
            + _int_field(6, result["score"]) + _int_field(7, result["query_position"]))


def gam_group(messages):
    """stream.hpp:24-118: one gzip member holding varint count, then varint length + message"""
    body = _varint(len(messages)) + b"".join(_varint(len(m)) + m for m in messages)
    return gzip.compress(body)


def _safe(name):
    return name.replace("/", "_").replace(":", "_")


class AlignerParams:
    def __init__(self):
        self.graphFile = ""
        self.fastqFile = ""
        self.alignmentFile = ""
        self.auggraphFile = ""
        self.seedFile = ""
        self.numThreads = 0
        self.initialBandwidth = 0
        self.rampBandwidth = 0
        self.dynamicRowStart = 64
        self.perReadFiles = True
        self.outputDir = "."
        # --find-seeds: no seed file; the seeds come from the library's k-mer index of the graph (Graph.find_seeds)
        self.findSeeds = False
        self.seedK = 15
        self.seedMax = 2
        self.seedWalks = 0          # --seed-walks: 0 = the in-node index, 1..256 = the walk index with that max_walks
        self.seedLoci = False       # --seed-loci: one seed per locus
        self.seedCoord = "file"     # --seed-coord: "file" or "topology"
        self.opsFile = ""           # --ops-out: per aligned read its operations (GA_F_OPS): counts, identity and the run string
        self.correctedFile = ""     # --corrected-out: per aligned read the graph's bases along its alignment (GA_F_PATHSEQ), as FASTA
        self.pileupFile = ""        # --pileup-out: per graph base that any aligned read touches, the eight counts of a pileup (GA_F_PILEUP)
        self.edgeSupportFile = ""   # --edge-support-out: per edge of the bigraph that any aligned read crosses, its count (a pileup of kind "edges")
        # --sites-out: the columns of a BASES pileup that pass the thresholds, selected on the device (Pileup.sites): --sites-min-depth,
        # --sites-min-alt, --sites-frac NUM/DEN; --sites-fold folds the two strands onto the forward copies
        self.sitesFile = ""
        self.sitesMinDepth = 1
        self.sitesMinAlt = 0
        self.sitesFrac = (0, 1)
        self.sitesFold = False
        # --supported-edges-out: the edges of the bigraph whose folded count is >= --min-edge-support, from one fold query on the device
        self.supportedEdgesFile = ""
        self.minEdgeSupport = 1


def align_reads(params, device=0, lib_path=None, out=sys.stdout, err=sys.stderr):
    """Aligner.cpp:230-322 with the per-read loop of :107-205.  Returns the list of (read name, result dict) written."""
    if not os.path.exists(params.fastqFile):
        err.write("No fastq file exists\n")
        raise SystemExit(0)
    reads = load_reads(params.fastqFile)
    out.write("%d reads\n" % len(reads))
    # (GA_F_OPS only when its file is asked for: the other output is the same with and without it)
    flags = binding.GA_F_TRACE | (binding.GA_F_OPS if getattr(params, "opsFile", "") else 0)
    # (nor GA_F_PATHSEQ)
    if getattr(params, "correctedFile", ""):
        flags |= binding.GA_F_PATHSEQ
    want_pileup = bool(getattr(params, "pileupFile", ""))
    want_edges = bool(getattr(params, "edgeSupportFile", ""))
    want_sites = bool(getattr(params, "sitesFile", ""))
    want_supported = bool(getattr(params, "supportedEdgesFile", ""))
    if want_pileup or want_edges or want_sites or want_supported:
        flags |= binding.GA_F_PILEUP
    find_seeds = getattr(params, "findSeeds", False)
    if params.seedFile == "" and not find_seeds:
        err.write("either initial full band or seed file must be set\n")
        raise SystemExit(0)
    seeds_of = {}                    # read number -> its seeds
    if not find_seeds:
        if not os.path.exists(params.seedFile):
            err.write("No seeds file exists\n")
            raise SystemExit(0)
        seeds_by_name = {}
        for name, seed in binding.decode_seed_gam(open(params.seedFile, "rb").read(), lib_path=lib_path):
            seeds_by_name.setdefault(name, []).append(seed)
        seeds_of = {i: seeds_by_name[r.seq_id] for i, r in enumerate(reads) if r.seq_id in seeds_by_name}
    graph = load_graph(params.graphFile, device=device, lib_path=lib_path)
    if find_seeds:
        walks = getattr(params, "seedWalks", 0)
        coord = getattr(params, "seedCoord", "file")
        st = graph.build_seed_index(k=params.seedK, max_walks=walks, coordinate=coord)
        line = "seed index: %d entries of %d k-mers (k %d), %.1f MB" % (st["entries"], st["kmers_seen"], st["k"], st["bytes"] / 1e6)
        if walks:
            ws = graph.seed_index_walk_stats()
            line += ", walks: %d of %d tail starts skipped (more than %d walks)" % (ws["tail_starts_skipped"], ws["tail_starts"], ws["max_walks"])
        out.write(line + "\n")
        if coord == "topology":
            cs = graph.seed_coord_stats()
            out.write("seed coordinate: topology, %d trees, %d cycles cut, %d + %d rounds\n" % (cs["trees"], cs["cycles_cut"], cs["cycle_rounds"], cs["depth_rounds"]))
        by_locus = getattr(params, "seedLoci", False)
        # seeds and job plan on the device from one upload of the reads (Graph.prepare_seeded), in the order the reads are aligned in;
        # a library or back end without that goes the two-call way
        try:
            seeded = graph.prepare_seeded([r.sequence for r in reads[::-1]], dict(max_seeds=params.seedMax), by_locus,
                                          params.initialBandwidth, params.rampBandwidth, flags=flags)
        except binding.SeededUnsupported:
            seeded = None
        if seeded is not None:
            found = seeded.seeds()
            for field in ("seeds", "support", "n_hits", "truncated", "locus_hits", "locus_span", "n_loci"):     # (back into the reads' order)
                if getattr(found, field) is not None:
                    setattr(found, field, getattr(found, field)[::-1])
        else:
            found = graph.find_seeds([r.sequence for r in reads], loci=by_locus, max_seeds=params.seedMax)
        seeds_of = {i: s for i, s in enumerate(found.seeds) if s}
        out.write("seeds found for %d of %d reads\n" % (len(seeds_of), len(reads)))
        if by_locus:
            out.write("one seed per locus: %d seeds from %d loci\n" % (sum(len(s) for s in found.seeds), sum(found.n_loci)))

    # the reference pops reads from the back of the list (Aligner.cpp:113-117)
    order = list(range(len(reads)))[::-1]
    with_seeds = [i for i in order if i in seeds_of]
    results = {}
    pile = graph.pileup("bases") if want_pileup or want_sites else None
    edge_pile = graph.pileup("edges") if want_edges or want_supported else None
    piles = [p for p in (pile, edge_pile) if p is not None]       # (one flagged batch is added to each in turn)
    if find_seeds and seeded is not None:
        try:
            seeded.run()
            for i, r in zip(order, seeded.collect()):
                if i in seeds_of:
                    results[i] = r
            for p in piles:
                p.add(seeded)
        finally:
            seeded.close()
    elif with_seeds:
        batch = graph.prepare([reads[i].sequence for i in with_seeds], [seeds_of[i] for i in with_seeds],
                              params.initialBandwidth, params.rampBandwidth, flags=flags)
        batch.run()
        for i, r in zip(with_seeds, batch.collect()):
            results[i] = r
        for p in piles:
            p.add(batch)
    written = []
    left = len(reads)
    for i in order:
        left -= 1
        rd = reads[i]
        out.write("thread 0 %d left\n" % left)
        out.write("read %s size %dbp\n" % (rd.seq_id, len(rd.sequence)))
        if i not in results:
            for s in (out, err):
                s.write("read %s has no seed hits\n" % rd.seq_id)
                s.write("read %s alignment failed\n" % rd.seq_id)
            continue
        r = results[i]
        if r["status"] == binding.GA_S_ASSERTION:
            for s in (out, err):
                s.write("read %salignment failed (assertion!)\n" % rd.seq_id)      # sic: no blank in the reference (Aligner.cpp:146)
            continue
        if r["status"] != 0:
            for s in (out, err):
                s.write("read %s alignment failed (%s)\n" % (rd.seq_id, binding.status_string(r["status"], lib_path)))
            continue
        out.write("read %s took 0ms\n" % rd.seq_id)
        if r["failed"] or r["score"] == 0x7FFFFFFF:
            for s in (out, err):
                s.write("read %s alignment failed\n" % rd.seq_id)
            continue
        out.write("read %s score %d\n" % (rd.seq_id, r["score"]))
        if r["score"] > len(rd.sequence) * 0.25:
            err.write("read %s score is poor: %d\n" % (rd.seq_id, r["score"]))
        out.write("read %s alignment positions: %d-%d (read %dbp)\n" % (rd.seq_id, r["alignment_start"], r["alignment_end"], len(rd.sequence)))
        out.write("thread 0 successfully aligned read %s with 0 cells\n" % rd.seq_id)
        written.append((rd, r))
        if params.perReadFiles:
            fn = os.path.join(params.outputDir, _safe("alignment_0_%s.gam" % rd.seq_id))
            out.write("write alignment to %s\n" % fn)
            with open(fn, "wb") as f:
                f.write(gam_group([encode_alignment(rd.seq_id, rd.sequence, r)]))
            out.write("alignment write finished\n")
            tn = os.path.join(params.outputDir, _safe("trace_0_%s.trace" % rd.seq_id))
            out.write("write trace to %s\n" % tn)
            with open(tn, "w") as f:
                for t in r["trace"]:
                    f.write("%d %d %d %d %d %s %s\n" % (t[0], t[1], t[2], t[3], t[4], chr(int(t[5])), chr(int(t[6]))))
            out.write("trace write finished\n")
    out.write("thread 0 finished with %d alignments\n" % len(written))
    err.write("final result has %d alignments\n" % len(written))
    if params.alignmentFile != "":
        with open(params.alignmentFile, "wb") as f:
            f.write(gam_group([encode_alignment(rd.seq_id, rd.sequence, r) for rd, r in written]))
    if getattr(params, "opsFile", ""):
        # per aligned read, in output order: name, matches, mismatches, insertions, deletions, identity = matches / all cells, the runs
        with open(params.opsFile, "w") as f:
            for rd, r in written:
                c = r["op_counts"]
                cells = c["match"] + c["mismatch"] + c["insertion"] + c["deletion"]
                f.write("%s\t%d\t%d\t%d\t%d\t%.6f\t%s\n" % (rd.seq_id, c["match"], c["mismatch"], c["insertion"], c["deletion"],
                                                             c["match"] / cells if cells else 0.0, binding.ops_string(r["ops"])))
    if getattr(params, "correctedFile", ""):
        # per aligned read, in output order: the backward part's bases and the forward part's on one line (nothing is stitched at the seed)
        with open(params.correctedFile, "w") as f:
            for rd, r in written:
                f.write(">%s\n%s\n" % (rd.seq_id, r["path_seq"].decode()))
    if want_pileup:
        write_pileup(params.pileupFile, pile, [r for r in results.values() if r["status"] == 0 and not r["failed"]])
    if want_edges:
        write_edge_support(params.edgeSupportFile, edge_pile)
    if want_sites:
        write_sites(params.sitesFile, pile, params.sitesFold, params.sitesMinDepth, params.sitesMinAlt, params.sitesFrac)
    if want_supported:
        write_supported_edges(params.supportedEdgesFile, edge_pile, params.minEdgeSupport)
    return [(rd.seq_id, r) for rd, r in written]


def write_edge_support(path, pile):
    """one line per edge of the bigraph whose folded count (the directed edge and its mirror summed) is >= 1: from_id from_reverse to_id
    to_reverse count, ordered by those.  The written counts must add up to what the pileup says it was given"""
    folded = pile.edge_support()
    written = 0
    with open(path, "w") as f:
        for (a, b), c in sorted(folded.items()):
            if c >= 1:
                written += c
                f.write("%d %d %d %d %d\n" % (a >> 1, a & 1, b >> 1, b & 1, c))
    total = int(pile.stats()["items_added"])
    if written != total:
        raise RuntimeError("edge support: %d counts written, %d items added to the pileup" % (written, total))


def write_sites(path, pile, fold, min_depth, min_alt, frac):
    """one line per site of the query (Pileup.sites: selected on the device, neither the planes nor a TraceItem list come down): node id,
    strand (+ / -), offset, graph base, then the eight counts -- folded onto the forward copy with `fold` --, in entry order"""
    sites = pile.sites(fold=fold, min_depth=min_depth, min_alt=min_alt, alt_frac=frac)
    with open(path, "w") as f:
        for s in sites:
            f.write("%d\t%s\t%d\t%s\t%s\n" % (int(s["node_id"]), "-" if s["reverse"] else "+", int(s["offset"]), s["graph_char"].decode(),
                                                "\t".join(str(int(c)) for c in s["counts"])))


def write_supported_edges(path, pile, min_support):
    """the lines of write_edge_support restricted to a folded count >= min_support, from one fold query (Pileup.supported_edges)"""
    with open(path, "w") as f:
        for (a, b), c in sorted(pile.supported_edges(min_support).items()):
            f.write("%d %d %d %d %d\n" % (a >> 1, a & 1, b >> 1, b & 1, c))


def write_pileup(path, pile, aligned):
    """one line per column with any nonzero plane: node id, strand (+ / -), offset, graph base, then the eight counts
    (binding.PILEUP_PLANES), ordered by node id, strand, offset.  The nodes and their bases are those of the aligned reads' TraceItem
    lists -- by the rule nothing is counted anywhere else, which the total over the whole pileup confirms"""
    base_of = {}
    for r in aligned:
        for t in r["trace"]:
            if int(t[4]) != 5:
                base_of.setdefault((int(t[0]), int(t[2])), {})[int(t[1])] = chr(int(t[5]))
    written = 0
    with open(path, "w") as f:
        for node_id, reverse in sorted(base_of):
            # (an item on a dummy node carries id 0, which the graph need not have; any other failure is an error)
            if pile.L.ga_graph_node_columns(pile.g.h, 2 * node_id + reverse, None, None) == binding.GA_E_INVALID:
                continue
            counts = pile.node(node_id, bool(reverse))
            for offset in np.flatnonzero(counts.any(axis=0)):
                col = counts[:, offset]
                written += int(col.sum())
                f.write("%d\t%s\t%d\t%s\t%s\n" % (node_id, "-" if reverse else "+", offset, base_of[(node_id, reverse)].get(int(offset), "N"),
                                                    "\t".join(str(int(c)) for c in col)))
    total = int(pile.counts().astype(np.int64).sum())
    if written != total:
        raise RuntimeError("pileup: %d counts written, %d in the pileup" % (written, total))


def parse_args(argv, err=sys.stderr):
    """AlignerMain.cpp:18-107"""
    p = AlignerParams()
    initial_full_band = False
    coord_given = False
    opts, _ = getopt.getopt(argv, "g:f:a:t:B:A:is:d:MSb:", ["find-seeds", "seed-k=", "seed-max=", "seed-walks=", "seed-loci", "seed-coord=", "ops-out=", "corrected-out=", "pileup-out=", "edge-support-out=",
                                                             "sites-out=", "sites-min-depth=", "sites-min-alt=", "sites-frac=", "sites-fold", "supported-edges-out=", "min-edge-support="])
    for o, a in opts:
        if o == "-g":
            p.graphFile = a
        elif o == "-f":
            p.fastqFile = a
        elif o == "-a":
            p.alignmentFile = a
        elif o == "-t":
            p.numThreads = int(a)
        elif o == "-b":
            p.initialBandwidth = int(a)
        elif o == "-B":
            p.rampBandwidth = int(a)
        elif o == "-A":
            p.auggraphFile = a
        elif o == "-i":
            initial_full_band = True
        elif o == "-s":
            p.seedFile = a
        elif o == "-d":
            p.dynamicRowStart = int(a)
        elif o == "--find-seeds":
            p.findSeeds = True
        elif o == "--seed-k":
            p.seedK = int(a)
        elif o == "--seed-max":
            p.seedMax = int(a)
        elif o == "--seed-walks":
            p.seedWalks = int(a)
        elif o == "--seed-loci":
            p.seedLoci = True
        elif o == "--seed-coord":
            p.seedCoord = a
            coord_given = True
        elif o == "--ops-out":
            p.opsFile = a
        elif o == "--corrected-out":
            p.correctedFile = a
        elif o == "--pileup-out":
            p.pileupFile = a
        elif o == "--edge-support-out":
            p.edgeSupportFile = a
        elif o == "--sites-out":
            p.sitesFile = a
        elif o == "--sites-min-depth":
            p.sitesMinDepth = int(a)
        elif o == "--sites-min-alt":
            p.sitesMinAlt = int(a)
        elif o == "--sites-frac":
            num, _, den = a.partition("/")
            p.sitesFrac = (int(num), int(den) if den else 1)
        elif o == "--sites-fold":
            p.sitesFold = True
        elif o == "--supported-edges-out":
            p.supportedEdgesFile = a
        elif o == "--min-edge-support":
            p.minEdgeSupport = int(a)

    def stop(msg):
        err.write(msg + "\n")
        raise SystemExit(0)
    if p.dynamicRowStart % 64 != 0:
        stop("dynamic row start has to be a multiple of 64")
    if p.sitesMinDepth < 1 or p.sitesMinAlt < 0 or not (0 <= p.sitesFrac[0] <= p.sitesFrac[1] and 1 <= p.sitesFrac[1] <= 65535):
        stop("--sites-min-depth must be >= 1 and --sites-frac NUM/DEN a fraction of at most 1 with DEN of 1..65535")
    if p.minEdgeSupport < 1:
        stop("--min-edge-support must be >= 1")
    if p.numThreads < 1:
        stop("number of threads must be >= 1")
    if p.initialBandwidth < 2:
        stop("bandwidth must be >= 2")
    if p.rampBandwidth != 0 and p.rampBandwidth <= p.initialBandwidth:
        stop("backup bandwidth must be higher than initial bandwidth")
    if not initial_full_band and p.seedFile == "" and not p.findSeeds:
        stop("either initial full band or seed file must be set")
    if p.findSeeds and p.seedFile != "":
        stop("--find-seeds stands in for the seed file: give one of the two")
    if p.findSeeds and not (11 <= p.seedK <= 31 and 1 <= p.seedMax <= 64):
        stop("--seed-k must be 11..31 and --seed-max 1..64")
    if not 0 <= p.seedWalks <= 256 or (p.seedWalks and not p.findSeeds):
        stop("--seed-walks must be 0..256 and goes with --find-seeds")
    if p.seedLoci and not p.findSeeds:
        stop("--seed-loci goes with --find-seeds")
    if p.seedCoord not in ("file", "topology") or (coord_given and not p.findSeeds):
        stop("--seed-coord must be file or topology and goes with --find-seeds")
    if initial_full_band:
        stop("-i (alignment without seeds) is not part of the GPU hot path; it asserts in the reference snapshot (GraphAligner.h:1138)")
    if p.auggraphFile != "":
        stop("-A (augmented graph output) is outside the hot path and not provided")
    return p


def main(argv=None):
    align_reads(parse_args(sys.argv[1:] if argv is None else argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
