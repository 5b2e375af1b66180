"""phanotate.py-compatible command line (same flags as file_handling.get_args, file_handling.py:42-68).

    phanotate.py [-o OUT] [-f FORMAT] [-s atg:0.85,gtg:0.10,ttg:0.05] [-e tag,tga,taa] [-l 90] [-d] infile

All contigs of the input go through the GPU in batches (phanotate.py:40 loops over them one by one).
Inputs of more than one batch stream through phanotate_amd.pipeline.Pipeline: two batches in flight per GPU, and with --gpus N
the batches go round the first N GPUs of the node — one process, one host thread and two libphx contexts per GPU, no process group
(contigs never interact, phanotate.py:40,56).  `python -m torch.distributed.run --nproc-per-node N phanotate.py ...` still works:
contigs are then sharded across ranks (phanotate_amd.shard) and rank 0 writes the output in input order.
"""
import argparse
import os
import sys

from . import __version__
from .api import Annotator, make_params
from .writers import FORMATS, write

STATUS_TEXT = {-2: "letter outside the nucleotide alphabet (the reference raises KeyError)", -3: "contig shorter than 6 bases", -4: "a tRNA hit lies outside the contig",
               -6: "parallel edges are forbidden (graphs.py:74)", -7: "integer overflow in path sums", -8: "an open reading frame of more than 65535 codons", -9: "negative cycle"}


def is_valid_file(x):
    if not os.path.exists(x):
        raise argparse.ArgumentTypeError("{0} does not exist".format(x))
    return x


def get_args(argv=None):
    usage = "phanotate.py [-opt1, [-opt2, ...]] infile"
    p = argparse.ArgumentParser(description="PHANOTATE: A phage genome annotator (MI355X-native path)", formatter_class=argparse.RawTextHelpFormatter, usage=usage)
    p.add_argument("infile", type=is_valid_file, help="input file in fasta format")
    p.add_argument("-o", "--outfile", action="store", default=sys.stdout, type=argparse.FileType("w"), help="where to write the output [stdout]")
    p.add_argument("-f", "--format", help="Output the features in the specified format [tabular]", type=str, default="tabular", choices=FORMATS)
    p.add_argument("-s", "--start_codons", action="store", default="atg:0.85,gtg:0.10,ttg:0.05", dest="start_codons", help="comma separated list of start codons and frequency [atg:0.85,gtg:0.10,ttg:0.05]")
    p.add_argument("-e", "--stop_codons", action="store", default="tag,tga,taa", dest="stop_codons", help="comma separated list of stop codons [tag,tga,taa]")
    p.add_argument("-l", "--minlen", action="store", type=int, default=90, dest="min_orf_len", help="to store a variable")
    p.add_argument("-d", "--dump", action="store_true")
    p.add_argument("-V", "--version", action="version", version=__version__)
    p.add_argument("--device", type=int, default=None, help="GPU ordinal [LOCAL_RANK or 0]")
    p.add_argument("--gpus", type=int, default=1, help="spread the batches over the first N GPUs of the node, from this one process [1]")
    p.add_argument("--batch-bases", type=int, default=400_000_000, help="bases per GPU batch [4e8]")
    p.add_argument("--margins", metavar="FILE", default=None, help="also write every ORF some source-to-target path runs through, with its path margin (DESIGN.md §11), to FILE")
    p.add_argument("--drop-margins", metavar="FILE", default=None, help="also write every called gene with its drop margin, the cost of the best path without it (DESIGN.md §12), to FILE")
    p.add_argument("--drop-replacements", metavar="FILE", default=None, help="also write every called gene with what the best path without it calls instead (DESIGN.md §13) to FILE")
    p.add_argument("--start-drops", metavar="FILE", default=None, help="also write every called gene with the cost of refusing its start and the start the best annotation then takes for its stop (DESIGN.md §17) to FILE")
    p.add_argument("--alt-starts", metavar="FILE", default=None, help="also write, for every called gene and every other start of its stop, the cost of the best annotation that takes that start instead (DESIGN.md §18) to FILE")
    p.add_argument("--forbid", metavar="FILE", default=None, help="ORFs to refuse in a second annotation (DESIGN.md §14): lines whose first four columns are START STOP FRAME CONTIG as the tabular output prints a gene; needs --reannotation")
    p.add_argument("--require", metavar="FILE", default=None, help="ORFs to keep in a second annotation (DESIGN.md §16), in the format of --forbid; alone or with --forbid; needs --reannotation, which then carries a #unmet: line per contig")
    p.add_argument("--evidence", metavar="FILE", default=None, help="per-ORF bonuses and penalties for a second annotation (DESIGN.md §19), in the format of --forbid with a fifth column BIAS: a finite number of SCORE units added to the ORF's weight (negative: support; an ORF named twice gets the sum); alone or with --forbid, not with --require; needs --reannotation, whose #delta: may then be negative")
    p.add_argument("--evidence-scan", metavar=("FILE", "OUT"), nargs=2, default=None, help="also take every line of FILE (the format of --evidence) on its own: write to OUT, per line, the cost and the effect of the best annotation under that one bias (DESIGN.md §20); independent of --evidence / --reannotation")
    p.add_argument("--curated-scan", metavar=("FILE", "OUT"), nargs=2, default=None, help="also take every line of FILE (the format of --evidence) on its own UNDER the ORFs of --require and --forbid: write to OUT, per contig, the baseline under the two sets alone and, per line, the cost and the effect of that one bias against the baseline (DESIGN.md §27); needs --require and --reannotation")
    p.add_argument("--reannotation", metavar="OUT", default=None, help="write the annotation without the ORFs of --forbid (keeping those of --require, or under the biases of --evidence) to OUT: the tabular block of every contig with a #delta: header line")
    p.add_argument("--remargins", metavar="FILE", default=None, help="also write every ORF with its path margin on the graph of the second annotation (under --forbid / --evidence; DESIGN.md §21) to FILE, in the format of --margins; needs --reannotation, not with --require")
    p.add_argument("--pin-margins", metavar="FILE", default=None, help="also write every ORF with its path margin and the kept ORFs of --require that the best path through it gives up (DESIGN.md §24) to FILE: the format of --margins with a LOST column behind MARGIN; needs --require and --reannotation")
    p.add_argument("--single-device-ranks", action="store_true", help=argparse.SUPPRESS)  # tests: every rank of a sharded launch on GPU `--device` (gloo-only group)
    args = p.parse_args(argv)
    if args.margins is not None and args.dump:
        p.error("argument --margins: not allowed with argument -d/--dump")
    if args.margins is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("argument --margins: not available under a multi-rank launch")
    if args.drop_margins is not None and args.dump:
        p.error("argument --drop-margins: not allowed with argument -d/--dump")
    if args.drop_margins is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("argument --drop-margins: not available under a multi-rank launch")
    if args.drop_replacements is not None and args.dump:
        p.error("argument --drop-replacements: not allowed with argument -d/--dump")
    if args.drop_replacements is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("argument --drop-replacements: not available under a multi-rank launch")
    if args.start_drops is not None and args.dump:
        p.error("argument --start-drops: not allowed with argument -d/--dump")
    if args.start_drops is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("argument --start-drops: not available under a multi-rank launch")
    if args.start_drops is not None and int(args.gpus) > 1:  # the scenarios work on the batch resident on one context
        p.error("argument --start-drops: not available with --gpus above 1")
    if args.alt_starts is not None and args.dump:
        p.error("argument --alt-starts: not allowed with argument -d/--dump")
    if args.alt_starts is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("argument --alt-starts: not available under a multi-rank launch")
    if args.alt_starts is not None and int(args.gpus) > 1:  # the scenarios work on the batch resident on one context
        p.error("argument --alt-starts: not available with --gpus above 1")
    if args.evidence_scan is not None and args.dump:
        p.error("argument --evidence-scan: not allowed with argument -d/--dump")
    if args.evidence_scan is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("argument --evidence-scan: not available under a multi-rank launch")
    if args.evidence_scan is not None and int(args.gpus) > 1:  # the scenarios work on the batch resident on one context
        p.error("argument --evidence-scan: not available with --gpus above 1")
    if args.curated_scan is not None and args.dump:
        p.error("argument --curated-scan: not allowed with argument -d/--dump")
    if args.curated_scan is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("argument --curated-scan: not available under a multi-rank launch")
    if args.curated_scan is not None and int(args.gpus) > 1:  # the scenarios work on the batch resident on one context
        p.error("argument --curated-scan: not available with --gpus above 1")
    if args.curated_scan is not None and args.require is None:
        p.error("argument --curated-scan: needs --require")
    if args.remargins is not None and args.dump:
        p.error("argument --remargins: not allowed with argument -d/--dump")
    if args.remargins is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("argument --remargins: not available under a multi-rank launch")
    if args.remargins is not None and int(args.gpus) > 1:  # the re-annotation works on the batch resident on one context
        p.error("argument --remargins: not available with --gpus above 1")
    if args.remargins is not None and args.require is not None:  # (margins under required ORFs: DESIGN.md §21, Limits)
        p.error("argument --remargins: not allowed with argument --require")
    if args.remargins is not None and args.reannotation is None:
        p.error("argument --remargins: needs --reannotation")
    if args.pin_margins is not None and args.dump:
        p.error("argument --pin-margins: not allowed with argument -d/--dump")
    if args.pin_margins is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("argument --pin-margins: not available under a multi-rank launch")
    if args.pin_margins is not None and int(args.gpus) > 1:  # the re-annotation works on the batch resident on one context
        p.error("argument --pin-margins: not available with --gpus above 1")
    if args.pin_margins is not None and args.require is None:
        p.error("argument --pin-margins: needs --require")
    if args.pin_margins is not None and args.reannotation is None:
        p.error("argument --pin-margins: needs --reannotation")
    for flag, val in (("--forbid", args.forbid), ("--require", args.require), ("--evidence", args.evidence), ("--reannotation", args.reannotation)):
        if val is not None and args.dump:
            p.error("argument %s: not allowed with argument -d/--dump" % flag)
        if val is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error("argument %s: not available under a multi-rank launch" % flag)
    if args.evidence is not None and args.require is not None:  # (required sets and biases in one solve: DESIGN.md §19, Limits)
        p.error("argument --evidence: not allowed with argument --require")
    if args.evidence is not None and args.reannotation is None:
        p.error("argument --evidence: needs --reannotation")
    if args.evidence is not None and int(args.gpus) > 1:
        p.error("argument --evidence: not available with --gpus above 1")
    if args.require is None and args.evidence is None and (args.forbid is None) != (args.reannotation is None):
        p.error("arguments --forbid and --reannotation: each needs the other")
    if args.require is not None and args.reannotation is None:
        p.error("argument --require: needs --reannotation")
    if args.forbid is not None and int(args.gpus) > 1:  # the re-annotation works on the batch resident on one context
        p.error("argument --forbid: not available with --gpus above 1")
    if args.require is not None and int(args.gpus) > 1:
        p.error("argument --require: not available with --gpus above 1")
    return args


def format_pin_margins(names, status, offsets, records, lost):
    """--pin-margins FILE for a run of contigs, as bytes: format_margins' block with a LOST column behind MARGIN — per contig with status
    >= 0 "#id:\t<name>", the header, one row per ORF with through == 1 (START STOP FRAME CONTIG SCORE MARGIN LOST CALLED), ordered by
    left, right, strand.  `lost` is parallel to `records` (Annotator.pinmargins())."""
    out = []
    for i, nm in enumerate(names):
        if status[i] < 0:
            continue
        out.append("#id:\t%s\n#START\tSTOP\tFRAME\tCONTIG\tSCORE\tMARGIN\tLOST\tCALLED\n" % nm)
        rec, lo = records[offsets[i]:offsets[i + 1]], lost[offsets[i]:offsets[i + 1]]
        rows = sorted((int(r["left"]), int(r["right"]), int(r["strand"]), k) for k, r in enumerate(rec) if r["through"])
        for left, right, strand, k in rows:
            a, z = (right, left) if strand < 0 else (left, right)  # as the tabular writer
            out.append("%d\t%d\t%s\t%s\t%E\t%E\t%d\t%d\n" % (a, z, "-" if strand < 0 else "+", nm, float(rec["score"][k]), float(rec["margin"][k]), int(lo[k]), 1 if rec["called"][k] else 0))
    return "".join(out).encode()


class ForbidError(ValueError):
    """A line of --forbid that cannot be used; the message quotes it."""


def parse_forbid(lines, flag="--forbid"):
    """--forbid FILE (--require FILE: `flag` names it in the messages): [(left, right, strand, contig name, the line)] for every line that is not empty or a '#' line.  The first four
    columns are START STOP FRAME CONTIG as write_tabular prints a gene (START > STOP on the reverse strand); further columns are ignored."""
    out = []
    for raw in lines:
        line = raw.rstrip("\r\n")
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        col = line.split("\t") if "\t" in line else line.split()
        try:
            if len(col) < 4 or col[2].strip() not in ("+", "-"):
                raise ValueError
            a, z = int(col[0]), int(col[1])
        except ValueError:
            raise ForbidError("%s: not START STOP FRAME CONTIG: %r" % (flag, line)) from None
        strand = 1 if col[2].strip() == "+" else -1
        out.append((min(a, z), max(a, z), strand, col[3].strip(), line))
    return out


def resolve_forbid(entries, names, lookup, flag="--forbid"):
    """Per contig of `names` the ORF indices the entries of parse_forbid name (None: none); lookup(i, left, right, strand) is
    Annotator.orf_index.  A line that names no ORF of its contig raises ForbidError quoting the line."""
    where = {}
    for i, nm in enumerate(names):
        where.setdefault(nm, i)
    out = [None] * len(names)
    for left, right, strand, contig, line in entries:
        try:
            i = where[contig]
            k = lookup(i, left, right, strand)
        except KeyError:
            raise ForbidError("%s: no such ORF in its contig: %r" % (flag, line)) from None
        if out[i] is None:
            out[i] = []
        out[i].append(k)
    return out


def parse_evidence(lines, flag="--evidence"):
    """--evidence FILE: parse_forbid's entries with a sixth member, the BIAS of the line's fifth column: a finite float in SCORE units
    (negative: support).  A line without one, or with one that is no finite number, raises ForbidError quoting the line."""
    import math

    out = []
    for entry in parse_forbid(lines, flag):
        line = entry[4]
        col = line.split("\t") if "\t" in line else line.split()
        try:
            b = float(col[4])
            if not math.isfinite(b):
                raise ValueError
        except (IndexError, ValueError):
            raise ForbidError("%s: no finite BIAS in the fifth column: %r" % (flag, line)) from None
        out.append(entry + (b,))
    return out


def resolve_evidence(entries, names, lookup, flag="--evidence"):
    """Per contig of `names` the (ORF index, BIAS) pairs the entries of parse_evidence name (None: none), as Annotator.evidence takes them:
    an ORF named twice appears twice and gets the sum there.  Errors as resolve_forbid."""
    where = {}
    for i, nm in enumerate(names):
        where.setdefault(nm, i)
    out = [None] * len(names)
    for left, right, strand, contig, line, b in entries:
        try:
            i = where[contig]
            k = lookup(i, left, right, strand)
        except KeyError:
            raise ForbidError("%s: no such ORF in its contig: %r" % (flag, line)) from None
        if out[i] is None:
            out[i] = []
        out[i].append((k, b))
    return out


def format_evidence_scan(names, status, offsets, records):
    """--evidence-scan FILE OUT: per contig with status >= 0 "#id:\t<name>", the header, one row per record of Annotator.evidence_scan()
    (a line of FILE, taken on its own): the ORF's START STOP FRAME as the tabular output prints a gene, repr(bias), DELTA — repr(delta),
    or "cycle" (the bonus makes a cycle negative: PHX_S_NEGCYCLE) or "inf" (no path, or no result) —, whether the new annotation calls the
    ORF (1 / 0), and the genes the run's annotation loses and gains."""
    import io

    import numpy as np

    buf = io.StringIO()
    for i, nm in enumerate(names):
        if status[i] < 0:
            continue
        buf.write("#id:\t" + nm + "\n#START\tSTOP\tFRAME\tBIAS\tDELTA\tCALLED\tREMOVED\tADDED\n")
        for r in records[offsets[i]:offsets[i + 1]]:
            rev = r["strand"] < 0
            left, right = (int(r["right"]), int(r["left"])) if rev else (int(r["left"]), int(r["right"]))  # locus.py:44-46
            if r["status"] == -9:
                delta = "cycle"
            elif r["status"] != 0 or not np.isfinite(r["delta"]):
                delta = "inf"
            else:
                delta = repr(float(r["delta"]))
            buf.write("%d\t%d\t%s\t%s\t%s\t%d\t%d\t%d\n" % (left, right, chr(44 - (-1 if rev else 1)), repr(float(r["bias"])), delta, int(r["called"]), int(r["n_removed"]),
                                                          int(r["n_added"])))
    return buf.getvalue()


def format_curated_scan(names, status, offsets, records):
    """--curated-scan FILE OUT: per contig with status >= 0 "#id:\t<name>", for a contig with records "#base:\t<DELTA>\t<unmet>" — the
    baseline under --require / --forbid alone, DELTA as below —, the header, and one row per record of Annotator.curated_scan() (a line of
    FILE, taken on its own under the two sets): format_evidence_scan's columns, REMOVED and ADDED counted against the baseline's genes,
    and UNMET, the required ORFs the new annotation does not call."""
    import io

    import numpy as np

    def cost(st, delta):
        return "cycle" if st == -9 else "inf" if st != 0 or not np.isfinite(delta) else repr(float(delta))

    buf = io.StringIO()
    for i, nm in enumerate(names):
        if status[i] < 0:
            continue
        buf.write("#id:\t" + nm + "\n")
        recs = records[offsets[i]:offsets[i + 1]]
        if len(recs):
            buf.write("#base:\t%s\t%d\n" % (cost(recs[0]["base_status"], recs[0]["base_delta"]), int(recs[0]["base_unmet"])))
        buf.write("#START\tSTOP\tFRAME\tBIAS\tDELTA\tCALLED\tREMOVED\tADDED\tUNMET\n")
        for r in recs:
            rev = r["strand"] < 0
            left, right = (int(r["right"]), int(r["left"])) if rev else (int(r["left"]), int(r["right"]))  # locus.py:44-46
            buf.write("%d\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%d\n" % (left, right, chr(44 - (-1 if rev else 1)), repr(float(r["bias"])), cost(r["status"], r["delta"]), int(r["called"]),
                                                                int(r["n_removed"]), int(r["n_added"]), int(r["unmet"])))
    return buf.getvalue()


def format_reannotation(names, status, offsets, genes, delta, unmet=None):
    """--reannotation OUT: per contig with status >= 0 the block write_tabular prints, with "#delta:\t<repr(delta)>" behind its #id line
    and, with --require (unmet given), "#unmet:\t<count>" behind that."""
    import io

    from .writers import write_tabular

    buf = io.StringIO()
    for i, nm in enumerate(names):
        if status[i] < 0:
            continue
        one = io.StringIO()
        write_tabular(one, nm, genes[offsets[i]:offsets[i + 1]])
        head, rest = one.getvalue().split("\n", 1)
        buf.write(head + "\n#delta:\t" + repr(float(delta[i])) + "\n" + ("" if unmet is None else "#unmet:\t%d\n" % int(unmet[i])) + rest)
    return buf.getvalue()


def format_start_drops(names, status, offsets, records):
    """--start-drops FILE: per contig with status >= 0 "#id:\t<name>", the header, one row per called gene of the device path in path
    order (the records of Annotator.start_drops()): the gene's START STOP FRAME as the tabular output prints them, repr(drop), and the
    START STOP of the ORF of the same stop the new annotation calls, or "-" when the stop is no longer called."""
    import io

    buf = io.StringIO()
    for i, nm in enumerate(names):
        if status[i] < 0:
            continue
        buf.write("#id:\t" + nm + "\n#START\tSTOP\tFRAME\tDROP\tRESTART\n")
        for r in records[offsets[i]:offsets[i + 1]]:
            rev = r["strand"] < 0
            left, right = (int(r["right"]), int(r["left"])) if rev else (int(r["left"]), int(r["right"]))  # locus.py:44-46
            if r["restart"] >= 0:
                a, b = (int(r["restart_right"]), int(r["restart_left"])) if rev else (int(r["restart_left"]), int(r["restart_right"]))
                tail = "%d\t%d" % (a, b)
            else:
                tail = "-"
            buf.write("%d\t%d\t%s\t%s\t%s\n" % (left, right, chr(44 - (-1 if rev else 1)), repr(float(r["drop"])), tail))
    return buf.getvalue()


def format_alt_starts(names, status, offsets, records):
    """--alt-starts FILE: per contig with status >= 0 "#id:\t<name>", the header, one row per record of Annotator.alt_starts() (a called
    gene of the device path and another start of its stop, required in its place): the gene's START STOP FRAME as the tabular output
    prints them, the alternative's START, DELTA — repr(delta), or "cycle" (the alternative's edge lies on a cycle: PHX_S_NEGCYCLE),
    "unmet" (the alternative cannot be called) or "inf" (no path) —, and the genes the run's annotation loses and gains."""
    import io

    import numpy as np

    buf = io.StringIO()
    for i, nm in enumerate(names):
        if status[i] < 0:
            continue
        buf.write("#id:\t" + nm + "\n#START\tSTOP\tFRAME\tALT\tDELTA\tREMOVED\tADDED\n")
        for r in records[offsets[i]:offsets[i + 1]]:
            rev = r["strand"] < 0
            left, right = (int(r["right"]), int(r["left"])) if rev else (int(r["left"]), int(r["right"]))  # locus.py:44-46
            alt = int(r["alt_right"]) if rev else int(r["alt_left"])
            if r["status"] == -9:
                delta = "cycle"
            elif r["unmet"] != 0:
                delta = "unmet"
            elif r["status"] != 0 or not np.isfinite(r["delta"]):
                delta = "inf"
            else:
                delta = repr(float(r["delta"]))
            buf.write("%d\t%d\t%s\t%d\t%s\t%d\t%d\n" % (left, right, chr(44 - (-1 if rev else 1)), alt, delta, int(r["n_removed"]), int(r["n_added"])))
    return buf.getvalue()


def dump_edges(out, ann, i, seq=None, start_codons="atg:0.85,gtg:0.10,ttg:0.05"):
    """-d/--dump (phanotate.py:58,61): one line per edge, repr(src) TAB repr(dst) TAB str(weight*1000), in the reference's
    Graph.iteredges order, the weights as the reference's 28-digit Decimal values (phx_dump_text)."""
    out.write(ann.dump_text(i).decode())


def format_tabular(names, status, offsets, genes):
    """locus.py:39-56 for a run of contigs, as bytes (libphx's phx_format_tabular)."""
    import ctypes as C

    import numpy as np

    from . import _lib

    L = _lib.lib()
    n = len(names)
    enc = [x.encode() for x in names]
    arr = (C.c_char_p * max(n, 1))(*enc)
    status = np.ascontiguousarray(status, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    genes = np.ascontiguousarray(genes)
    text, tlen = C.c_void_p(), C.c_int64()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = L.phx_format_tabular(n, arr, vp(genes), vp(offsets), vp(status), C.byref(text), C.byref(tlen))
    if rc:
        raise _lib.PhxError(rc, "phx_format_tabular")
    out = C.string_at(text.value, tlen.value)
    L.phx_free_text(text)
    return out


def format_margins(names, status, offsets, records):
    """--margins FILE for a run of contigs, as bytes (libphx's phx_format_margins): per contig with status >= 0 "#id:\t<name>", the
    header, one row per ORF with through == 1 (START STOP FRAME CONTIG SCORE MARGIN CALLED), ordered by left, right, strand."""
    import ctypes as C

    import numpy as np

    from . import _lib

    L = _lib.lib()
    n = len(names)
    enc = [x.encode() for x in names]
    arr = (C.c_char_p * max(n, 1))(*enc)
    status = np.ascontiguousarray(status, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    records = np.ascontiguousarray(records, _lib.MARGIN_DT)
    text, tlen = C.c_void_p(), C.c_int64()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = L.phx_format_margins(n, arr, vp(records), vp(offsets), vp(status), C.byref(text), C.byref(tlen))
    if rc:
        raise _lib.PhxError(rc, "phx_format_margins")
    out = C.string_at(text.value, tlen.value)
    L.phx_free_text(text)
    return out


def format_replacements(names, status, offsets, records, genes):
    """--drop-replacements FILE for a run of contigs, as bytes (libphx's phx_format_replacements): per contig with status >= 0
    "#id:\t<name>", the header, one row per called gene of the device path (START STOP FRAME CONTIG DROP REMOVED ADDED), in path order;
    records[k]["gene_off"] indexes genes."""
    import ctypes as C

    import numpy as np

    from . import _lib

    L = _lib.lib()
    n = len(names)
    enc = [x.encode() for x in names]
    arr = (C.c_char_p * max(n, 1))(*enc)
    status = np.ascontiguousarray(status, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    records = np.ascontiguousarray(records, _lib.REPL_DT)
    genes = np.ascontiguousarray(genes, _lib.GENE_DT)
    text, tlen = C.c_void_p(), C.c_int64()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = L.phx_format_replacements(n, arr, vp(records), vp(genes), vp(offsets), vp(status), C.byref(text), C.byref(tlen))
    if rc:
        raise _lib.PhxError(rc, "phx_format_replacements")
    out = C.string_at(text.value, tlen.value)
    L.phx_free_text(text)
    return out


def format_drops(names, status, offsets, records):
    """--drop-margins FILE for a run of contigs, as bytes (libphx's phx_format_drops): per contig with status >= 0 "#id:\t<name>", the
    header, one row per called gene of the device path (START STOP FRAME CONTIG SCORE DROP CALLED), in path order."""
    import ctypes as C

    import numpy as np

    from . import _lib

    L = _lib.lib()
    n = len(names)
    enc = [x.encode() for x in names]
    arr = (C.c_char_p * max(n, 1))(*enc)
    status = np.ascontiguousarray(status, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    records = np.ascontiguousarray(records, _lib.DROP_DT)
    text, tlen = C.c_void_p(), C.c_int64()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = L.phx_format_drops(n, arr, vp(records), vp(offsets), vp(status), C.byref(text), C.byref(tlen))
    if rc:
        raise _lib.PhxError(rc, "phx_format_drops")
    out = C.string_at(text.value, tlen.value)
    L.phx_free_text(text)
    return out


def main(argv=None):
    import json
    import time

    import numpy as np

    from .fasta import Fasta
    from .shard import partition, run_sharded_flat

    t_start = time.perf_counter()
    args = get_args(argv)
    device = args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0"))
    # the HIP runtime and the context come up (~0.2 s) on a worker thread while this one reads the FASTA file
    import threading

    ctx_box = {}

    def make_context():
        try:
            ctx_box["ann"] = Annotator(make_params(args.start_codons, args.stop_codons, args.min_orf_len), device=device)
        except BaseException as e:  # re-raised on the main thread
            ctx_box["err"] = e

    ctx_thread = threading.Thread(target=make_context, daemon=True)
    threaded = int(os.environ.get("WORLD_SIZE", "1")) == 1  # (sharded runs bring torch.distributed up first, on this thread)
    if threaded:
        ctx_thread.start()

    def drop_context():  # every early exit: never leave the interpreter while the worker is still inside hipInit / phx_create
        if threaded:
            ctx_thread.join()
        if "ann" in ctx_box:
            ctx_box.pop("ann").close()

    try:
        fa = Fasta(args.infile)
    except BaseException:
        drop_context()
        raise
    if not len(fa) or not int(fa.lens.sum()):
        drop_context()
        sys.stdout.write("Error: no sequences found in infile\n")  # phanotate.py:33-35
        return 0
    t_parsed = time.perf_counter()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1:
        from .shard import init_group

        dist, _ = init_group(rank, world, device=device, single_device=args.single_device_ranks)
    if world == 1:
        ctx_thread.join()
    else:
        make_context()
    if "err" in ctx_box:
        raise ctx_box["err"]
    ann = ctx_box["ann"]
    t_ctx = time.perf_counter()
    t_parts = {"upload_s": 0.0, "run_s": 0.0, "download_s": 0.0, "batches": 0}
    import shutil

    from .trna import find_trnas_many

    have_finder = bool(shutil.which("aragorn") or shutil.which("tRNAscan-SE"))

    def trnas_of(idx):  # functions.add_trnas per contig (functions.py:457-495); None: neither tool is installed
        if not have_finder:
            for _ in idx:
                sys.stderr.write("Warning: tRNAscan or Aragorn were not found, proceding without tRNA masking.\n")
            return None
        return find_trnas_many(fa.seq(int(i)) for i in idx)  # the finder processes of a batch run side by side

    if args.dump:  # the reference dumps the first contig's edges and exits (phanotate.py:58-61)
        ann.upload_raw(fa.ptrs[:1], fa.lens[:1], fa)
        ann.set_trnas(trnas_of([0]))
        ann.run()
        dump_edges(args.outfile, ann, 0, fa.seq(0), args.start_codons)
        ann.close()
        return 0

    n_total = len(fa)
    margin_parts = []  # --margins: (status, offsets, records) of every batch, in order
    drop_parts = []  # --drop-margins: the same of the drop margins
    repl_parts = []  # --drop-replacements: (status, offsets, records, genes) of every batch, in order
    start_parts = []  # --start-drops: (status, offsets, records) of every batch, in order
    alt_parts = []  # --alt-starts: the same of Annotator.alt_starts()
    reann_parts = []  # --reannotation: (status, offsets, genes, delta[, unmet]) of every batch, in order
    remargin_parts = []  # --remargins: (status, offsets, records) of Annotator.remargins() of every batch, in order
    pin_parts = []  # --pin-margins: (status, offsets, records, lost) of Annotator.pinmargins() of every batch, in order
    scan_parts = []  # --evidence-scan: (status, offsets, records) of Annotator.evidence_scan() of every batch, in order
    cscan_parts = []  # --curated-scan: (status, offsets, records) of Annotator.curated_scan() of every batch, in order
    forbid_entries = require_entries = evidence_entries = scan_entries = cscan_entries = None
    try:
        if args.curated_scan is not None:
            with open(args.curated_scan[0]) as fh:
                cscan_entries = parse_evidence(fh, "--curated-scan")
        if args.evidence_scan is not None:
            with open(args.evidence_scan[0]) as fh:
                scan_entries = parse_evidence(fh, "--evidence-scan")
        if args.evidence is not None:
            with open(args.evidence) as fh:
                evidence_entries = parse_evidence(fh)
        if args.forbid is not None:
            with open(args.forbid) as fh:
                forbid_entries = parse_forbid(fh)
        if args.require is not None:
            with open(args.require) as fh:
                require_entries = parse_forbid(fh, "--require")
    except (OSError, ForbidError) as e:
        drop_context()
        sys.stderr.write("Error: %s\n" % e)
        return 2
    mine = list(range(n_total)) if world == 1 else partition(fa.lens.tolist(), world)[rank]

    def annotate_flat(idx):  # this rank's contigs, in batches of --batch-bases, straight from the C buffer of the FASTA reader
        idx = np.asarray(idx, np.int64)
        n_gpu = max(1, int(args.gpus)) if world == 1 else 1
        # batches: at most --batch-bases each; with several GPUs at least two per GPU, so that every lane has two in flight
        limit = args.batch_bases
        if n_gpu > 1 and len(idx):
            limit = max(1, min(limit, -(-int(fa.lens[idx].sum()) // (2 * n_gpu))))
        cuts, lo = [], 0
        while lo < len(idx) or not cuts:
            hi, size = lo, 0
            while hi < len(idx) and (hi == lo or size + int(fa.lens[idx[hi]]) <= limit):
                size += int(fa.lens[idx[hi]])
                hi += 1
            cuts.append((lo, hi))
            lo = hi
            if lo >= len(idx):
                break
        t_parts["batches"] = len(cuts)
        if forbid_entries is not None or require_entries is not None or evidence_entries is not None or args.start_drops is not None or args.alt_starts is not None or scan_entries is not None:  # the re-annotation and the scenarios work on the batch resident on one context: the batches one after the other
            parts = []
            for lo, hi in cuts:
                t0 = time.perf_counter()
                ann.upload_raw(fa.ptrs[idx[lo:hi]], fa.lens[idx[lo:hi]], fa)
                ann.set_trnas(trnas_of(idx[lo:hi]))
                t1 = time.perf_counter()
                ann.run()
                t2 = time.perf_counter()
                parts.append(ann.download_flat())
                t3 = time.perf_counter()
                if args.margins is not None:  # the siblings on the same resident batch, as in the one-batch branch below
                    margin_parts.append(ann.margins())
                if args.drop_replacements is not None:
                    repl_parts.append(ann.replacements())
                if args.drop_margins is not None:
                    drop_parts.append(ann.drop_margins())
                if args.start_drops is not None:
                    start_parts.append(ann.start_drops()[:3])
                if args.alt_starts is not None:
                    alt_parts.append(ann.alt_starts()[:3])
                names = [fa.names[int(i)] for i in idx[lo:hi]]
                here = set(names)
                if scan_entries is not None:
                    scan_parts.append(ann.evidence_scan(resolve_evidence([e for e in scan_entries if e[3] in here], names, ann.orf_index, "--evidence-scan"))[:3])
                refused = resolve_forbid([e for e in forbid_entries or [] if e[3] in here], names, ann.orf_index)
                if evidence_entries is not None:
                    reann_parts.append(ann.evidence(resolve_evidence([e for e in evidence_entries if e[3] in here], names, ann.orf_index), refused))
                elif forbid_entries is None and require_entries is None:
                    pass
                elif require_entries is None:
                    reann_parts.append(ann.reannotate(refused))
                else:
                    reann_parts.append(ann.constrain(refused, resolve_forbid([e for e in require_entries if e[3] in here], names, ann.orf_index, "--require")))
                if cscan_entries is not None:  # (a scenario batch of its own: the batch's re-annotation above stays the cached one)
                    cscan_parts.append(ann.curated_scan(resolve_evidence([e for e in cscan_entries if e[3] in here], names, ann.orf_index, "--curated-scan"), refused,
                                                        resolve_forbid([e for e in require_entries if e[3] in here], names, ann.orf_index, "--require"))[:3])
                if args.remargins is not None:  # (behind the batch's re-annotation: the margins are that solve's)
                    remargin_parts.append(ann.remargins())
                if args.pin_margins is not None:  # (likewise)
                    pin_parts.append(ann.pinmargins())
                t_parts["upload_s"] += t1 - t0; t_parts["run_s"] += t2 - t1; t_parts["download_s"] += t3 - t2
        elif len(cuts) == 1 and n_gpu == 1:
            lo, hi = cuts[0]
            t0 = time.perf_counter()
            ann.upload_raw(fa.ptrs[idx[lo:hi]], fa.lens[idx[lo:hi]], fa)
            ann.set_trnas(trnas_of(idx[lo:hi]))
            t1 = time.perf_counter()
            ann.run()
            t2 = time.perf_counter()
            parts = [ann.download_flat()]
            t3 = time.perf_counter()
            if args.margins is not None:
                margin_parts.append(ann.margins())
            if args.drop_replacements is not None:  # (before the drop margins: they are then computed once)
                repl_parts.append(ann.replacements())
            if args.drop_margins is not None:
                drop_parts.append(ann.drop_margins())
            t_parts["upload_s"] += t1 - t0; t_parts["run_s"] += t2 - t1; t_parts["download_s"] += t3 - t2
        else:  # a stream of batches: two in flight per GPU, the batches round the GPUs (pipeline.Pipeline)
            from .pipeline import Pipeline

            t0 = time.perf_counter()
            pipe = Pipeline(ann.params, device=device, depth=2, devices=([device] + [d for d in range(n_gpu) if d != device][: n_gpu - 1]) if n_gpu > 1 else None, first=ann)
            t1 = time.perf_counter()
            gen = ((fa.ptrs[idx[lo:hi]], fa.lens[idx[lo:hi]], fa, (lambda a=lo, b=hi: trnas_of(idx[a:b]))) for lo, hi in cuts)
            try:
                parts = list(pipe.run(gen, margins=args.margins is not None, drop_margins=args.drop_margins is not None, replacements=args.drop_replacements is not None))
                t2 = time.perf_counter()
                k = 3
                if args.margins is not None:
                    margin_parts.extend(p[k] for p in parts)
                    k += 1
                if args.drop_margins is not None:
                    drop_parts.extend(p[k] for p in parts)
                    k += 1
                if args.drop_replacements is not None:
                    repl_parts.extend(p[k] for p in parts)
                parts = [p[:3] for p in parts]
            finally:
                pipe.close()
            t_parts["contexts_s"] = t1 - t0; t_parts["pipeline_s"] = t2 - t1; t_parts["gpus"] = n_gpu
        if len(parts) == 1:
            return parts[0]
        st = np.concatenate([p[0] for p in parts])
        genes = np.concatenate([p[2] for p in parts])
        counts = np.concatenate([np.diff(p[1]) for p in parts])
        return st, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), genes

    known = set(fa.names)
    for flag, entries in (("--forbid", forbid_entries), ("--require", require_entries), ("--evidence", evidence_entries), ("--evidence-scan", scan_entries), ("--curated-scan", cscan_entries)):
        for e in entries or []:
            if e[3] not in known:
                drop_context()
                sys.stderr.write("Error: %s: no such ORF in its contig: %r\n" % (flag, e[4]))
                return 2
    try:
        merged = run_sharded_flat(mine, annotate_flat, rank, world, dist, mine=(mine, n_total))
    except ForbidError as e:
        ann.close()
        sys.stderr.write("Error: %s\n" % e)
        return 2
    t_gpu = time.perf_counter()
    rc = 0
    t_fmt = t_gpu
    if rank == 0:
        status, offsets, genes = merged
        for i in np.nonzero(status < 0)[0]:
            sys.stderr.write("Error: contig %s: %s\n" % (fa.names[i], STATUS_TEXT.get(int(status[i]), "status %d" % int(status[i]))))
            rc = 1
        if args.format == "tabular":
            text = format_tabular(fa.names, status, offsets, genes)
            t_fmt = time.perf_counter()
            args.outfile.flush()
            if hasattr(args.outfile, "buffer"):
                args.outfile.buffer.write(text)
            else:
                args.outfile.write(text.decode())
        else:
            for i in range(n_total):
                if status[i] >= 0:
                    write(args.outfile, args.format, fa.names[i], fa.seq(i).decode(), genes[offsets[i] : offsets[i + 1]])
            t_fmt = time.perf_counter()
        args.outfile.flush()
        if args.margins is not None:
            m_status = np.concatenate([m[0] for m in margin_parts])
            m_counts = np.concatenate([np.diff(m[1]) for m in margin_parts])
            m_offsets = np.concatenate([[0], np.cumsum(m_counts)]).astype(np.int64)
            m_records = np.concatenate([m[2] for m in margin_parts])
            with open(args.margins, "wb") as fh:
                fh.write(format_margins(fa.names, m_status, m_offsets, m_records))
        if args.remargins is not None:
            x_status = np.concatenate([m[0] for m in remargin_parts])
            x_counts = np.concatenate([np.diff(m[1]) for m in remargin_parts])
            x_offsets = np.concatenate([[0], np.cumsum(x_counts)]).astype(np.int64)
            with open(args.remargins, "wb") as fh:
                fh.write(format_margins(fa.names, x_status, x_offsets, np.concatenate([m[2] for m in remargin_parts])))
        if args.pin_margins is not None:
            p_status = np.concatenate([m[0] for m in pin_parts])
            p_counts = np.concatenate([np.diff(m[1]) for m in pin_parts])
            p_offsets = np.concatenate([[0], np.cumsum(p_counts)]).astype(np.int64)
            with open(args.pin_margins, "wb") as fh:
                fh.write(format_pin_margins(fa.names, p_status, p_offsets, np.concatenate([m[2] for m in pin_parts]), np.concatenate([m[3] for m in pin_parts])))
        if args.drop_margins is not None:
            d_status = np.concatenate([m[0] for m in drop_parts])
            d_counts = np.concatenate([np.diff(m[1]) for m in drop_parts])
            d_offsets = np.concatenate([[0], np.cumsum(d_counts)]).astype(np.int64)
            d_records = np.concatenate([m[2] for m in drop_parts])
            with open(args.drop_margins, "wb") as fh:
                fh.write(format_drops(fa.names, d_status, d_offsets, d_records))
        if args.drop_replacements is not None:
            r_status = np.concatenate([m[0] for m in repl_parts])
            r_counts = np.concatenate([np.diff(m[1]) for m in repl_parts])
            r_offsets = np.concatenate([[0], np.cumsum(r_counts)]).astype(np.int64)
            r_records, r_genes, g0 = [], [], 0
            for m in repl_parts:  # (each batch's gene_off counts from its own genes)
                rr = m[2].copy()
                rr["gene_off"] += g0
                g0 += len(m[3])
                r_records.append(rr)
                r_genes.append(m[3])
            with open(args.drop_replacements, "wb") as fh:
                fh.write(format_replacements(fa.names, r_status, r_offsets, np.concatenate(r_records), np.concatenate(r_genes)))
        if args.start_drops is not None:
            s_status = np.concatenate([m[0] for m in start_parts])
            s_counts = np.concatenate([np.diff(m[1]) for m in start_parts])
            s_offsets = np.concatenate([[0], np.cumsum(s_counts)]).astype(np.int64)
            with open(args.start_drops, "w") as fh:
                fh.write(format_start_drops(fa.names, s_status, s_offsets, np.concatenate([m[2] for m in start_parts])))
        if args.alt_starts is not None:
            a_status = np.concatenate([m[0] for m in alt_parts])
            a_counts = np.concatenate([np.diff(m[1]) for m in alt_parts])
            a_offsets = np.concatenate([[0], np.cumsum(a_counts)]).astype(np.int64)
            with open(args.alt_starts, "w") as fh:
                fh.write(format_alt_starts(fa.names, a_status, a_offsets, np.concatenate([m[2] for m in alt_parts])))
        if args.evidence_scan is not None:
            e_status = np.concatenate([m[0] for m in scan_parts])
            e_counts = np.concatenate([np.diff(m[1]) for m in scan_parts])
            e_offsets = np.concatenate([[0], np.cumsum(e_counts)]).astype(np.int64)
            with open(args.evidence_scan[1], "w") as fh:
                fh.write(format_evidence_scan(fa.names, e_status, e_offsets, np.concatenate([m[2] for m in scan_parts])))
        if args.curated_scan is not None:
            c_status = np.concatenate([m[0] for m in cscan_parts])
            c_counts = np.concatenate([np.diff(m[1]) for m in cscan_parts])
            c_offsets = np.concatenate([[0], np.cumsum(c_counts)]).astype(np.int64)
            with open(args.curated_scan[1], "w") as fh:
                fh.write(format_curated_scan(fa.names, c_status, c_offsets, np.concatenate([m[2] for m in cscan_parts])))
        if args.reannotation is not None:
            q_status = np.concatenate([m[0] for m in reann_parts])
            q_counts = np.concatenate([np.diff(m[1]) for m in reann_parts])
            q_offsets = np.concatenate([[0], np.cumsum(q_counts)]).astype(np.int64)
            with open(args.reannotation, "w") as fh:
                fh.write(format_reannotation(fa.names, q_status, q_offsets, np.concatenate([m[2] for m in reann_parts]), np.concatenate([m[3] for m in reann_parts]),
                                             np.concatenate([m[4] for m in reann_parts]) if args.require is not None else None))
    t_end = time.perf_counter()
    if os.environ.get("PHX_CLI_TIMING") and rank == 0:
        sys.stderr.write("PHX_CLI_TIMING " + json.dumps({"parse_s": round(t_parsed - t_start, 4), "gpu_s": round(t_gpu - t_parsed, 4), "format_s": round(t_fmt - t_gpu, 4),
                                                         "write_s": round(t_end - t_fmt, 4), "total_s": round(t_end - t_start, 4), "bases": int(fa.lens.sum()), "genes": int(len(merged[2])),
                                                         "gpu_parts": dict({k: round(v, 4) for k, v in t_parts.items()}, context_s=round(t_ctx - t_parsed, 4))}) + "\n")
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return rc


if __name__ == "__main__":
    sys.exit(main())
