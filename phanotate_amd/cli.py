"""phanotate.py-compatible command line (same flags as file_handling.get_args, file_handling.py:42-68).

    phanotate.py [-o OUT] [-f FORMAT] [-s atg:0.85,gtg:0.10,ttg:0.05] [-e tag,tga,taa] [-l 90] [-d] infile

All contigs of the input go through the GPU in batches (phanotate.py:40 loops over them one by one).
Inputs of more than one batch stream through phanotate_amd.pipeline.Pipeline: two batches in flight per GPU, and with --gpus N
the batches go round the first N GPUs of the node — one process, one host thread and two libphx contexts per GPU, no process group
(contigs never interact, phanotate.py:40,56).  `python -m torch.distributed.run --nproc-per-node N phanotate.py ...` still works:
contigs are then sharded across ranks (phanotate_amd.shard) and rank 0 writes the output in input order.
"""
import argparse
import collections
import os
import sys

from . import __version__, _lib
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
    p.add_argument("--profile", metavar="FILE", default=None, help="also write the coding profile of every contig (DESIGN.md §34) to FILE: per stretch between neighbouring nodes of the graph, what it costs the best annotation to have it inside a forward gene, inside a reverse gene, or between genes")
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
    p.add_argument("--redrop-margins", metavar="FILE", default=None, help="also write every gene of the second annotation with its drop margin on that annotation's graph, the cost of the best path under the same --forbid / --evidence that calls nothing at its stop (DESIGN.md §29), to FILE, in the format of --drop-margins; needs --reannotation, not with --require")
    p.add_argument("--redrop-replacements", metavar="FILE", default=None, help="also write every gene of the second annotation with what the best path under the same --forbid / --evidence that calls nothing at its stop calls instead (DESIGN.md §30) to FILE, in the format of --drop-replacements; needs --reannotation, not with --require")
    p.add_argument("--pin-margins", metavar="FILE", default=None, help="also write every ORF with its path margin and the kept ORFs of --require that the best path through it gives up (DESIGN.md §24) to FILE: the format of --margins with a LOST column behind MARGIN; needs --require and --reannotation")
    p.add_argument("--pin-drop-margins", metavar="FILE", default=None, help="also write every gene of the second annotation with its drop margin under the ORFs of --require — the cost of the best annotation that calls nothing at its stop, and the kept ORFs of --require that annotation gives up (DESIGN.md §32) — to FILE: the format of --drop-margins with a LOST column behind DROP; needs --require and --reannotation")
    p.add_argument("--pin-drop-replacements", metavar="FILE", default=None, help="also write every gene of the second annotation with what the best annotation under the ORFs of --require that calls nothing at its stop calls instead, and the kept ORFs of --require it gives up (DESIGN.md §33), to FILE: the format of --drop-replacements with a LOST column behind DROP; needs --require and --reannotation")
    p.add_argument("--single-device-ranks", action="store_true", help=argparse.SUPPRESS)  # tests: every rank of a sharded launch on GPU `--device` (gloo-only group)
    args = p.parse_args(argv)
    for applies, message in _refusals(args, int(os.environ.get("WORLD_SIZE", "1"))):
        if applies:
            p.error(message)
    return args


# The relations between flags: (the flag a rule is about or None, whether it applies to args with that flag present, the message).
_RULES = (
    ("curated_scan", lambda a: a.require is None, "argument --curated-scan: needs --require"),
    ("remargins", lambda a: a.require is not None, "argument --remargins: not allowed with argument --require"),  # (margins under required ORFs: DESIGN.md §21, Limits)
    ("remargins", lambda a: a.reannotation is None, "argument --remargins: needs --reannotation"),
    ("redrop_margins", lambda a: a.require is not None, "argument --redrop-margins: not allowed with argument --require"),  # (drops under required ORFs: DESIGN.md §29, Limits)
    ("redrop_margins", lambda a: a.reannotation is None, "argument --redrop-margins: needs --reannotation"),
    ("redrop_replacements", lambda a: a.require is not None, "argument --redrop-replacements: not allowed with argument --require"),  # (as --redrop-margins: DESIGN.md §30, Limits)
    ("redrop_replacements", lambda a: a.reannotation is None, "argument --redrop-replacements: needs --reannotation"),
    ("pin_margins", lambda a: a.require is None, "argument --pin-margins: needs --require"),
    ("pin_margins", lambda a: a.reannotation is None, "argument --pin-margins: needs --reannotation"),
    ("pin_drop_margins", lambda a: a.require is None, "argument --pin-drop-margins: needs --require"),
    ("pin_drop_margins", lambda a: a.reannotation is None, "argument --pin-drop-margins: needs --reannotation"),
    ("pin_drop_replacements", lambda a: a.require is None, "argument --pin-drop-replacements: needs --require"),
    ("pin_drop_replacements", lambda a: a.reannotation is None, "argument --pin-drop-replacements: needs --reannotation"),
    ("evidence", lambda a: a.require is not None, "argument --evidence: not allowed with argument --require"),  # (required sets and biases in one solve: DESIGN.md §19, Limits)
    ("evidence", lambda a: a.reannotation is None, "argument --evidence: needs --reannotation"),
    (None, lambda a: a.require is None and a.evidence is None and (a.forbid is None) != (a.reannotation is None), "arguments --forbid and --reannotation: each needs the other"),
    ("require", lambda a: a.reannotation is None, "argument --require: needs --reannotation"),
)
# The flags of OUTPUTS and INPUTS in the order get_args looks at them.
_CHECK_ORDER = ("margins", "drop_margins", "drop_replacements", "start_drops", "alt_starts", "evidence_scan", "curated_scan", "remargins", "redrop_margins", "redrop_replacements", "pin_margins", "pin_drop_margins", "pin_drop_replacements", "profile", "forbid", "require", "evidence", "reannotation")


def _refusals(args, world):
    """(applies, message) of every refusal of get_args.  THE ORDER IS CONTRACT: a user whose command line breaks several rules is told
    the first one, and tests pin which.  Flag by flag in _CHECK_ORDER: -d/--dump, a multi-rank launch and, for a side
    output, --gpus above 1 where it works on the batch resident on one context, then the rules of _RULES about it; behind all flags the
    other rules, in their order, and last --gpus above 1 for the entry files (the re-annotation works on the resident batch too)."""
    flags = {x.dest: x.flag for x in (*OUTPUTS.values(), *INPUTS.values())}
    has = lambda dest: dest is None or getattr(args, dest) is not None
    gpus = lambda dest: (int(args.gpus) > 1, "argument %s: not available with --gpus above 1" % flags[dest])
    for dest in filter(has, _CHECK_ORDER):
        yield args.dump, "argument %s: not allowed with argument -d/--dump" % flags[dest]
        yield world > 1, "argument %s: not available under a multi-rank launch" % flags[dest]
        if dest in OUTPUTS:
            if OUTPUTS[dest].resident:
                yield gpus(dest)
            for about, applies, message in _RULES:
                if about == dest:
                    yield applies(args), message
    for about, applies, message in _RULES:
        if about not in OUTPUTS and has(about):
            yield applies(args), message
    for dest in filter(has, INPUTS):
        yield gpus(dest)


def format_pin_margins(names, status, offsets, records, lost):
    """--pin-margins FILE for a run of contigs, as bytes: format_margins' block with a LOST column behind MARGIN — per contig with status
    >= 0 "#id:\t<name>", the header, one row per ORF with through == 1 (START STOP FRAME CONTIG SCORE MARGIN LOST CALLED), ordered by
    left, right, strand.  `lost` is parallel to `records` (Annotator.pinmargins())."""
    out = []
    for nm, cut in _blocks(names, status, offsets):
        out.append("#id:\t%s\n#START\tSTOP\tFRAME\tCONTIG\tSCORE\tMARGIN\tLOST\tCALLED\n" % nm)
        rec, lo = records[cut], lost[cut]
        for _, _, _, k in sorted((int(r["left"]), int(r["right"]), int(r["strand"]), k) for k, r in enumerate(rec) if r["through"]):
            out.append("%d\t%d\t%s\t" % _ends(rec[k]) + "%s\t%E\t%E\t%d\t%d\n" % (nm, float(rec["score"][k]), float(rec["margin"][k]), int(lo[k]), 1 if rec["called"][k] else 0))
    return "".join(out).encode()


def format_pin_drops(names, status, offsets, records, lost):
    """--pin-drop-margins FILE for a run of contigs, as bytes: format_drops' block with a LOST column behind DROP — per contig with status
    >= 0 "#id:\t<name>", the header, one row per called gene of the re-annotation's device path (START STOP FRAME CONTIG SCORE DROP LOST
    CALLED), in path order.  `lost` is parallel to `records` (Annotator.pindrops())."""
    out = []
    for nm, cut in _blocks(names, status, offsets):
        out.append("#id:\t%s\n#START\tSTOP\tFRAME\tCONTIG\tSCORE\tDROP\tLOST\tCALLED\n" % nm)
        rec, lo = records[cut], lost[cut]
        for k in range(len(rec)):
            out.append("%d\t%d\t%s\t" % _ends(rec[k]) + "%s\t%E\t%E\t%d\t%d\n" % (nm, float(rec["score"][k]), float(rec["drop"][k]), int(lo[k]), 1 if rec["called"][k] else 0))
    return "".join(out).encode()


def format_pin_replacements(names, status, offsets, records, genes, lost):
    """--pin-drop-replacements FILE for a run of contigs, as bytes: format_replacements' block with a LOST column behind DROP — per contig
    with status >= 0 "#id:\t<name>", the header, one row per called gene of the re-annotation's device path (START STOP FRAME CONTIG DROP
    LOST REMOVED ADDED), in path order; records[k]["gene_off"] indexes genes, `lost` is parallel to `records`
    (Annotator.pinreplacements())."""
    def listed(gs):
        return ",".join("%s%d..%d" % (("tRNA:" if abs(int(g["frame"])) == 4 else "",) + _ends(g)[:2]) for g in gs) or "-"

    out = []
    for nm, cut in _blocks(names, status, offsets):
        out.append("#id:\t%s\n#START\tSTOP\tFRAME\tCONTIG\tDROP\tLOST\tREMOVED\tADDED\n" % nm)
        rec, lo = records[cut], lost[cut]
        for k in range(len(rec)):
            g0, g1 = int(rec["gene_off"][k]), int(rec["gene_off"][k]) + int(rec["n_removed"][k])
            out.append("%d\t%d\t%s\t" % _ends(rec[k]) + "%s\t%E\t%d\t%s\t%s\n" % (nm, float(rec["drop"][k]), int(lo[k]), listed(genes[g0:g1]), listed(genes[g1:g1 + int(rec["n_added"][k])])))
    return "".join(out).encode()


def format_profile(names, status, offsets, records, lost=None):
    """--profile FILE for a run of contigs, as bytes: per contig with status >= 0 "#id:\t<name>", the header, then one row per stretch (LO HI
    FWD REV GAP) from left to right.  LO / HI are node positions (Annotator.nodes() pos; 0 and L + 1 at the ends), the three numbers
    Annotator.profile()'s fwd / rev / gap, printed as format_margins prints a margin (INF: nothing of that kind covers the stretch).  Slots
    without extent (lo == hi) are left out; neighbouring slots with the same three values are one row.  With `lost` (int32[total, 3],
    parallel to `records`: Annotator.pinprofile()) each of the three numbers is followed by a LOST column, the kept required ORFs that the
    number gives up, and a row is one run of equal values and equal counts."""
    import numpy as np

    out = []
    for nm, cut in _blocks(names, status, offsets):
        out.append(("#id:\t%s\n#LO\tHI\tFWD\tLOST\tREV\tLOST\tGAP\tLOST\n" if lost is not None else "#id:\t%s\n#LO\tHI\tFWD\tREV\tGAP\n") % nm)
        rec = records[cut]
        ls = None if lost is None else np.asarray(lost).reshape(-1, 3)[cut][rec["lo"] != rec["hi"]]
        rec = rec[rec["lo"] != rec["hi"]]
        if not len(rec):
            continue
        first = np.ones(len(rec), bool)  # the first slot of every run of equal triples
        first[1:] = (rec["fwd"][1:] != rec["fwd"][:-1]) | (rec["rev"][1:] != rec["rev"][:-1]) | (rec["gap"][1:] != rec["gap"][:-1])
        if ls is not None:
            first[1:] |= (ls[1:] != ls[:-1]).any(axis=1)
        a = np.flatnonzero(first)
        z = np.append(a[1:], len(rec)) - 1
        for i, j in zip(a.tolist(), z.tolist()):
            if ls is not None:
                out.append("%d\t%d\t%E\t%d\t%E\t%d\t%E\t%d\n" % (int(rec["lo"][i]), int(rec["hi"][j]), float(rec["fwd"][i]), int(ls[i, 0]), float(rec["rev"][i]), int(ls[i, 1]), float(rec["gap"][i]), int(ls[i, 2])))
                continue
            out.append("%d\t%d\t%E\t%E\t%E\n" % (int(rec["lo"][i]), int(rec["hi"][j]), float(rec["fwd"][i]), float(rec["rev"][i]), float(rec["gap"][i])))
    return "".join(out).encode()


def _blocks(names, status, offsets):
    """(name, slice of its records) of every contig with status >= 0: the contigs the side outputs print a block for."""
    for i, nm in enumerate(names):
        if status[i] >= 0:
            yield nm, slice(offsets[i], offsets[i + 1])


def _ends(r):
    """(START, STOP, FRAME) of a record as the tabular output prints a gene: START > STOP on the reverse strand (locus.py:44-46)."""
    return (int(r["right"]), int(r["left"]), "-") if r["strand"] < 0 else (int(r["left"]), int(r["right"]), "+")


def _delta(status, delta, unmet=0):
    """The DELTA column: "cycle" (PHX_S_NEGCYCLE), then "unmet" (a required ORF cannot be called), then "inf" (no path, or no result),
    else repr(delta)."""
    import math

    return "cycle" if status == -9 else "unmet" if unmet != 0 else "inf" if status != 0 or not math.isfinite(delta) else repr(float(delta))


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
    return _resolve(entries, names, lookup, flag, lambda k, entry: k)


def _resolve(entries, names, lookup, flag, item):
    """The walk of resolve_forbid and resolve_evidence: item(ORF index, entry) is what a contig's list gains per entry."""
    where = {}
    for i, nm in enumerate(names):
        where.setdefault(nm, i)
    out = [None] * len(names)
    for entry in entries:
        left, right, strand, contig, line = entry[:5]
        try:
            i = where[contig]
            k = lookup(i, left, right, strand)
        except KeyError:
            raise ForbidError("%s: no such ORF in its contig: %r" % (flag, line)) from None
        if out[i] is None:
            out[i] = []
        out[i].append(item(k, entry))
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
    return _resolve(entries, names, lookup, flag, lambda k, entry: (k, entry[5]))


def format_evidence_scan(names, status, offsets, records):
    """--evidence-scan FILE OUT: per contig with status >= 0 "#id:\t<name>", the header, one row per record of Annotator.evidence_scan()
    (a line of FILE, taken on its own): the ORF's START STOP FRAME as the tabular output prints a gene, repr(bias), DELTA — repr(delta),
    or "cycle" (the bonus makes a cycle negative: PHX_S_NEGCYCLE) or "inf" (no path, or no result) —, whether the new annotation calls the
    ORF (1 / 0), and the genes the run's annotation loses and gains."""
    import io

    buf = io.StringIO()
    for nm, cut in _blocks(names, status, offsets):
        buf.write("#id:\t" + nm + "\n#START\tSTOP\tFRAME\tBIAS\tDELTA\tCALLED\tREMOVED\tADDED\n")
        for r in records[cut]:
            buf.write("%d\t%d\t%s\t" % _ends(r) + "%s\t%s\t%d\t%d\t%d\n" % (repr(float(r["bias"])), _delta(r["status"], r["delta"]), int(r["called"]), int(r["n_removed"]), int(r["n_added"])))
    return buf.getvalue()


def format_curated_scan(names, status, offsets, records):
    """--curated-scan FILE OUT: per contig with status >= 0 "#id:\t<name>", for a contig with records "#base:\t<DELTA>\t<unmet>" — the
    baseline under --require / --forbid alone, DELTA as below —, the header, and one row per record of Annotator.curated_scan() (a line of
    FILE, taken on its own under the two sets): format_evidence_scan's columns, REMOVED and ADDED counted against the baseline's genes,
    and UNMET, the required ORFs the new annotation does not call."""
    import io

    buf = io.StringIO()
    for nm, cut in _blocks(names, status, offsets):
        buf.write("#id:\t" + nm + "\n")
        recs = records[cut]
        if len(recs):
            buf.write("#base:\t%s\t%d\n" % (_delta(recs[0]["base_status"], recs[0]["base_delta"]), int(recs[0]["base_unmet"])))
        buf.write("#START\tSTOP\tFRAME\tBIAS\tDELTA\tCALLED\tREMOVED\tADDED\tUNMET\n")
        for r in recs:
            buf.write("%d\t%d\t%s\t" % _ends(r) + "%s\t%s\t%d\t%d\t%d\t%d\n" % (repr(float(r["bias"])), _delta(r["status"], r["delta"]), int(r["called"]), int(r["n_removed"]), int(r["n_added"]),
                                                                              int(r["unmet"])))
    return buf.getvalue()


def format_reannotation(names, status, offsets, genes, delta, unmet=None):
    """--reannotation OUT: per contig with status >= 0 the block write_tabular prints, with "#delta:\t<repr(delta)>" behind its #id line
    and, with --require (unmet given), "#unmet:\t<count>" behind that."""
    import io

    from .writers import write_tabular

    buf = io.StringIO()
    for i, nm in enumerate(names):  # (not _blocks: delta and unmet go by the contig's index)
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
    for nm, cut in _blocks(names, status, offsets):
        buf.write("#id:\t" + nm + "\n#START\tSTOP\tFRAME\tDROP\tRESTART\n")
        for r in records[cut]:
            if r["restart"] >= 0:
                tail = "%d\t%d" % ((int(r["restart_right"]), int(r["restart_left"])) if r["strand"] < 0 else (int(r["restart_left"]), int(r["restart_right"])))
            else:
                tail = "-"
            buf.write("%d\t%d\t%s\t" % _ends(r) + "%s\t%s\n" % (repr(float(r["drop"])), tail))
    return buf.getvalue()


def format_alt_starts(names, status, offsets, records):
    """--alt-starts FILE: per contig with status >= 0 "#id:\t<name>", the header, one row per record of Annotator.alt_starts() (a called
    gene of the device path and another start of its stop, required in its place): the gene's START STOP FRAME as the tabular output
    prints them, the alternative's START, DELTA — repr(delta), or "cycle" (the alternative's edge lies on a cycle: PHX_S_NEGCYCLE),
    "unmet" (the alternative cannot be called) or "inf" (no path) —, and the genes the run's annotation loses and gains."""
    import io

    buf = io.StringIO()
    for nm, cut in _blocks(names, status, offsets):
        buf.write("#id:\t" + nm + "\n#START\tSTOP\tFRAME\tALT\tDELTA\tREMOVED\tADDED\n")
        for r in records[cut]:
            alt = int(r["alt_right"]) if r["strand"] < 0 else int(r["alt_left"])
            buf.write("%d\t%d\t%s\t" % _ends(r) + "%d\t%s\t%d\t%d\n" % (alt, _delta(r["status"], r["delta"], r["unmet"]), int(r["n_removed"]), int(r["n_added"])))
    return buf.getvalue()


def dump_edges(out, ann, i, seq=None, start_codons="atg:0.85,gtg:0.10,ttg:0.05"):
    """-d/--dump (phanotate.py:58,61): one line per edge, repr(src) TAB repr(dst) TAB str(weight*1000), in the reference's
    Graph.iteredges order, the weights as the reference's 28-digit Decimal values (phx_dump_text)."""
    out.write(ann.dump_text(i).decode())


def _format_c(fn, names, status, offsets, *arrays):
    """The text one of libphx's phx_format_* functions prints for a run of contigs, as bytes.  fn(n, names, *arrays, offsets, status,
    &text, &length): `arrays` holds (array, dtype or None) per record array, in the function's order."""
    import ctypes as C

    import numpy as np

    L = _lib.lib()
    n = len(names)
    enc = [x.encode() for x in names]
    arr = (C.c_char_p * max(n, 1))(*enc)
    held = [np.ascontiguousarray(a, dt) for a, dt in arrays] + [np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(status, np.int32)]
    text, tlen = C.c_void_p(), C.c_int64()
    rc = getattr(L, fn)(n, arr, *[x.ctypes.data_as(C.c_void_p) for x in held], C.byref(text), C.byref(tlen))
    if rc:
        raise _lib.PhxError(rc, fn)
    out = C.string_at(text.value, tlen.value)
    L.phx_free_text(text)
    return out


def format_tabular(names, status, offsets, genes):
    """locus.py:39-56 for a run of contigs, as bytes (libphx's phx_format_tabular)."""
    return _format_c("phx_format_tabular", names, status, offsets, (genes, None))


def format_margins(names, status, offsets, records):
    """--margins FILE for a run of contigs, as bytes (libphx's phx_format_margins): per contig with status >= 0 "#id:\t<name>", the
    header, one row per ORF with through == 1 (START STOP FRAME CONTIG SCORE MARGIN CALLED), ordered by left, right, strand."""
    return _format_c("phx_format_margins", names, status, offsets, (records, _lib.MARGIN_DT))


def format_replacements(names, status, offsets, records, genes):
    """--drop-replacements FILE for a run of contigs, as bytes (libphx's phx_format_replacements): per contig with status >= 0
    "#id:\t<name>", the header, one row per called gene of the device path (START STOP FRAME CONTIG DROP REMOVED ADDED), in path order;
    records[k]["gene_off"] indexes genes."""
    return _format_c("phx_format_replacements", names, status, offsets, (records, _lib.REPL_DT), (genes, _lib.GENE_DT))


def format_drops(names, status, offsets, records):
    """--drop-margins FILE for a run of contigs, as bytes (libphx's phx_format_drops): per contig with status >= 0 "#id:\t<name>", the
    header, one row per called gene of the device path (START STOP FRAME CONTIG SCORE DROP CALLED), in path order."""
    return _format_c("phx_format_drops", names, status, offsets, (records, _lib.DROP_DT))


def _merge(parts):
    """(status, offsets, *arrays) of a run of batches from the same of every batch, in order: the statuses concatenated, the offsets
    rebuilt from every batch's counts, each further array concatenated."""
    import numpy as np

    counts = np.concatenate([np.diff(p[1]) for p in parts])
    return (np.concatenate([p[0] for p in parts]), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)) + tuple(np.concatenate(a) for a in list(zip(*parts))[2:])


def _merge_replacements(parts):
    """_merge for Annotator.replacements(): each batch's gene_off counts from its own genes.  (Further arrays, pinreplacements()' lost, as _merge has them.)"""
    shifted, g0 = [], 0
    for status, offsets, records, genes, *more in parts:
        records = records.copy()
        records["gene_off"] += g0
        g0 += len(genes)
        shifted.append((status, offsets, records, genes, *more))
    return _merge(shifted)


class _Entries:
    """The lines of the entry files that name contigs of the batch resident on `ann`, as ORF indices: entries(dest) is what the resolver
    of INPUTS[dest] makes of them ([None] per contig for a file not given), worked out when a fetch first asks for it and kept for the
    batch — Annotator.orf_index is pure, so the re-annotation and the curated scan share one walk over --forbid and --require."""

    def __init__(self, ann, names, lines):
        self.ann, self.names, self.here, self.lines, self.done = ann, names, set(names), lines, {}

    def __call__(self, dest):
        if dest not in self.done:
            mine = [e for e in self.lines.get(dest, ()) if e[3] in self.here]
            self.done[dest] = INPUTS[dest].resolve(mine, self.names, self.ann.orf_index, INPUTS[dest].flag)
        return self.done[dest]


def _reannotate(ann, entries):
    """The batch's second annotation, for --reannotation: under --evidence, or --require, or --forbid alone."""
    refused = entries("forbid")
    if "evidence" in entries.lines:
        return ann.evidence(entries("evidence"), refused)
    if "require" in entries.lines:
        return ann.constrain(refused, entries("require"))
    return ann.reannotate(refused)


def _path(args, dest, half):
    """The path a flag names: its value, or for a flag of two values (FILE OUT) that half of it."""
    value = getattr(args, dest)
    return value if isinstance(value, str) else value[half]


_In = collections.namedtuple("_In", "flag dest parse resolve")
_Out = collections.namedtuple("_Out", "flag dest fmt mode fetch resident piped merge")


def _dest(flag):  # as argparse names it
    return flag[2:].replace("-", "_")


def _out(flag, fmt, mode, fetch, resident=False, piped=None, merge=_merge):
    return _Out(flag, _dest(flag), fmt, mode, fetch, resident, piped, merge)


# The entry files, in the order main opens and parses them: the flag as the messages name it (for the two scans the FILE half of the
# flag's value), the parser of its lines and the resolver of its lines to ORF indices.  Each works on the batch resident on one context.
INPUTS = {_dest(flag): _In(flag, _dest(flag), parse, resolve) for flag, parse, resolve in (
    ("--curated-scan", parse_evidence, resolve_evidence),
    ("--evidence-scan", parse_evidence, resolve_evidence),
    ("--evidence", parse_evidence, resolve_evidence),
    ("--forbid", parse_forbid, resolve_forbid),
    ("--require", parse_forbid, resolve_forbid),
)}
# The side outputs, in the order main writes their files (for the two scans to the OUT half of the flag's value).  fmt(names, *merge(what
# fetch(ann, entries) returned per batch)) is the file's content and mode how it is opened; resident: it works on the batch resident on one
# context, so no --gpus above 1 and the batches one after the other; piped: the keyword under which Pipeline.run collects it (None: it
# cannot) — the rows with one stand in the order of the members an item of Pipeline.run gains.
OUTPUTS = {o.dest: o for o in (
    _out("--margins", format_margins, "wb", lambda ann, entries: ann.margins(), piped="margins"),
    _out("--remargins", format_margins, "wb", lambda ann, entries: ann.remargins(), resident=True),
    _out("--redrop-margins", format_drops, "wb", lambda ann, entries: ann.redrops(), resident=True),
    _out("--redrop-replacements", format_replacements, "wb", lambda ann, entries: ann.rereplacements(), resident=True, merge=_merge_replacements),
    _out("--pin-margins", format_pin_margins, "wb", lambda ann, entries: ann.pinmargins(), resident=True),
    _out("--pin-drop-margins", format_pin_drops, "wb", lambda ann, entries: ann.pindrops(), resident=True),
    _out("--pin-drop-replacements", format_pin_replacements, "wb", lambda ann, entries: ann.pinreplacements(), resident=True, merge=_merge_replacements),
    _out("--drop-margins", format_drops, "wb", lambda ann, entries: ann.drop_margins(), piped="drop_margins"),
    _out("--drop-replacements", format_replacements, "wb", lambda ann, entries: ann.replacements(), piped="replacements", merge=_merge_replacements),
    _out("--start-drops", format_start_drops, "w", lambda ann, entries: ann.start_drops()[:3], resident=True),
    _out("--alt-starts", format_alt_starts, "w", lambda ann, entries: ann.alt_starts()[:3], resident=True),
    _out("--evidence-scan", format_evidence_scan, "w", lambda ann, entries: ann.evidence_scan(entries("evidence_scan"))[:3], resident=True),
    _out("--curated-scan", format_curated_scan, "w", lambda ann, entries: ann.curated_scan(entries("curated_scan"), entries("forbid"), entries("require"))[:3], resident=True),
    _out("--profile", format_profile, "wb", lambda ann, entries: ann.profile(), resident=True),  # (it needs nothing else and conflicts with nothing: no row in _RULES)
    _out("--reannotation", format_reannotation, "w", _reannotate),  # (format_reannotation's unmet: the fifth member constrain() returns, so only with --require)
)}
# A batch's fetches, in this order.  THE ORDER IS CONTRACT: the replacements in front of the drop margins (the drops are then computed
# once); the curated scan behind the batch's re-annotation, which thereby stays the cached one; remargins, the re-annotation's drop
# margins, its replacements (behind its drop margins: an existing order; the trees are then built once more), pinmargins
# and the pinned drop margins (behind pinmargins, which they build on) behind the re-annotation, whose margins they are, the pinned
# replacements behind the pinned drop margins (as the re-annotation's: the trees are then built once more).  The entry files are resolved where a fetch first needs them, so a line that names no ORF is
# reported in the order --evidence-scan, --forbid, --evidence or --require, --curated-scan.
_FETCH_ORDER = ("margins", "drop_replacements", "drop_margins", "start_drops", "alt_starts", "evidence_scan", "reannotation", "curated_scan", "remargins", "redrop_margins", "redrop_replacements", "pin_margins", "pin_drop_margins", "pin_drop_replacements", "profile")
# The entry files in the order main looks for a line that names a contig the FASTA file does not hold.
_UNKNOWN_ORDER = ("forbid", "require", "evidence", "evidence_scan", "curated_scan")
assert set(_CHECK_ORDER) == set(OUTPUTS) | set(INPUTS) and set(_FETCH_ORDER) == set(OUTPUTS) and set(_UNKNOWN_ORDER) == set(INPUTS)  # a new row takes its place in each order


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
    outputs = [o for o in OUTPUTS.values() if getattr(args, o.dest) is not None]
    parts = {o.dest: [] for o in outputs}  # per side output what its fetch returned for every batch, in order
    lines = {}  # per entry file given: its parsed lines
    try:
        for i in INPUTS.values():
            if getattr(args, i.dest) is not None:
                with open(_path(args, i.dest, 0)) as fh:
                    lines[i.dest] = i.parse(fh, i.flag)
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
        if lines or any(o.resident for o in outputs) or (len(cuts) == 1 and n_gpu == 1):  # the batches one after the other, each resident on the caller's context
            flat, fetches = [], sorted(outputs, key=lambda o: _FETCH_ORDER.index(o.dest))
            for lo, hi in cuts:
                t0 = time.perf_counter()
                ann.upload_raw(fa.ptrs[idx[lo:hi]], fa.lens[idx[lo:hi]], fa)
                ann.set_trnas(trnas_of(idx[lo:hi]))
                t1 = time.perf_counter()
                ann.run()
                t2 = time.perf_counter()
                flat.append(ann.download_flat())
                t3 = time.perf_counter()
                # (without an entry file no work per contig here: the plain run is the one the benchmark times)
                entries = _Entries(ann, [fa.names[int(i)] for i in idx[lo:hi]], lines) if lines else None
                for o in fetches:
                    parts[o.dest].append(o.fetch(ann, entries))
                t_parts["upload_s"] += t1 - t0; t_parts["run_s"] += t2 - t1; t_parts["download_s"] += t3 - t2
        else:  # a stream of batches: two in flight per GPU, the batches round the GPUs (pipeline.Pipeline)
            from .pipeline import Pipeline

            t0 = time.perf_counter()
            pipe = Pipeline(ann.params, device=device, depth=2, devices=([device] + [d for d in range(n_gpu) if d != device][: n_gpu - 1]) if n_gpu > 1 else None, first=ann)
            t1 = time.perf_counter()
            gen = ((fa.ptrs[idx[lo:hi]], fa.lens[idx[lo:hi]], fa, (lambda a=lo, b=hi: trnas_of(idx[a:b]))) for lo, hi in cuts)
            try:
                flat = list(pipe.run(gen, **{o.piped: o.dest in parts for o in OUTPUTS.values() if o.piped}))
                t2 = time.perf_counter()
                for k, o in enumerate(outputs, 3):  # (all of them Pipeline.run's on this path, and OUTPUTS lists those in the order of an item's members)
                    parts[o.dest].extend(p[k] for p in flat)
                flat = [p[:3] for p in flat]
            finally:
                pipe.close()
            t_parts["contexts_s"] = t1 - t0; t_parts["pipeline_s"] = t2 - t1; t_parts["gpus"] = n_gpu
        return flat[0] if len(flat) == 1 else _merge(flat)

    known = set(fa.names)
    for dest in _UNKNOWN_ORDER:
        for e in lines.get(dest, ()):
            if e[3] not in known:
                drop_context()
                sys.stderr.write("Error: %s: no such ORF in its contig: %r\n" % (INPUTS[dest].flag, e[4]))
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
        for o in outputs:
            with open(_path(args, o.dest, 1), o.mode) as fh:
                fh.write(o.fmt(fa.names, *o.merge(parts[o.dest])))
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
