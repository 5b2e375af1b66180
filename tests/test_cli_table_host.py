"""The command line's tables, pinned from outside (no GPU): which refusal get_args reports for a command line, as literal
messages, and which Annotator / Pipeline calls main makes for a batch, in which order, as literal lists, with a recording stand-in for
both classes.  Neither test reads the tables of phanotate_amd/cli.py: both passed unchanged on the cli.py from before the tables."""
import os

import numpy as np
import pytest

from phanotate_amd import _lib, cli

DUMP, RANKS, GPUS = ": not allowed with argument -d/--dump", ": not available under a multi-rank launch", ": not available with --gpus above 1"
# (argv behind the FASTA file — F: an entry or output file, O: an output file —, WORLD_SIZE, "ok" or the last line of stderr behind "error: ")
ARG_CASES = [
    # -d/--dump, per flag
    ("--margins F -d", 1, "argument --margins" + DUMP),
    ("--drop-margins F -d", 1, "argument --drop-margins" + DUMP),
    ("--drop-replacements F -d", 1, "argument --drop-replacements" + DUMP),
    ("--start-drops F -d", 1, "argument --start-drops" + DUMP),
    ("--alt-starts F -d", 1, "argument --alt-starts" + DUMP),
    ("--evidence-scan F O -d", 1, "argument --evidence-scan" + DUMP),
    ("--curated-scan F O -d", 1, "argument --curated-scan" + DUMP),
    ("--remargins F -d", 1, "argument --remargins" + DUMP),
    ("--pin-margins F -d", 1, "argument --pin-margins" + DUMP),
    ("--forbid F -d", 1, "argument --forbid" + DUMP),
    ("--require F -d", 1, "argument --require" + DUMP),
    ("--evidence F -d", 1, "argument --evidence" + DUMP),
    ("--reannotation O -d", 1, "argument --reannotation" + DUMP),
    # a multi-rank launch, per flag
    ("--margins F", 2, "argument --margins" + RANKS),
    ("--drop-margins F", 2, "argument --drop-margins" + RANKS),
    ("--drop-replacements F", 2, "argument --drop-replacements" + RANKS),
    ("--start-drops F", 2, "argument --start-drops" + RANKS),
    ("--alt-starts F", 2, "argument --alt-starts" + RANKS),
    ("--evidence-scan F O", 2, "argument --evidence-scan" + RANKS),
    ("--curated-scan F O", 2, "argument --curated-scan" + RANKS),
    ("--remargins F", 2, "argument --remargins" + RANKS),
    ("--pin-margins F", 2, "argument --pin-margins" + RANKS),
    ("--forbid F", 2, "argument --forbid" + RANKS),
    ("--require F", 2, "argument --require" + RANKS),
    ("--evidence F", 2, "argument --evidence" + RANKS),
    ("--reannotation O", 2, "argument --reannotation" + RANKS),
    # --gpus above 1, per flag that works on a resident batch
    ("--start-drops F --gpus 2", 1, "argument --start-drops" + GPUS),
    ("--alt-starts F --gpus 2", 1, "argument --alt-starts" + GPUS),
    ("--evidence-scan F O --gpus 2", 1, "argument --evidence-scan" + GPUS),
    ("--curated-scan F O --gpus 2", 1, "argument --curated-scan" + GPUS),  # (in front of "needs --require")
    ("--remargins F --gpus 2", 1, "argument --remargins" + GPUS),
    ("--pin-margins F --gpus 2", 1, "argument --pin-margins" + GPUS),
    ("--evidence F --reannotation O --gpus 2", 1, "argument --evidence" + GPUS),
    ("--forbid F --reannotation O --gpus 2", 1, "argument --forbid" + GPUS),
    ("--require F --reannotation O --gpus 2", 1, "argument --require" + GPUS),
    # the relations between flags
    ("--curated-scan F O", 1, "argument --curated-scan: needs --require"),
    ("--remargins F --require F --reannotation O", 1, "argument --remargins: not allowed with argument --require"),
    ("--remargins F --forbid F", 1, "argument --remargins: needs --reannotation"),
    ("--pin-margins F", 1, "argument --pin-margins: needs --require"),
    ("--pin-margins F --require F", 1, "argument --pin-margins: needs --reannotation"),
    ("--evidence F --require F --reannotation O", 1, "argument --evidence: not allowed with argument --require"),
    ("--evidence F", 1, "argument --evidence: needs --reannotation"),
    ("--forbid F", 1, "arguments --forbid and --reannotation: each needs the other"),
    ("--reannotation O", 1, "arguments --forbid and --reannotation: each needs the other"),
    ("--require F", 1, "argument --require: needs --reannotation"),
    # accepted
    ("", 1, "ok"),
    ("", 2, "ok"),
    ("-d", 1, "ok"),
    ("--margins F --drop-margins F --drop-replacements F --gpus 2", 1, "ok"),
    ("--forbid F --reannotation O --remargins F --evidence F --evidence-scan F O --start-drops F --alt-starts F", 1, "ok"),
    ("--require F --forbid F --reannotation O --pin-margins F --curated-scan F O", 1, "ok"),
    # which refusal comes first when several apply
    ("--evidence F --remargins F", 1, "argument --remargins: needs --reannotation"),
    ("--require F --curated-scan F O", 1, "argument --require: needs --reannotation"),
    ("--require F --reannotation O --pin-margins F --remargins F", 1, "argument --remargins: not allowed with argument --require"),
    ("--require F --reannotation O --pin-margins F --evidence F", 1, "argument --evidence: not allowed with argument --require"),
    ("--start-drops F -d --gpus 2", 2, "argument --start-drops" + DUMP),  # dump, multi-rank and gpus on one flag
    ("--start-drops F --gpus 2", 2, "argument --start-drops" + RANKS),
    ("--reannotation O --forbid F --start-drops F --margins F -d", 1, "argument --margins" + DUMP),  # the flags' own order, not the command line's
    ("--evidence F --forbid F -d", 1, "argument --forbid" + DUMP),
    ("--evidence F --gpus 2", 1, "argument --evidence: needs --reannotation"),
    ("--evidence F --forbid F --reannotation O --gpus 2", 1, "argument --evidence" + GPUS),
    ("--forbid F --require F --gpus 2", 1, "argument --require: needs --reannotation"),
    ("--pin-margins F --curated-scan F O", 1, "argument --curated-scan: needs --require"),
]


@pytest.mark.parametrize("tail,world,want", ARG_CASES, ids=["%s|%d" % (t or "-", w) for t, w, _ in ARG_CASES])
def test_get_args_reports_this_refusal(tail, world, want, tmp_path, monkeypatch, capsys):
    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    given = tmp_path / "f.txt"
    given.write_text("1\t9\t+\tc1\t-1.0\n")
    argv = [str(fasta)] + [{"F": str(given), "O": str(tmp_path / "o.txt")}.get(word, word) for word in tail.split()]
    monkeypatch.setenv("WORLD_SIZE", str(world))
    try:
        cli.get_args(argv)
        got = "ok"
    except SystemExit as e:
        assert e.code == 2
        got = capsys.readouterr().err.strip().splitlines()[-1].split("error: ", 1)[1]
    assert got == want


def test_the_cases_cover_every_message():
    assert len({want for _, _, want in ARG_CASES}) == 45  # 13 flags x (dump, multi-rank), 9 x gpus, 9 relations, "ok"


# ---- the calls of a batch ----
class Recorder:
    """Stand-ins for cli.Annotator and pipeline.Pipeline that note their calls in one list and hand back one gene and one record per
    contig: contig j of the input (counted over the batches) has the gene 100 j + 1 .. 100 j + 90."""

    def __init__(self, no_orfs=False):
        self.calls, self.seen = [], 0
        rec = self

        def batch(n, dt):
            a = np.zeros(n, dt)
            a["left"] = 100 * (rec.seen - n + np.arange(n)) + 1
            a["right"] = a["left"] + 89
            a["strand"] = 1
            return a

        def flat(n, dt, *more):
            return (np.zeros(n, np.int32), np.arange(n + 1, dtype=np.int64), batch(n, dt)) + more

        def margin_records(n):
            a = batch(n, _lib.MARGIN_DT)
            a["through"] = 1
            return a

        def replacement(n):
            a = batch(n, _lib.REPL_DT)
            a["n_removed"] = 1
            a["gene_off"] = np.arange(n)
            return flat(n, _lib.GENE_DT)[:2] + (a, batch(n, _lib.GENE_DT))

        class Annotator:
            def __init__(self, params=None, device=0, **kw):
                self.params, self.n = params, 0

            def note(self, name):
                rec.calls.append(name)

            def upload_raw(self, ptrs, lens, keep=None):
                self.note("upload_raw")
                self.n = len(lens)
                rec.seen += self.n

            def set_trnas(self, trnas):
                self.note("set_trnas")

            def run(self):
                self.note("run")

            def download_flat(self):
                self.note("download_flat")
                return flat(self.n, _lib.GENE_DT)

            def margins(self):
                self.note("margins")
                return flat(self.n, _lib.MARGIN_DT)[:2] + (margin_records(self.n),)

            def remargins(self):
                self.note("remargins")
                return flat(self.n, _lib.MARGIN_DT)[:2] + (margin_records(self.n),)

            def pinmargins(self):
                self.note("pinmargins")
                return flat(self.n, _lib.MARGIN_DT)[:2] + (margin_records(self.n), np.zeros(self.n, np.int32))

            def drop_margins(self):
                self.note("drop_margins")
                return flat(self.n, _lib.DROP_DT)

            def replacements(self):
                self.note("replacements")
                return replacement(self.n)

            def start_drops(self):
                self.note("start_drops")
                return flat(self.n, _lib.START_DT, None)

            def alt_starts(self):
                self.note("alt_starts")
                return flat(self.n, _lib.ALT_DT, None)

            def evidence_scan(self, hits):
                self.note("evidence_scan")
                return flat(self.n, _lib.EVSCAN_DT, None)

            def curated_scan(self, hits, forbid=None, require=None):
                self.note("curated_scan")
                return flat(self.n, _lib.CUSCAN_DT, None)

            def orf_index(self, i, left, right, strand):  # (not noted: how often a file's lines are resolved is not part of the order)
                if no_orfs:
                    raise KeyError("contig %d has no such ORF" % i)
                return 0

            def reannotate(self, forbid):
                self.note("reannotate")
                return flat(self.n, _lib.GENE_DT, np.zeros(self.n))

            def evidence(self, bias, forbid=None):
                self.note("evidence")
                return flat(self.n, _lib.GENE_DT, np.zeros(self.n))

            def constrain(self, forbid=None, require=None):
                self.note("constrain")
                return flat(self.n, _lib.GENE_DT, np.zeros(self.n), np.zeros(self.n, np.int32))

            def close(self):
                self.note("close")

        class Pipeline:
            def __init__(self, params=None, device=0, depth=2, devices=None, first=None):
                pass

            def run(self, batches, margins=False, drop_margins=False, replacements=False):
                rec.calls.append(("Pipeline.run", margins, drop_margins, replacements))
                for b in batches:
                    n = len(b[1])
                    rec.seen += n
                    item = flat(n, _lib.GENE_DT)
                    if margins:
                        item += (flat(n, _lib.MARGIN_DT)[:2] + (margin_records(n),),)
                    if drop_margins:
                        item += (flat(n, _lib.DROP_DT),)
                    if replacements:
                        item += (replacement(n),)
                    yield item

            def close(self):
                rec.calls.append("Pipeline.close")

        self.Annotator, self.Pipeline = Annotator, Pipeline


BATCH = ["upload_raw", "set_trnas", "run", "download_flat"]


@pytest.fixture
def run_cli(tmp_path, monkeypatch):
    """run(argv behind the FASTA file, as in ARG_CASES with FORBID, REQUIRE and BIASES for the entry files; two_batches: --batch-bases
    below two contigs; no_orfs: Annotator.orf_index finds nothing) -> (exit code, the calls, {flag: path of its output})."""
    import phanotate_amd.pipeline

    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PHX_CLI_TIMING"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr("shutil.which", lambda *a, **k: None)  # no tRNA finder: the batches get no hits
    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\n" + "acgt" * 30 + "\n>c2\n" + "ttga" * 30 + "\n")
    words = {"FORBID": "1\t90\t+\tc1\n", "REQUIRE": "101\t190\t+\tc2\n", "BIASES": "1\t90\t+\tc1\t-1.0\n101\t190\t+\tc2\t2.5\n"}
    for word, text in words.items():
        (tmp_path / word).write_text(text)

    def run(tail, two_batches=False, no_orfs=False):
        rec = Recorder(no_orfs)
        monkeypatch.setattr(cli, "Annotator", rec.Annotator)
        monkeypatch.setattr(phanotate_amd.pipeline, "Pipeline", rec.Pipeline)  # (main imports the class from there when it streams)
        argv, outs, prev = [str(fasta), "-o", str(tmp_path / "out.tsv")], {}, None
        for word in tail.split():
            if word in words:
                argv.append(str(tmp_path / word))
            elif word in ("F", "O"):
                outs[prev] = str(tmp_path / (prev.strip("-") + ".out"))
                argv.append(outs[prev])
            else:
                argv.append(word)
                prev = word
        rc = cli.main(argv + (["--batch-bases", "150"] if two_batches else []))
        return rc, rec.calls, outs

    return run


def test_plain_run_is_four_calls(run_cli):
    rc, calls, _ = run_cli("")
    assert rc == 0 and calls == BATCH


def test_one_batch_fetches_the_three_siblings_on_its_context(run_cli):
    rc, calls, outs = run_cli("--margins F --drop-margins F --drop-replacements F")
    assert rc == 0 and calls == BATCH + ["margins", "replacements", "drop_margins"]
    for path in outs.values():
        text = open(path).read()
        assert "#id:\tc1\n" in text and "#id:\tc2\n" in text


def expected_replacements(shift):
    rec, genes = np.zeros(2, _lib.REPL_DT), np.zeros(2, _lib.GENE_DT)
    for a in (rec, genes):
        a["left"], a["right"], a["strand"] = [1, 101], [90, 190], 1
    rec["n_removed"], rec["gene_off"] = 1, [0, shift]
    return cli.format_replacements(["c1", "c2"], np.zeros(2, np.int32), np.array([0, 1, 2], np.int64), rec, genes)


def test_two_batches_stream_through_the_pipeline(run_cli):
    rc, calls, outs = run_cli("--margins F --drop-margins F --drop-replacements F", two_batches=True)
    assert rc == 0 and calls == [("Pipeline.run", True, True, True), "Pipeline.close"]
    assert open(outs["--drop-replacements"], "rb").read() == expected_replacements(1)
    assert open(outs["--drop-margins"], "rb").read().count(b"#id:") == 2 and b"DROP" in open(outs["--drop-margins"], "rb").read()
    # an item's members are taken by what was asked for: the replacements come third here, fourth above
    rc, calls, outs = run_cli("--drop-replacements F --margins F", two_batches=True)
    assert rc == 0 and calls == [("Pipeline.run", True, False, True), "Pipeline.close"]
    assert open(outs["--drop-replacements"], "rb").read() == expected_replacements(1)
    assert b"MARGIN" in open(outs["--margins"], "rb").read()


def test_every_resident_output_in_the_order_of_a_batch(run_cli):
    rc, calls, outs = run_cli("--require REQUIRE --forbid FORBID --reannotation O --pin-margins F --curated-scan BIASES O --margins F --drop-replacements F --drop-margins F "
                              "--start-drops F --alt-starts F --evidence-scan BIASES O", two_batches=True)
    assert rc == 0
    assert calls == 2 * (BATCH + ["margins", "replacements", "drop_margins", "start_drops", "alt_starts", "evidence_scan", "constrain", "curated_scan", "pinmargins"])
    # the second batch's record points at the second batch's gene: gene_off shifted by the genes of the batch before
    got = open(outs["--drop-replacements"], "rb").read()
    assert got == expected_replacements(1) and got != expected_replacements(0)
    assert sorted(outs) == sorted(["--reannotation", "--pin-margins", "--curated-scan", "--margins", "--drop-replacements", "--drop-margins", "--start-drops", "--alt-starts",
                                   "--evidence-scan"])
    for flag, path in outs.items():
        assert open(path).read().count("#id:\tc") == 2, flag
    assert open(outs["--reannotation"]).read().count("#unmet:\t0\n") == 2  # --require: the #unmet: line


def test_evidence_with_forbid_and_remargins(run_cli):
    rc, calls, outs = run_cli("--evidence BIASES --forbid FORBID --reannotation O --remargins F")
    assert rc == 0 and calls == BATCH + ["evidence", "remargins"]
    text = open(outs["--reannotation"]).read()
    assert text.count("#delta:\t0.0\n") == 2 and "#unmet:" not in text


def test_a_line_without_an_orf_closes_the_context(run_cli, capsys):
    rc, calls, outs = run_cli("--forbid FORBID --reannotation O --margins F", no_orfs=True)
    assert rc == 2 and calls == BATCH + ["margins", "close"]
    assert capsys.readouterr().err.strip().splitlines()[-1] == "Error: --forbid: no such ORF in its contig: '1\\t90\\t+\\tc1'"
    assert not os.path.exists(outs["--margins"])
