"""Masked re-annotation, the parts that need no GPU: the --forbid parser and its resolution to ORF indices, the
--reannotation writer, the CLI's refusals, and the C-ABI's declarations.  (The masked solver is the window schedule of k_sssp_lds with
refused edges left out of a window's tile, no schedule of its own: the GPU tests check it against the in-place Bellman-Ford.)"""
import ctypes as C
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from phanotate_amd import _lib
from phanotate_amd.cli import ForbidError, format_reannotation, parse_forbid, resolve_forbid
from phanotate_amd.writers import write_tabular


def some_genes():
    g = np.zeros(4, _lib.GENE_DT)
    g["left"], g["right"], g["strand"], g["frame"], g["score"] = [100, 700, 1500, 2000], [402, 1002, 1602, 2300], [1, -1, 1, -1], [1, -2, 4, -3], [-4.8, -1.25e-3, -20.0, -7.0]
    return g


def test_round_trip_from_write_tabular_lines():
    genes = some_genes()
    buf = io.StringIO()
    write_tabular(buf, "ctg one", genes)
    lines = buf.getvalue().splitlines(keepends=True)
    assert lines[0].startswith("#id:") and lines[1].startswith("#START")
    got = parse_forbid(lines)  # the whole block as a user would paste it: '#' lines are skipped, the SCORE column is ignored
    cds = [g for g in genes if abs(int(g["frame"])) <= 3]
    assert [(a, z, s, c) for a, z, s, c, _ in got] == [(int(g["left"]), int(g["right"]), int(g["strand"]), "ctg one") for g in cds]
    assert [x[4] for x in got] == [ln.rstrip("\n") for ln in lines[2:]]
    # reverse-strand rows are printed STOP < START swapped: left / right come back in order
    assert got[1][:3] == (700, 1002, -1) and lines[3].split("\t")[:2] == ["1002", "700"]


def test_extra_columns_comments_blank_lines_and_spaces():
    text = ["# a comment\n", "\n", "100\t402\t+\tc1\t-4.8E+00\tanything\telse\n", "  # indented comment\n", "1002 700 - c2\r\n", "5\t9\t+\tc1"]
    got = parse_forbid(text)
    assert [x[:4] for x in got] == [(100, 402, 1, "c1"), (700, 1002, -1, "c2"), (5, 9, 1, "c1")]
    assert got[1][4] == "1002 700 - c2"


@pytest.mark.parametrize("line", ["100\t402\t+", "a\tb\t+\tc1", "100\t402\t*\tc1", "100\t402\t1\tc1"])
def test_malformed_lines_are_quoted(line):
    with pytest.raises(ForbidError) as e:
        parse_forbid([line + "\n"])
    assert repr(line) in str(e.value)


def test_resolution_and_an_unknown_orf():
    table = {(0, 100, 402, 1): 7, (1, 700, 1002, -1): 3, (0, 5, 9, 1): 0}

    def lookup(i, left, right, strand):
        return table[(i, left, right, strand)]

    entries = parse_forbid(["100\t402\t+\tc1\n", "1002\t700\t-\tc2\n", "5\t9\t+\tc1\n"])
    assert resolve_forbid(entries, ["c1", "c2", "c3"], lookup) == [[7, 0], [3], None]
    for bad in ("100\t403\t+\tc1", "100\t402\t-\tc1", "100\t402\t+\tc2", "100\t402\t+\tnobody"):
        with pytest.raises(ForbidError) as e:
            resolve_forbid(parse_forbid([bad + "\n"]), ["c1", "c2", "c3"], lookup)
        assert repr(bad) in str(e.value)


def test_reannotation_writer():
    genes = some_genes()
    status = np.array([0, -2, 1], np.int32)
    offsets = np.array([0, 4, 4, 4], np.int64)
    delta = np.array([0.125, np.inf, np.inf])
    text = format_reannotation(["a", "bad", "c"], status, offsets, genes, delta)
    one = io.StringIO()
    write_tabular(one, "a", genes)
    head, rest = one.getvalue().split("\n", 1)
    assert text == head + "\n#delta:\t0.125\n" + rest + "#id:\tc\n#delta:\tinf\n#START\tSTOP\tFRAME\tCONTIG\tSCORE\n"
    assert float(re.search(r"#delta:\t(\S+)", text).group(1)) == 0.125


def test_cli_refuses_the_flags_alone_with_dump_and_under_a_multi_rank_launch(tmp_path):
    fa = tmp_path / "x.fasta"
    fa.write_text(">x\nacgtacgtacgt\n")
    fb = tmp_path / "f.txt"
    fb.write_text("1\t9\t+\tx\n")
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fa)]
    both = ["--forbid", str(fb), "--reannotation", str(tmp_path / "o.txt")]
    for extra, env, word in ((both[:2], {}, "each needs the other"), (both[2:], {}, "each needs the other"), (both + ["-d"], {}, "-d/--dump"),
                             (both, {"WORLD_SIZE": "2", "RANK": "0"}, "multi-rank"), (both + ["--gpus", "2"], {}, "--gpus above 1")):
        r = subprocess.run(exe + extra, capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)


def test_declared_exported_and_refused_without_a_context():
    header = open(os.path.join(ROOT, "include", "phx.h")).read()
    for name in ("phx_reannotate_flat", "phx_orf_offsets", "phx_tap_repath", "phx_reannotate_ms"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.EXPORTS
    L = _lib.lib()
    n = C.c_int32()
    ms = (C.c_float * 3)()
    assert L.phx_reannotate_flat(None, None, None, 0, None, 0, None, None, None, None) == -1
    assert L.phx_tap_repath(None, 0, None, 0, C.byref(n), None, 0) == -1
    assert L.phx_reannotate_ms(None, ms) == -1
    assert L.phx_orf_offsets(None, None) == -1
