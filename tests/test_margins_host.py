"""Host side of the per-ORF path margins (no GPU): the C formatter of --margins FILE against a plain Python rendering of its format,
the CLI's refusal of --margins with --dump, and the new entry points in the header and the export list."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def lib():
    from phanotate_amd import _lib

    return _lib


def py_format(names, status, offsets, rec):
    """The format DESIGN.md §11 states, in plain Python: a block per contig with status >= 0, rows with through == 1 ordered by left,
    right, strand; START > STOP on the reverse strand; SCORE and MARGIN '%E'."""
    out = []
    for i, nm in enumerate(names):
        if status[i] < 0:
            continue
        out.append("#id:\t%s\n" % nm)
        out.append("#START\tSTOP\tFRAME\tCONTIG\tSCORE\tMARGIN\tCALLED\n")
        rows = [r for r in rec[offsets[i]:offsets[i + 1]] if r["through"]]
        rows.sort(key=lambda r: (int(r["left"]), int(r["right"]), int(r["strand"])))
        for r in rows:
            a, z = (int(r["right"]), int(r["left"])) if r["strand"] < 0 else (int(r["left"]), int(r["right"]))
            out.append("%d\t%d\t%s\t%s\t%s\t%s\t%d\n" % (a, z, "+" if r["strand"] > 0 else "-", nm, "%E" % float(r["score"]), "%E" % float(r["margin"]), int(r["called"])))
    return "".join(out).encode()


def c_format(lib, names, status, offsets, rec):
    L = lib.lib()
    arr = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    status = np.ascontiguousarray(status, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    rec = np.ascontiguousarray(rec, lib.MARGIN_DT)
    text, tlen = C.c_void_p(), C.c_int64()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = L.phx_format_margins(len(names), arr, vp(rec), vp(offsets), vp(status), C.byref(text), C.byref(tlen))
    assert rc == 0
    out = C.string_at(text.value, tlen.value)
    L.phx_free_text(text)
    return out


def random_records(lib, rng, n_contig, per, names_len=8):
    counts = [0 if k % 7 == 3 else int(rng.randint(0, per)) for k in range(n_contig)]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rec = np.zeros(int(offsets[-1]), lib.MARGIN_DT)
    t = len(rec)
    left = rng.randint(1, 200000, t)
    rec["left"] = left
    rec["right"] = left + 3 * rng.randint(30, 2000, t) + 2
    rec["strand"] = rng.choice([-1, 1], t)
    rec["frame"] = rec["strand"] * rng.randint(1, 4, t)
    rec["score"] = -np.exp(rng.uniform(-5, 40, t))
    rec["margin"] = np.where(rng.rand(t) < 0.2, 0.0, np.round(np.exp(rng.uniform(-7, 25, t)) * 1000) / 1000.0)
    rec["called"] = (rng.rand(t) < 0.05).astype(np.int32)
    rec["through"] = (rng.rand(t) < 0.8).astype(np.int32)
    rec["margin"][rec["through"] == 0] = np.inf
    # ties on left (two starts of one stop on the reverse strand share the left end), and one pair equal on left and right
    if t > 10:
        rec["left"][5] = rec["left"][4]
        rec["left"][7], rec["right"][7] = rec["left"][6], rec["right"][6]
        rec["strand"][7] = -rec["strand"][6]
    status = np.zeros(n_contig, np.int32)
    status[1::9] = -2  # error contigs: skipped
    status[2::11] = 1  # no path: a block (its records have through == 0 here anyway)
    names = ["ctg_%0*d" % (names_len, k) for k in range(n_contig)]
    return names, status, offsets, rec


def test_format_margins_matches_python_rendering(lib):
    rng = np.random.RandomState(5)
    names, status, offsets, rec = random_records(lib, rng, 12, 40)
    assert status[1] < 0 and offsets[4] == offsets[3]  # a skipped error contig and an empty one
    assert (rec["strand"] < 0).any() and (~np.isfinite(rec["margin"])).any()
    assert c_format(lib, names, status, offsets, rec) == py_format(names, status, offsets, rec)


def test_format_margins_many_threads_same_text(lib, monkeypatch):
    """Beyond 1 MB of text the formatter splits the contigs over worker threads: the text must not depend on their number."""
    rng = np.random.RandomState(6)
    names, status, offsets, rec = random_records(lib, rng, 300, 400)
    want = py_format(names, status, offsets, rec)
    assert len(want) > (1 << 20)
    assert c_format(lib, names, status, offsets, rec) == want
    monkeypatch.setenv("PHX_HOST_THREADS", "3")
    assert c_format(lib, names, status, offsets, rec) == want


def test_format_margins_no_contigs_and_bad_args(lib):
    assert c_format(lib, [], np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, lib.MARGIN_DT)) == b""
    L = lib.lib()
    text, tlen = C.c_void_p(), C.c_int64()
    assert L.phx_format_margins(-1, None, None, None, None, C.byref(text), C.byref(tlen)) == -1


def test_margins_with_dump_is_refused(tmp_path):
    fa = os.path.join(ROOT, "tests", "golden", "phiX174.fasta.gz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), fa, "--dump", "--margins", str(tmp_path / "m.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--margins" in r.stderr and "--dump" in r.stderr
    assert not (tmp_path / "m.tsv").exists()


def test_margins_under_a_multi_rank_launch_is_refused(tmp_path):
    fa = os.path.join(ROOT, "tests", "golden", "phiX174.fasta.gz")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), fa, "--margins", str(tmp_path / "m.tsv")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "--margins" in r.stderr and "multi-rank" in r.stderr


def test_margin_entry_points_are_declared_and_exported(lib):
    txt = open(os.path.join(ROOT, "include", "phx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(phx_[a-z0-9_]+)\s*\(", txt))
    new = {"phx_margins_flat", "phx_tap_dist_target", "phx_margins_ms", "phx_format_margins"}
    assert new <= names and new <= set(lib.EXPORTS)
    L = lib.lib()
    for n in new:
        assert hasattr(L, n)
    assert lib.MARGIN_DT.itemsize == 40 and L.phx_version() == 410
