"""Coding profiles, the parts that need no GPU: the two-entry sparse table with push-down that k_pf_cand runs, restated
in Python against brute force; the 64-bit key (the bit pattern of float(Delta) / 1000.0 orders like Delta); format_profile; the command
line's rows; the record's size and the prototypes."""
import math
import os
import random
import re
import struct

import numpy as np
import pytest

from phanotate_amd import _lib, cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NONE = struct.unpack("<Q", struct.pack("<d", INF))[0]  # PF_NONE


def key_of(delta):
    """the table's key of an edge: the bit pattern of mu = float(delta) / 1000.0 as an unsigned integer"""
    return struct.unpack("<Q", struct.pack("<d", float(delta) / 1000.0))[0]


def sparse_min(n, intervals):
    """k_pf_cand's table for one track over n slots: intervals = [(a, z, key)] with 0 <= a <= z < n.  Level k entry i covers the slots
    [i, i + 2^k); an interval goes to level floor(log2 len) at both ends; the push-down gathers level k-1 entry i from level k at i and at
    i - 2^(k-1).  Returns level 0."""
    lv = 1
    while (2 << (lv - 1)) <= n:
        lv += 1
    tab = [NONE] * (n * lv)
    for a, z, key in intervals:
        k = (z - a + 1).bit_length() - 1
        assert 0 <= k < lv and 0 <= a and z < n
        for i in (k * n + a, k * n + z - (1 << k) + 1):
            tab[i] = min(tab[i], key)
    for k in range(lv - 1, 0, -1):
        h = 1 << (k - 1)
        for i in range(n):
            m = tab[k * n + i]
            if i >= h:
                m = min(m, tab[k * n + i - h])
            if m != NONE:
                tab[(k - 1) * n + i] = min(tab[(k - 1) * n + i], m)
    return tab[:n]


def brute_min(n, intervals):
    out = [NONE] * n
    for a, z, key in intervals:
        for s in range(a, z + 1):
            out[s] = min(out[s], key)
    return out


SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 257)


def test_sparse_table_matches_brute_force():
    rng = random.Random(34)
    for trial in range(2000):
        n = SIZES[trial % len(SIZES)]
        kind = (trial // len(SIZES)) % 5
        if kind == 0:  # an empty track
            iv = []
        elif kind == 1:  # ranges of length 1 only
            iv = [(a, a, rng.randrange(1 << 62)) for a in (rng.randrange(n) for _ in range(rng.randrange(1, 2 * n + 1)))]
        elif kind == 2:  # full ranges, and equal keys among them
            iv = [(0, n - 1, rng.choice((5, 5, 7, 1 << 40))) for _ in range(rng.randrange(1, 4))]
        else:  # anything; kind 4 draws the keys from three values, so that equal keys meet
            iv = []
            for _ in range(rng.randrange(1, 3 * n + 2)):
                a = rng.randrange(n)
                z = rng.randrange(a, n)
                iv.append((a, z, rng.choice((0, 17, NONE - 1)) if kind == 4 else rng.randrange(NONE)))
        assert sparse_min(n, iv) == brute_min(n, iv), (n, kind, iv)


def test_key_is_monotone_in_delta():
    """float(a) / 1000 <= float(b) / 1000 for Python ints 0 <= a <= b, and the patterns of the quotients order the same way as unsigned
    integers: the minimum of the keys is the key of the minimum Delta, so min of mu = mu of min."""
    rng = random.Random(35)
    for trial in range(20000):
        bits = rng.choice((1, 8, 52, 53, 54, 63, 64, 65, 128, 500, 1000))
        a = rng.randrange(1 << bits)
        step = rng.choice((0, 1, 2, 999, 1000, 1001, rng.randrange(1 << max(bits - 50, 1)), rng.randrange(1 << bits)))
        b = min(a + step, (1 << 1000) - 1) if trial % 2 else rng.randrange(a, min(a + (1 << bits), 1 << 1000))
        assert 0 <= a <= b < (1 << 1000)
        ma, mb = float(a) / 1000.0, float(b) / 1000.0
        assert ma <= mb
        ka, kb = key_of(a), key_of(b)
        assert (ka <= kb) and (ka == kb) == (ma == mb) and kb < NONE
    # ... and so over a set: the minimum of the keys is the key of the exact minimum
    for trial in range(500):
        ds = [rng.randrange(1 << rng.choice((10, 60, 70, 300))) for _ in range(rng.randrange(1, 9))]
        assert min(key_of(d) for d in ds) == key_of(min(ds))
        assert struct.unpack("<d", struct.pack("<Q", min(key_of(d) for d in ds)))[0] == min(float(d) / 1000.0 for d in ds) == float(min(ds)) / 1000.0
    assert key_of(0) == 0 and math.isinf(struct.unpack("<d", struct.pack("<Q", NONE))[0])


def slots(rows):
    return np.array(rows, _lib.PROFILE_DT)


def test_format_profile():
    rec = slots([
        (0, 10, INF, INF, 0.0),      # contig a
        (10, 10, 1.0, 2.0, 3.0),     #   an empty slot: left out, and it does not break the run around it ...
        (10, 25, INF, INF, 0.0),     #   ... so this one merges with the first
        (25, 40, 0.0, 1.5, 12.25),
        (40, 40, 0.0, 1.5, 12.25),   #   empty
        (40, 90, 0.0, 1.5, 12.25),   #   merges
        (90, 101, 0.0, 1.5, 12.5),   #   one value differs: a row of its own
        (0, 7, INF, INF, INF),       # contig c: no path
        (7, 9, INF, INF, INF),
    ])
    status = np.array([0, -2, 1, 0], np.int32)
    offsets = np.array([0, 7, 7, 9, 9], np.int64)
    text = cli.format_profile(["a", "bad", "c", "empty"], status, offsets, rec).decode()
    assert text == ("#id:\ta\n#LO\tHI\tFWD\tREV\tGAP\n"
                    "0\t25\tINF\tINF\t0.000000E+00\n"
                    "25\t90\t0.000000E+00\t1.500000E+00\t1.225000E+01\n"
                    "90\t101\t0.000000E+00\t1.500000E+00\t1.250000E+01\n"
                    "#id:\tc\n#LO\tHI\tFWD\tREV\tGAP\n"
                    "0\t9\tINF\tINF\tINF\n"
                    "#id:\tempty\n#LO\tHI\tFWD\tREV\tGAP\n")
    # numbers as format_margins prints a margin
    m = np.zeros(1, _lib.MARGIN_DT)
    m["left"], m["right"], m["strand"], m["through"], m["margin"], m["score"] = 1, 9, 1, 1, 12.25, -3.0
    assert "1.225000E+01" in cli.format_margins(["a"], np.zeros(1, np.int32), np.array([0, 1], np.int64), m).decode()
    assert cli.format_profile([], np.zeros(0, np.int32), np.zeros(1, np.int64), slots([])) == b""


# the two orders as they stood before --profile
PARENT_CHECK_ORDER = ("margins", "drop_margins", "drop_replacements", "start_drops", "alt_starts", "evidence_scan", "curated_scan", "remargins", "redrop_margins", "redrop_replacements", "pin_margins", "pin_drop_margins", "pin_drop_replacements", "forbid", "require", "evidence", "reannotation")
PARENT_FETCH_ORDER = ("margins", "drop_replacements", "drop_margins", "start_drops", "alt_starts", "evidence_scan", "reannotation", "curated_scan", "remargins", "redrop_margins", "redrop_replacements", "pin_margins", "pin_drop_margins", "pin_drop_replacements")


def test_cli_rows(tmp_path, monkeypatch, capsys):
    row = cli.OUTPUTS["profile"]
    assert row.flag == "--profile" and row.fmt is cli.format_profile and row.mode == "wb" and row.resident and row.piped is None
    for order, parent in ((cli._CHECK_ORDER, PARENT_CHECK_ORDER), (cli._FETCH_ORDER, PARENT_FETCH_ORDER)):
        assert order.count("profile") == 1
        assert tuple(x for x in order if x != "profile") == parent
    assert not [r for r in cli._RULES if r[0] == "profile"]  # it needs nothing else and conflicts with nothing
    fa = tmp_path / "in.fasta"
    fa.write_text(">a\nacgt\n")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = cli.get_args([str(fa), "--profile", "p.tsv"])
    assert args.profile == "p.tsv"
    args = cli.get_args([str(fa), "--profile", "p.tsv", "--margins", "m.tsv", "--drop-margins", "d.tsv"])
    assert (args.profile, args.margins, args.drop_margins) == ("p.tsv", "m.tsv", "d.tsv")
    for more, want in ((["--dump"], "argument --profile: not allowed with argument -d/--dump"), (["--gpus", "2"], "argument --profile: not available with --gpus above 1")):
        with pytest.raises(SystemExit):
            cli.get_args([str(fa), "--profile", "p.tsv"] + more)
        assert capsys.readouterr().err.rstrip().endswith("error: " + want)


def test_record_and_prototypes():
    assert _lib.PROFILE_DT.itemsize == 32
    assert [(_lib.PROFILE_DT.fields[k][1], _lib.PROFILE_DT.fields[k][0].str) for k in ("lo", "hi", "fwd", "rev", "gap")] == [(0, "<i4"), (4, "<i4"), (8, "<f8"), (16, "<f8"), (24, "<f8")]
    txt = open(os.path.join(ROOT, "include", "phx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    flat = re.sub(r"\s+", " ", txt)
    assert "int phx_profile_flat(phx_ctx *ctx, phx_profile_slot *rec, int64_t cap, int64_t *offsets , int32_t *status , int64_t *total);" in flat
    assert "int phx_profile_ms(phx_ctx *ctx, float *ms );" in flat
    assert re.search(r"typedef struct phx_profile_slot \{ int32_t lo, hi; double fwd, rev, gap; \} phx_profile_slot;", flat)
    assert "phx_profile_flat" in _lib.EXPORTS and "phx_profile_ms" in _lib.EXPORTS
