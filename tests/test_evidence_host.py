"""Host side of the evidence-weighted re-annotation (no GPU): the header, the export list and the entry point without a
context, --evidence's parsing and refusals, and the overflow rule's arithmetic restated in Python integers."""
import math
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_header_exports_and_annotator_method():
    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    m = re.search(r"int phx_evidence_flat\(([^;]*)\);", text)
    assert m is not None
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "bias", "forbid", "orf_offsets", "flags", "genes", "cap", "offsets", "status", "delta", "total"]
    assert args[1] == "const int64_t *bias"
    assert "phx_evidence_flat" in _lib.EXPORTS
    assert re.search(r"#define PHX_VERSION 410\b", text)  # callers probe for the symbol
    L = _lib.lib()
    assert len(L.phx_evidence_flat.argtypes) == 11
    assert L.phx_evidence_flat(None, None, None, None, 0, None, 0, None, None, None, None) == -1  # PHX_E_ARG without a context
    assert callable(api.Annotator.evidence)


def test_evidence_file_round_trip_fifth_column_and_duplicates():
    from phanotate_amd.cli import ForbidError, parse_evidence, parse_forbid, resolve_evidence

    lines = ["# hits\n", "\n", "100\t400\t+\tc1\t-3.5\n", "900 300 - c2 2\n", "100\t400\t+\tc1\t-1.25\tblastp\n", "7\t70\t+\tc1\t1e3\n"]
    ents = parse_evidence(lines)
    assert [e[:5] for e in ents] == parse_forbid(lines, "--evidence")  # parse_forbid's rules for the first four columns
    assert [e[5] for e in ents] == [-3.5, 2.0, -1.25, 1000.0]
    # written back as START STOP FRAME CONTIG BIAS, the entries read the same
    again = parse_evidence(["%d\t%d\t%s\t%s\t%r\n" % (((lo, hi) if st > 0 else (hi, lo)) + ("+" if st > 0 else "-", nm, b)) for lo, hi, st, nm, _, b in ents])
    assert [e[:4] + e[5:] for e in again] == [e[:4] + e[5:] for e in ents]

    table = {(0, 100, 400, 1): 5, (1, 300, 900, -1): 0, (0, 7, 70, 1): 2}

    def lookup(i, left, right, strand):
        return table[(i, left, right, strand)]

    assert resolve_evidence(ents, ["c1", "c2"], lookup) == [[(5, -3.5), (5, -1.25), (2, 1000.0)], [(0, 2.0)]]  # a duplicate stays: evidence() sums
    assert resolve_evidence(ents[:1], ["c1", "c2"], lookup) == [[(5, -3.5)], None]
    with pytest.raises(ForbidError) as e:
        resolve_evidence(parse_evidence(["17\t23\t+\tc1\t1\n"]), ["c1", "c2"], lookup)
    assert str(e.value).startswith("--evidence: no such ORF in its contig") and repr("17\t23\t+\tc1\t1") in str(e.value)
    # malformed lines are quoted: the first four columns by parse_forbid's message, the fifth by its own
    with pytest.raises(ForbidError) as e:
        parse_evidence(["100\t400\tx\tc1\t1.0\n"])
    assert str(e.value).startswith("--evidence: not START STOP FRAME CONTIG") and repr("100\t400\tx\tc1\t1.0") in str(e.value)
    for bad in ("100\t400\t+\tc1", "100\t400\t+\tc1\tstrong", "100\t400\t+\tc1\tnan", "100\t400\t+\tc1\t-inf", "100 400 + c1", "100\t400\t+\tc1\t"):
        with pytest.raises(ForbidError) as e:
            parse_evidence([bad + "\n"])
        assert str(e.value).startswith("--evidence: no finite BIAS in the fifth column") and repr(bad) in str(e.value), bad


def test_cli_refusals_of_evidence_need_no_device(tmp_path):
    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    ev = tmp_path / "e.txt"
    ev.write_text("1\t9\t+\tc1\t-2.5\n")
    out = tmp_path / "o.txt"
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    for bad, word in ((["--evidence", str(ev)], b"--evidence: needs --reannotation"),
                      (["--evidence", str(ev), "--reannotation", str(out), "--require", str(ev)], b"--evidence: not allowed with argument --require"),
                      (["--evidence", str(ev), "--reannotation", str(out), "-d"], b"-d/--dump"),
                      (["--evidence", str(ev), "--reannotation", str(out), "--gpus", "2"], b"--evidence: not available with --gpus above 1"),
                      (["--reannotation", str(out)], b"each needs the other")):
        r = subprocess.run(exe + bad, capture_output=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    r = subprocess.run(exe + ["--evidence", str(ev), "--reannotation", str(out)], capture_output=True, timeout=120, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and b"multi-rank" in r.stderr


# ---- the overflow rule (phx_layout.inc contig_sum_bits, k_rs_mask's sums, the limb test of k_rs_lds under the bias policy), restated ----

B_MAX = 1 << 52  # phx_evidence_flat refuses |B| beyond it


def sum_bits(bound, extra, maxexp):
    """contig_sum_bits: the binary exponent of the fp64 bound (plus `extra` when positive), or the widest single weight's, plus 5."""
    x = bound + extra if extra > 0.0 else bound
    return max(math.frexp(x)[1], maxexp) + 5


def device_extra(bs):
    """The sum of |B| as k_rs_mask adds it up (two 64-bit counters, the low and the high 32 bits of every |B|) and k_rs_lds reads it under the bias policy."""
    lo = sum(abs(b) & 0xFFFFFFFF for b in bs)
    hi = sum(abs(b) >> 32 for b in bs)
    assert lo < 1 << 64 and hi < 1 << 64
    return float(hi) * 4294967296.0 + float(lo)


def test_the_overflow_rule_restated():
    rng = random.Random(1901)
    # 1. the two halves cannot wrap for any contig (fewer than 2^31 ORFs, |B| <= 2^52) and give the sum to fp64's precision
    assert (1 << 31) * (B_MAX & 0xFFFFFFFF or 0xFFFFFFFF) < 1 << 64 and (1 << 31) * (B_MAX >> 32) < 1 << 64
    for _ in range(200):
        bs = [rng.choice((-1, 1)) * rng.randint(1, B_MAX) for _ in range(rng.randint(1, 400))]
        want = sum(abs(b) for b in bs)
        assert abs(device_extra(bs) - want) <= want * 2.0 ** -51
    assert device_extra([B_MAX] * 1000) == float(1000 * B_MAX) and device_extra([-B_MAX, 3, -5]) == float(B_MAX + 8)
    # 2. extra = 0 is the layout's own figure; a positive one only ever raises it
    for _ in range(200):
        bound, maxexp = rng.uniform(1e3, 1e30), rng.randint(0, 80)
        assert sum_bits(bound, 0.0, maxexp) == max(math.frexp(bound)[1], maxexp) + 5
        assert sum_bits(bound, rng.uniform(0, 1e30), maxexp) >= sum_bits(bound, 0.0, maxexp)
    # 3. what the rule buys.  A tentative distance of a biased solve is a walk that uses every ORF edge at most once: |d| <= bound + sum|B|
    #    < 2^eb (one of the five bits covers the rounding of the fp64 sum).  While bits = eb + 5 <= 64 NL, every candidate d + w stays below
    #    the threshold of the unreached pattern, 2^(64 NL - 3), and the unreached pattern 2^(64 NL - 2) plus any weight stays above it.
    for nl in (2, 4, 8, 17):
        eb = 64 * nl - 5  # the largest exponent the class admits
        worst = (1 << eb) * 2  # |d| + |w|, each below 2^eb
        assert worst < 1 << (64 * nl - 3)
        assert (1 << (64 * nl - 2)) - (1 << eb) >= 1 << (64 * nl - 3)
        assert eb + 5 <= 64 * nl < (eb + 1) + 5
    # 4. the classes: a contig whose bound sits at 2^100 is a 128-bit contig; biases push it out only when bound + sum|B| crosses 2^123
    bound = 2.0 ** 100
    assert sum_bits(bound, 0.0, 0) == 106 and sum_bits(bound, device_extra([B_MAX] * 4096), 0) == 106
    assert sum_bits(2.0 ** 123 * (1 - 2.0 ** -53), 0.0, 0) == 128 and sum_bits(2.0 ** 123 * (1 - 2.0 ** -53), device_extra([B_MAX] * (1 << 20)), 0) == 129
    # ... and no real contig gets there: all its ORFs at 2^52 add less than 2^83, so the unbiased bound would have to lie within 2^-40 of its
    # class's edge — the overflow status exists for completeness, the GPU suite cannot reach it
    assert (1 << 31) * B_MAX == 1 << 83
    for nl in (2, 4, 8):  # (1088 bits: fp64 ends at 2^1024, below that class's edge — no fp64 bound leaves it)
        edge = 2.0 ** (64 * nl - 5)
        below = edge * (1 - 2.0 ** -39)
        assert sum_bits(below, float(1 << 83), 0) == 64 * nl  # still inside


def test_python_bias_conversion_is_trunc_of_thousandths():
    # what Annotator.evidence documents: B = math.trunc(b * 1000.0), towards zero on both sides
    assert [math.trunc(b * 1000.0) for b in (0.0004, -0.0004, 1.9999, -1.9999, 2.5, -0.001, 1e-9)] == [0, 0, 1999, -1999, 2500, -1, 0]
    assert math.trunc((B_MAX / 1000.0) * 1000.0) <= B_MAX
