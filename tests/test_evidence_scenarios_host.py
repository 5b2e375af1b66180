"""Evidence scenario batches (phx_evidence_scenarios_flat), the parts that need no device: the host's list merge, the bit
rule of a bias slice, the binary search over a slot's sorted pair list and the slot byte count restated in numpy / python ints, the
--evidence-scan formatter and its argument refusals, and the new entry points of the header, the binding and the Annotator."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

B_MAX = 1 << 52


# ---- the list merge (scen_flat) ----
# Per scenario: the pairs sorted by ORF, duplicates summed in exact integers, a summed |B| > 2^52 refused, zero sums dropped, the ORFs the
# scenario refuses dropped.  What is left is one (ORF, B) per ORF in ascending order: the device never arbitrates.

def merge(pairs, refused):
    sums = {}
    for k, B in pairs:
        sums[k] = sums.get(k, 0) + B
    if any(abs(B) > B_MAX for B in sums.values()):
        raise ValueError("a bias beyond 2^52")
    return [(k, sums[k]) for k in sorted(sums) if sums[k] != 0 and k not in set(refused)]


def test_the_merge_sums_duplicates_drops_zero_sums_and_refused_orfs():
    assert merge([(5, -1000), (2, 7), (5, 400), (2, -7), (9, 1)], []) == [(5, -600), (9, 1)]
    assert merge([(5, -1000), (9, 1)], [5, 5, 7]) == [(9, 1)]
    assert merge([], [1]) == [] and merge([(3, 0)], []) == []
    # the bound holds for the sum, not for the parts; int64 parts cannot wrap a python sum
    assert merge([(1, B_MAX + 5), (1, -5)], []) == [(1, B_MAX)]
    assert merge([(1, 2 ** 62), (1, 2 ** 62), (1, -(2 ** 63)), (1, 3)], []) == [(1, 3)]
    for bad in ([(1, B_MAX + 1)], [(1, B_MAX), (1, 1)], [(4, -B_MAX), (4, -1), (2, 5)], [(1, 2 ** 62), (1, 2 ** 62)]):
        with pytest.raises(ValueError):
            merge(bad, [])
    with pytest.raises(ValueError):  # the refused ORF's bias is ignored only when it is a legal one
        merge([(1, B_MAX + 1)], [1])
    rng = np.random.RandomState(2001)
    for _ in range(200):
        pairs = [(int(rng.randint(12)), int(rng.randint(-3, 4))) for _ in range(rng.randint(0, 30))]
        refused = rng.randint(0, 12, rng.randint(0, 4)).tolist()
        got = merge(pairs, refused)
        assert [k for k, _ in got] == sorted({k for k, _ in got}) and all(B != 0 and k not in refused for k, B in got)
        dense = np.zeros(12, np.int64)  # evidence()'s own summing, per ORF of the contig
        for k, B in pairs:
            dense[k] += B
        dense[refused] = 0
        assert got == [(k, int(dense[k])) for k in range(12) if dense[k] != 0]


# ---- a biased slot's slices ----
# Every slot has a refused slice of ((edge_off & 31) + n_edge) / 32 + 2 words at mask0; a biased slot has a bias slice of the same size at
# bbit0 in the region behind all refused and all required slices.  k_sce_mask sets in-edge slot e as bit (edge_off & 31) + e of the slice;
# the solver reads bit edge_off + e of a pointer moved back by edge_off >> 5 words (sce_bbit, sc_view's rule).

def slice_words(edge_off, n_edge):
    return ((edge_off & 31) + n_edge) // 32 + 2


def writer_bit(base0, edge_off, e):  # k_sc_mask / k_sce_mask
    lo = edge_off & 31
    return base0 + ((lo + e) >> 5), (lo + e) & 31


def reader_bit(base0, edge_off, e):  # rs_refused / rs_biased / inorder_contig behind sc_view and sce_bbit
    base = base0 - (edge_off >> 5)
    x = edge_off + e
    return base + (x >> 5), x & 31


def test_a_bias_slice_keeps_edge_off_modulo_32_and_no_two_slots_share_a_bit():
    rng = np.random.RandomState(2002)
    for _ in range(300):
        n_contig = rng.randint(1, 6)
        n_edge = [int(rng.choice([1, 2, 31, 32, 33, 63, 64, 65, rng.randint(1, 5000)])) for _ in range(n_contig)]
        edge_off = np.concatenate([[0], np.cumsum(n_edge)]).tolist()
        slots = [(int(rng.randint(n_contig)), bool(rng.randint(2))) for _ in range(rng.randint(1, 12))]  # (contig, biased)
        slots.sort(key=lambda s: s[1])  # the biased slots follow the plain ones in the table
        mwords = sum(slice_words(edge_off[c], n_edge[c]) for c, _ in slots)
        bwords = sum(slice_words(edge_off[c], n_edge[c]) for c, b in slots if b)
        bias_base = mwords + 2 + 0 + 2  # behind the refused slices and the (empty) required region, each with two spare words
        owner, m0, b0 = {}, 0, 0
        for s, (c, biased) in enumerate(slots):
            eo, ne = edge_off[c], n_edge[c]
            for kind, base0 in (("F", m0),) + ((("B", bias_base + b0),) if biased else ()):
                for e in sorted({0, 1, ne // 2, ne - 1} | set(rng.randint(0, ne, 8).tolist())):
                    w = writer_bit(base0, eo, e)
                    assert w == reader_bit(base0, eo, e), (eo, e)
                    assert base0 <= w[0] < base0 + slice_words(eo, ne)
                    assert owner.setdefault(w, (s, kind, e)) == (s, kind, e)
            m0 += slice_words(eo, ne)
            if biased:
                b0 += slice_words(eo, ne)
                assert bias_base + b0 <= mwords + 2 + 2 + bwords + 2  # inside the buffer the host allocates and clears
        assert m0 == mwords and b0 == bwords


# ---- the sorted pair list and its search (k_sce_sort, bias_at under BLIST) ----

def rank_sort(keys):
    """k_sce_sort: a pair's place is the number of pairs in front of it, an equal key counting when it was staged earlier."""
    out = [None] * len(keys)
    for i, k in enumerate(keys):
        at = sum(1 for j, kj in enumerate(keys) if kj < k or (kj == k and j < i))
        assert out[at] is None
        out[at] = i
    return out


def bias_at(keys, vals, x):
    """bias_at<true>: the first pair whose key is >= x; its B when the key is x, else 0."""
    lo, hi = 0, len(keys)
    while lo < hi:
        mid = (lo + hi) >> 1
        if keys[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return vals[lo] if lo < len(keys) and keys[lo] == x else 0


def test_ranking_by_counting_sorts_and_the_binary_search_finds_every_pair_and_nothing_else():
    rng = np.random.RandomState(2003)
    for n in [0, 1, 2, 3, 4, 31, 32, 33, 64, 65, 257, 700]:
        edge_off = int(rng.randint(0, 1 << 33))  # the keys are in-edge slots of the batch: beyond 2^32 for a large one
        keys = (edge_off + rng.choice(4 * n + 8, n, replace=False)).tolist()
        vals = [int(v) for v in rng.randint(-(1 << 40), 1 << 40, n)]
        order = rank_sort(keys)
        skeys, svals = [keys[i] for i in order], [vals[i] for i in order]
        assert skeys == sorted(keys)
        for k, v in zip(keys, vals):
            assert bias_at(skeys, svals, k) == v
        for x in set(range(edge_off - 2, edge_off + 4 * n + 10)) - set(keys):
            assert bias_at(skeys, svals, x) == 0
    assert rank_sort([7, 3, 7, 3, 1]) == [4, 1, 3, 0, 2]  # equal keys keep their staging order: every place is taken once


# ---- the slot byte count (scen_slot_bytes) ----

DSCSLOT, DREANNREC, DGENE, DSCBIAS = 40, 40, 24, 40


def slot_bytes(V, E, nl, dmeta, pinned=False, n_bias=0):
    plain = V * (nl * 8 + 4 + 4) + (E // 32 + 3) * 4 + (V // 32 + 2) + (V + 1) * DGENE + dmeta + DSCSLOT + DREANNREC
    return plain + (V * 8 + (E // 32 + 3) * 4 + 16 if pinned else 0) + ((E // 32 + 3) * 4 + DSCBIAS + n_bias * 48 if n_bias else 0)


def test_a_biased_slot_costs_a_slice_a_record_and_48_bytes_per_listed_orf():
    V, E, nl = 2200, 20000, 2  # about a 50 kb contig
    for dmeta in (256, 512):
        plain = slot_bytes(V, E, nl, dmeta)
        assert slot_bytes(V, E, nl, dmeta, n_bias=0) == plain  # no bias: a plain slot
        one = slot_bytes(V, E, nl, dmeta, n_bias=1)
        assert one - plain == (E // 32 + 3) * 4 + 40 + 48
        assert slot_bytes(V, E, nl, dmeta, n_bias=65) - one == 64 * 48
        assert one - plain < 8 * E // 50  # a dense slice of one word per in-edge slot would be 8 E bytes
        # the list beats the dense slice until a sixth of the in-edge slots carry a bias; a contig has far fewer ORFs than that
        assert slot_bytes(V, E, nl, dmeta, n_bias=E // 6 - 100) - plain < 8 * E
    # the structures' sizes as the header lays them out: two int64, two int32, two uint64; int32 x 2 + int64
    assert DSCBIAS == 8 + 8 + 4 + 4 + 16 and 16 == 4 + 4 + 8


# ---- Annotator.evidence_scenarios' argument handling needs no device up to the library call ----

def test_bias_units_are_evidences():
    import math

    from phanotate_amd.api import Annotator

    assert Annotator._bias_units(0, 0, -1.5) == -1500 and Annotator._bias_units(0, 0, 0.0009) == 0 and Annotator._bias_units(0, 0, -0.0019) == -1
    for b in (2.5, -0.3, 1e6 + 0.1234, 4503599627370.496):
        assert Annotator._bias_units(0, 0, b) == math.trunc(b * 1000.0)
    for bad in (float("nan"), float("inf"), -float("inf"), 2.0 ** 60 / 1000.0):
        with pytest.raises(ValueError):
            Annotator._bias_units(3, 4, bad)


# ---- --evidence-scan ----

def test_evidence_scan_formatter_on_hand_made_records():
    from phanotate_amd import _lib
    from phanotate_amd.cli import format_evidence_scan

    assert _lib.EVSCAN_DT.names == ("left", "right", "strand", "orf", "bias", "status", "was_called", "delta", "called", "n_removed", "n_added")
    rec = np.zeros(6, _lib.EVSCAN_DT)
    rec[0] = (100, 402, 1, 7, -5.0, 0, 0, -1.25, 1, 1, 1)                   # a bonus that gets the ORF called
    rec[1] = (500, 900, -1, 11, 0.30000000000000004, 0, 1, 0.3, 1, 0, 0)    # reverse: START is the right end; a penalty the gene survives
    rec[2] = (1000, 1300, 1, 20, -40.0, -9, 0, np.inf, 0, 9, 0)            # the bonus makes a cycle negative
    rec[3] = (1000, 1300, 1, 20, 2.0, 0, 1, 0.0, 0, 1, 2)                  # an equal-length alternative takes over
    rec[4] = (1000, 1300, 1, 21, -0.0004, 0, 0, 0.0, 0, 0, 0)              # less than a unit: no bias
    rec[5] = (50, 200, -1, 2, 1.0, 1, 0, np.inf, 0, 0, 0)                  # no path
    status = np.array([0, -2, 1], np.int32)
    offsets = np.array([0, 5, 5, 6], np.int64)
    text = format_evidence_scan(["a", "bad", "c"], status, offsets, rec)
    head = "#START\tSTOP\tFRAME\tBIAS\tDELTA\tCALLED\tREMOVED\tADDED"
    assert text.splitlines() == [
        "#id:\ta", head,
        "100\t402\t+\t-5.0\t-1.25\t1\t1\t1",
        "900\t500\t-\t0.30000000000000004\t0.3\t1\t0\t0",
        "1000\t1300\t+\t-40.0\tcycle\t0\t9\t0",
        "1000\t1300\t+\t2.0\t0.0\t0\t1\t2",
        "1000\t1300\t+\t-0.0004\t0.0\t0\t0\t0",
        "#id:\tc", head,
        "200\t50\t-\t1.0\tinf\t0\t0\t0",
    ]
    assert format_evidence_scan([], np.zeros(0, np.int32), np.zeros(1, np.int64), rec[:0]) == ""
    for ln in text.splitlines()[2:4]:  # repr(bias) and repr(delta) read back to the same doubles
        assert repr(float(ln.split("\t")[3])) == ln.split("\t")[3] and repr(float(ln.split("\t")[4])) == ln.split("\t")[4]


def test_cli_refusals_of_evidence_scan_need_no_device(tmp_path):
    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    ev = tmp_path / "ev.txt"
    ev.write_text("1\t9\t+\tc1\t-1.0\n")
    out = tmp_path / "o.txt"
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    for bad, word in ((["--evidence-scan", str(ev), str(out), "-d"], b"--evidence-scan: not allowed with argument -d/--dump"),
                      (["--evidence-scan", str(ev), str(out), "--gpus", "2"], b"--evidence-scan: not available with --gpus above 1"),
                      (["--evidence-scan", str(ev)], b"--evidence-scan: expected 2 arguments")):
        r = subprocess.run(exe + bad, capture_output=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    r = subprocess.run(exe + ["--evidence-scan", str(ev), str(out)], capture_output=True, timeout=120, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and b"--evidence-scan: not available under a multi-rank launch" in r.stderr
    # --evidence keeps its own rules and messages beside it
    r = subprocess.run(exe + ["--evidence", str(ev), "--evidence-scan", str(ev), str(out)], capture_output=True, timeout=120)
    assert r.returncode == 2 and b"argument --evidence: needs --reannotation" in r.stderr
    assert not out.exists()


def test_the_parser_of_evidence_scan_is_evidences_and_names_its_flag():
    from phanotate_amd.cli import ForbidError, parse_evidence

    got = parse_evidence(["# c\n", "\n", "10\t99\t+\tc1\t-2.5\tnote\n", "300 100 - c2 1e-3\n"], "--evidence-scan")
    assert [e[:4] + e[5:] for e in got] == [(10, 99, 1, "c1", -2.5), (100, 300, -1, "c2", 0.001)]
    for bad in ("10\t99\t+\tc1\n", "10\t99\t+\tc1\tnan\n", "10\t99\t+\tc1\tinf\n", "10\t99\t*\tc1\t1.0\n", "a\t99\t+\tc1\t1.0\n"):
        with pytest.raises(ForbidError) as e:
            parse_evidence([bad], "--evidence-scan")
        assert str(e.value).startswith("--evidence-scan: ") and repr(bad.rstrip("\n")) in str(e.value)


# ---- the entry points ----

def test_header_exports_and_annotator_methods():
    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    m = re.search(r"int phx_evidence_scenarios_flat\(([^;]*)\);", text)
    assert m is not None
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "n_scen", "scen_contig", "forbid_off", "forbid_orf", "bias_off", "bias_orf", "bias_val", "orf_offsets", "flags",
                                                        "genes", "cap", "offsets", "status", "delta", "total"]
    assert re.search(r"#define PHX_VERSION 410\b", text)  # (callers probe for the symbol)
    assert "phx_evidence_scenarios_flat" in _lib.EXPORTS
    L = _lib.lib()
    assert len(L.phx_evidence_scenarios_flat.argtypes) == 16 and len(L.phx_pinned_scenarios_flat.argtypes) == 16 and len(L.phx_scenarios_flat.argtypes) == 13
    # argument errors come before any device work: without a context, PHX_E_ARG
    assert L.phx_evidence_scenarios_flat(None, 0, None, None, None, None, None, None, None, 0, None, 0, None, None, None, None) == -1
    for name in ("evidence_scenarios", "evidence_scan", "evidence", "scenarios", "scenario_path", "scenarios_ms", "scenario_chunks"):
        assert callable(getattr(api.Annotator, name)), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "No scenario batches of biased solves" not in design and "## 20. " in design
