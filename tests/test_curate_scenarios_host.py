"""Combined scenario batches (phx_curate_scenarios_flat), the parts that need no device: the entry point in the header, the
binding and the Annotator, what Annotator.curate_scenarios() hands to the library (read back from a stub in the library's place), the slot
table's four ranges and the tile path's flag fields under REQ with BLIST restated in python, the --curated-scan formatter and refusals,
and the seeded draws the GPU test hands to the device as one call, counted on the CPU oracle's graphs."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_evidence_gpu import settle

import curate_draws as cd


# ---- the entry points ----
def test_header_binding_annotator_methods_and_record_type():
    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    m = re.search(r"int phx_curate_scenarios_flat\(([^;]*)\);", text)
    assert m is not None
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "n_scen", "scen_contig", "forbid_off", "forbid_orf", "require_off", "require_orf", "bias_off", "bias_orf", "bias_val",
                                                        "orf_offsets", "flags", "genes", "cap", "offsets", "status", "delta", "unmet", "total"]
    assert args[9] == "const int64_t *bias_val" and args[17] == "int32_t *unmet"
    assert re.search(r"#define PHX_VERSION 410\b", text)  # (callers probe for the symbol)
    assert "phx_curate_scenarios_flat — probe for the symbol" in text and "since added: phx_curate_scenarios_flat" in text
    assert "phx_curate_scenarios_flat" in _lib.EXPORTS
    L = _lib.lib()
    assert len(L.phx_curate_scenarios_flat.argtypes) == 19
    # argument errors come before any device work: without a context, PHX_E_ARG
    assert L.phx_curate_scenarios_flat(None, 0, None, None, None, None, None, None, None, None, None, 0, None, 0, None, None, None, None, None) == -1
    for name in ("curate_scenarios", "curated_scan", "curate", "pinned_scenarios", "evidence_scenarios"):
        assert callable(getattr(api.Annotator, name)), name
    assert _lib.CUSCAN_DT.names == _lib.EVSCAN_DT.names + ("unmet", "base_status", "base_delta", "base_unmet")
    for name in _lib.EVSCAN_DT.names:
        assert _lib.CUSCAN_DT[name] == _lib.EVSCAN_DT[name], name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 27. " in design and design.count("(since added: §27)") >= 2


# ---- what curate_scenarios() hands over ----
class Stub:
    """An Annotator whose library call is recorded instead of made: two contigs of 10 and 15 ORFs."""

    def __new__(cls):
        from phanotate_amd.api import Annotator

        ann = object.__new__(Annotator)
        ann.n, ann._orf_offs, ann.calls = 2, np.array([0, 10, 25], np.int64), []
        ann.L = type("L", (), {"phx_curate_scenarios_flat": "the entry point"})()

        def genes_flat(fn, name, head, count, with_unmet):
            S = head[0]
            rd = lambda p, n, ct: np.ctypeslib.as_array((ct * n).from_address(p.value)).copy()
            foff, roff, boff = rd(head[2], S + 1, C.c_int64), rd(head[4], S + 1, C.c_int64), rd(head[6], S + 1, C.c_int64)
            ann.calls.append(dict(fn=fn, name=name, S=S, count=count, with_unmet=with_unmet, flags=head[10], contig=rd(head[1], max(S, 1), C.c_int32)[:S].tolist(), foff=foff.tolist(),
                                  forf=rd(head[3], max(int(foff[-1]), 1), C.c_int32)[:foff[-1]].tolist(), roff=roff.tolist(), rorf=rd(head[5], max(int(roff[-1]), 1), C.c_int32)[:roff[-1]].tolist(),
                                  boff=boff.tolist(), borf=rd(head[7], max(int(boff[-1]), 1), C.c_int32)[:boff[-1]].tolist(), bval=rd(head[8], max(int(boff[-1]), 1), C.c_int64)[:boff[-1]].tolist(),
                                  oo=rd(head[9], 3, C.c_int64).tolist(), n_head=len(head)))
            return "result"

        ann._genes_flat = genes_flat
        return ann


def test_curate_scenarios_marshals_offsets_duplicates_and_none_lists():
    ann = Stub()
    scen = [(1, [(3, -2.5), (3, 1.0), (14, 0.0004)], [2, 2, 7], np.array([3, 9])),  # duplicates of every kind go through as given: the library merges
            (0, None, None, None),
            (0, {4: 1.5}, None, [5]),
            (1, None, [0], None),
            (0, [(9, -0.001)], [], [])]
    assert ann.curate_scenarios(scen) == "result"
    (c,) = ann.calls
    assert c["fn"] == "the entry point" and c["name"] == "phx_curate_scenarios_flat" and c["S"] == 5 and c["count"] == 5 and c["with_unmet"] is True
    assert c["n_head"] == 11 and c["flags"] == 0 and c["oo"] == [0, 10, 25]
    assert c["contig"] == [1, 0, 0, 1, 0]
    assert c["foff"] == [0, 3, 3, 3, 4, 4] and c["forf"] == [2, 2, 7, 0]
    assert c["roff"] == [0, 2, 2, 3, 3, 3] and c["rorf"] == [3, 9, 5]
    assert c["boff"] == [0, 3, 3, 4, 4, 5] and c["borf"] == [3, 3, 14, 4, 9] and c["bval"] == [-2500, 1000, 0, 1500, -1]
    # no scenario at all: arrays of one spare entry, offsets [0]
    assert ann.curate_scenarios([]) == "result"
    assert ann.calls[1]["S"] == 0 and ann.calls[1]["foff"] == ann.calls[1]["roff"] == ann.calls[1]["boff"] == [0]
    # a generator is taken once
    ann.curate_scenarios(s for s in scen[:2])
    assert ann.calls[2]["contig"] == [1, 0]


def test_curate_scenarios_raises_the_siblings_errors_before_the_library_call():
    ann = Stub()
    for bad in ([(0, None, None)], [(0, None, None, None, None)], [7], [(0, [(1, 2.0, 3)], None, None)]):
        with pytest.raises(ValueError):
            ann.curate_scenarios(bad)
    for bad in ([(2, None, None, None)], [(-1, None, None, None)], [(0, None, [10], None)], [(0, None, None, [-1])], [(1, None, None, [15])], [(0, [(10, 1.0)], None, None)],
                [(0, {-1: 1.0}, None, None)]):
        with pytest.raises(IndexError):
            ann.curate_scenarios(bad)
    for b in (float("nan"), float("inf"), 2.0 ** 60 / 1000.0):
        with pytest.raises(ValueError):
            ann.curate_scenarios([(0, [(1, b)], None, [2])])
    with pytest.raises(ValueError):  # the sum counts
        ann.curate_scenarios([(0, [(1, 2.0 ** 52 / 1000.0 * 0.75), (1, 2.0 ** 52 / 1000.0 * 0.75)], None, [2])])
    assert ann.calls == []
    ann.curate_scenarios([(1, [(14, 1.0)], [14], [13])])  # a refused ORF's bias is the library's to drop; refused and required in one scenario its to refuse
    assert len(ann.calls) == 1


def test_evidence_scenarios_still_hands_over_what_it_did():
    """The bias marshalling is shared with evidence_scenarios(): its arrays are what they were."""
    from phanotate_amd.api import Annotator

    boff, borf, bval = Annotator._scenario_bias_arrays([(1, [(3, -2.5), (3, 1.0)]), (0, None), (0, {4: 1.5})], np.array([0, 10, 25]))
    assert boff.tolist() == [0, 2, 2, 3] and borf.tolist() == [3, 3, 4] and bval.tolist() == [-2500, 1000, 1500]
    assert borf.dtype == np.int32 and bval.dtype == np.int64 and boff.dtype == np.int64
    boff, borf, bval = Annotator._scenario_bias_arrays([], np.array([0]))
    assert boff.tolist() == [0] and len(borf) == 1 and len(bval) == 1


# ---- the slot table's four ranges (scen_compute, scen_range) ----
EV0 = 1 << 30


def table(kinds):
    """A chunk's slot table from the scenarios' kinds in call order ((pinned, biased) each): the index a scenario's pairs carry until the
    chunk is closed, and its place in the closed table — plain, pinned, biased, both."""
    count = {0: 0, 1: 0, 2: 0, 3: 0}
    ids = []
    for pinned, biased in kinds:
        r = 3 if pinned and biased else 1 if pinned else 2 if biased else 0
        k = count[r]
        ids.append((r, -1 - EV0 - k if r == 3 else -1 - k if r == 1 else EV0 + k if r == 2 else k))
        count[r] += 1
    n_plain, n_head, n_first3 = count[0], count[0] + count[1], count[0] + count[1] + count[2]
    place = lambda x: n_first3 + (-1 - EV0 - x) if x < -EV0 else n_plain + (-1 - x) if x < 0 else n_head + (x - EV0) if x >= EV0 else x
    return [place(x) for _, x in ids], [r for r, _ in ids], [count[r] for r in range(4)]


def test_the_fourth_range_sits_behind_the_biased_one_and_every_slot_has_one_place():
    rng = np.random.RandomState(2701)
    for _ in range(200):
        kinds = [(bool(rng.randint(2)), bool(rng.randint(2))) for _ in range(rng.randint(1, 40))]
        places, ranges, n_range = table(kinds)
        assert sorted(places) == list(range(len(kinds)))
        first = np.concatenate([[0], np.cumsum(n_range)])  # scen_range's `first` of every range
        for p, r in zip(places, ranges):
            assert first[r] <= p < first[r + 1]
        for r in range(4):  # a range keeps the call's order
            mine = [p for p, rr in zip(places, ranges) if rr == r]
            assert mine == sorted(mine)
        # k_sce_sort's one launch over ranges 2 and 3: blockIdx.x + first[2] runs to the table's end
        assert first[2] + n_range[2] + n_range[3] == len(kinds)
    # the ends of the index ranges: EV0 - 1 slots of a kind do not collide or overflow an int
    assert -1 - EV0 - (EV0 - 1) == -(1 << 31) and -1 - (EV0 - 1) == -EV0 and EV0 + (EV0 - 1) == (1 << 31) - 1


DSCSLOT, DREANNREC, DGENE, DSCBIAS = 40, 40, 24, 40


def slot_bytes(V, E, nl, dmeta, pinned=False, n_bias=0):
    plain = V * (nl * 8 + 4 + 4) + (E // 32 + 3) * 4 + (V // 32 + 2) + (V + 1) * DGENE + dmeta + DSCSLOT + DREANNREC
    return plain + (V * 8 + (E // 32 + 3) * 4 + 16 if pinned else 0) + ((E // 32 + 3) * 4 + DSCBIAS + n_bias * 48 if n_bias else 0)


def test_a_both_slot_costs_the_pinned_and_the_biased_part_together():
    V, E, nl, dmeta = 2200, 20000, 2, 256
    plain = slot_bytes(V, E, nl, dmeta)
    pin, ev, both = slot_bytes(V, E, nl, dmeta, True), slot_bytes(V, E, nl, dmeta, n_bias=3), slot_bytes(V, E, nl, dmeta, True, 3)
    assert both - plain == (pin - plain) + (ev - plain) and both > pin > plain and both > ev
    assert slot_bytes(V, E, nl, dmeta, True, 0) == pin  # every bias refused or zero: the pinned slot


# ---- the tile path's flags under REQ with BLIST (lds_sweep) ----
def fill_both_list(r_mk, r_mb, j, W, B, M, mod):
    """One prefetched row under RePol<true, true, true>: the unrolled fill writes W, minus M where bit 16 + j of r_mk is set, or no edge
    where bit j is; the block behind it adds B to the entry where bit j of r_mb is set and bit j of r_mk is not.  None: no edge."""
    w = W
    if (r_mk >> (16 + j)) & 1:
        w = (w - M) % mod
    entry = None if (r_mk >> j) & 1 else w
    if r_mb and (r_mb >> j) & 1 and not (r_mk >> j) & 1:
        entry = (entry + B) % mod
    return entry


def test_b_after_the_top_limb_equals_b_first_on_the_sweeps_limbs():
    rng = np.random.RandomState(2702)
    for nl in (2, 4, 8, 17):
        snl = nl + 1
        mod, M = 1 << (64 * snl), 1 << (64 * nl)
        for _ in range(300):
            ept = 2
            W = [int(rng.randint(-(1 << 40), 1 << 40)) << int(rng.randint(0, 64 * nl - 44)) for _ in range(ept)]
            B = [int(rng.randint(-(1 << 52), (1 << 52) + 1)) for _ in range(ept)]
            refused, required, biased = [rng.randint(4) == 0 for _ in range(ept)], [bool(rng.randint(2)) for _ in range(ept)], [bool(rng.randint(2)) for _ in range(ept)]
            r_mk = sum(1 << j for j in range(ept) if refused[j]) | sum(0x10000 << j for j in range(ept) if required[j])
            r_mb = sum(1 << j for j in range(ept) if biased[j])
            for j in range(ept):
                want = None if refused[j] else (W[j] + (B[j] if biased[j] else 0) - (M if required[j] else 0)) % mod  # §22: W + B - M
                assert fill_both_list(r_mk, r_mb, j, W[j] % mod, B[j], M, mod) == want
    # the required flags are never read as biased ones: a required row without a bias keeps W - M
    assert fill_both_list(0x10000, 0, 0, 5, 999, 1 << 128, 1 << 192) == (5 - (1 << 128)) % (1 << 192)


# ---- --curated-scan ----
def test_curated_scan_formatter_on_hand_made_records():
    from phanotate_amd import _lib
    from phanotate_amd.cli import format_curated_scan

    rec = np.zeros(5, _lib.CUSCAN_DT)
    rec[0] = (100, 402, 1, 7, -5.0, 0, 0, 3.75, 1, 1, 1, 0, 0, 5.0, 0)                    # a bonus that gets the ORF called under the pins
    rec[1] = (500, 900, -1, 11, 0.30000000000000004, 0, 1, 5.3, 1, 0, 0, 1, 0, 5.0, 0)    # reverse: START is the right end; a pin given up
    rec[2] = (1000, 1300, 1, 20, -40.0, -9, 0, np.inf, 0, 9, 0, 2, 0, 5.0, 0)            # the bonus makes a cycle negative: unmet = |R|
    rec[3] = (50, 200, -1, 2, 1.0, 1, 0, np.inf, 0, 0, 0, 1, 1, np.inf, 1)               # a contig whose baseline has no path
    rec[4] = (60, 210, 1, 3, -1.0, -9, 0, np.inf, 0, 0, 0, 1, -9, np.inf, 1)             # ... and one whose baseline is a cycle through a pin
    status = np.array([0, -2, 1, 0, 0], np.int32)
    offsets = np.array([0, 3, 3, 4, 5, 5], np.int64)
    text = format_curated_scan(["a", "bad", "c", "d", "e"], status, offsets, rec)
    head = "#START\tSTOP\tFRAME\tBIAS\tDELTA\tCALLED\tREMOVED\tADDED\tUNMET"
    assert text.splitlines() == [
        "#id:\ta", "#base:\t5.0\t0", head,
        "100\t402\t+\t-5.0\t3.75\t1\t1\t1\t0",
        "900\t500\t-\t0.30000000000000004\t5.3\t1\t0\t0\t1",
        "1000\t1300\t+\t-40.0\tcycle\t0\t9\t0\t2",
        "#id:\tc", "#base:\tinf\t1", head,
        "200\t50\t-\t1.0\tinf\t0\t0\t0\t1",
        "#id:\td", "#base:\tcycle\t1", head,
        "60\t210\t+\t-1.0\tcycle\t0\t0\t0\t1",
        "#id:\te", head,  # no line of FILE names the contig: no baseline was solved
    ]
    assert format_curated_scan([], np.zeros(0, np.int32), np.zeros(1, np.int64), rec[:0]) == ""
    # --evidence-scan's columns, UNMET appended
    from phanotate_amd.cli import format_evidence_scan

    ev = np.zeros(1, _lib.EVSCAN_DT)
    for name in _lib.EVSCAN_DT.names:
        ev[0][name] = rec[0][name]
    assert format_evidence_scan(["a"], status[:1], np.array([0, 1]), ev).splitlines()[2] + "\t0" == text.splitlines()[3]


def test_cli_refusals_of_curated_scan_need_no_device(tmp_path):
    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    ev = tmp_path / "ev.txt"
    ev.write_text("1\t9\t+\tc1\t-1.0\n")
    rq = tmp_path / "rq.txt"
    rq.write_text("1\t9\t+\tc1\n")
    out, re_out = tmp_path / "o.txt", tmp_path / "r.txt"
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    full = ["--require", str(rq), "--reannotation", str(re_out), "--curated-scan", str(ev), str(out)]
    for bad, word in ((full + ["-d"], b"--curated-scan: not allowed with argument -d/--dump"),
                      (full + ["--gpus", "2"], b"--curated-scan: not available with --gpus above 1"),
                      (["--curated-scan", str(ev), str(out)], b"--curated-scan: needs --require"),
                      (["--forbid", str(rq), "--reannotation", str(re_out), "--curated-scan", str(ev), str(out)], b"--curated-scan: needs --require"),
                      (["--require", str(rq), "--curated-scan", str(ev), str(out)], b"--require: needs --reannotation"),
                      (["--require", str(rq), "--reannotation", str(re_out), "--curated-scan", str(ev)], b"--curated-scan: expected 2 arguments")):
        r = subprocess.run(exe + bad, capture_output=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    r = subprocess.run(exe + full, capture_output=True, timeout=120, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and b"--curated-scan: not available under a multi-rank launch" in r.stderr
    assert not out.exists()


def test_cli_still_refuses_evidence_with_require(tmp_path):
    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    ev = tmp_path / "ev.txt"
    ev.write_text("1\t9\t+\tc1\t-1.0\n")
    rq = tmp_path / "rq.txt"
    rq.write_text("1\t9\t+\tc1\n")
    out, re_out = tmp_path / "o.txt", tmp_path / "r.txt"
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    for extra in ([], ["--curated-scan", str(ev), str(out)]):
        r = subprocess.run(exe + ["--evidence", str(ev), "--require", str(rq), "--reannotation", str(re_out)] + extra, capture_output=True, timeout=120)
        assert r.returncode == 2 and b"--evidence: not allowed with argument --require" in r.stderr, r.stderr[-500:]


# ---- the GPU test's one call of 45 scenarios, on the CPU oracle's graphs ----
def test_all_45_seeded_draws_settle(oracle):
    """tests/test_curate_scenarios_gpu.py hands the draws of curate_draws.mixes to the device as ONE call and asks status 0 of every
    scenario.  Here the yardstick alone — the same weights on the oracle's graph of the same contig — says that all 45 settle with a path
    (the count tests/test_curate_host.py prints for the same draws)."""
    import phanotate_amd as pa

    graphs = [cd.OracleGraph(oracle, s) for s in cd.mix_seqs(pa)]
    draws = ok = 0
    for row in cd.mixes(graphs):
        for g, d in zip(graphs, row):
            if d is None:
                continue
            draws += 1
            M = cd.big_m(g.edges, d)
            edges, pinned = cd.weights(g.edges, g.orf_edge, d, M)
            dist, par = settle(g.V, edges, g.src)
            ok += dist is not None and dist[g.tgt] is not None
    assert (draws, ok) == (45, 45)
