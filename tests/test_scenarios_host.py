"""Scenario batches (phx_scenarios_flat), the parts that need no device: the arithmetic of the slots' bitmap slices and
of the tap-order -> device-order permutation restated in plain Python, the --start-drops formatter and its argument refusals, and the
new entry points of the header, the binding and the Annotator."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


# ---- the slots' bitmap slices ----
# The host lays the slices of a chunk out one after the other (scen_compute): slot s of a contig with `edge_off`, `n_edge` starts at word
# mask0[s] and holds ((edge_off & 31) + n_edge) / 32 + 2 words.  k_sc_mask sets in-edge slot e as bit (edge_off & 31) + e of the slice;
# the shared solver code reads bit edge_off + e of a pointer moved back by edge_off >> 5 words (sc_view).  Both must name the same bit,
# inside the slot's own slice.

def slice_words(edge_off, n_edge):
    return ((edge_off & 31) + n_edge) // 32 + 2


def writer_bit(mask0, edge_off, e):  # k_sc_mask
    lo = edge_off & 31
    return mask0 + ((lo + e) >> 5), (lo + e) & 31


def reader_bit(mask0, edge_off, e):  # rs_refused / inorder_contig behind sc_view
    base = mask0 - (edge_off >> 5)
    x = edge_off + e
    return base + (x >> 5), x & 31


def test_a_slots_bitmap_slice_keeps_edge_off_modulo_32_and_stays_its_own():
    rng = np.random.RandomState(17)
    for _ in range(300):
        n_contig = rng.randint(1, 6)
        n_edge = [int(rng.choice([1, 2, 31, 32, 33, 63, 64, 65, rng.randint(1, 5000)])) for _ in range(n_contig)]
        edge_off = np.concatenate([[0], np.cumsum(n_edge)]).tolist()  # the batch's edges are packed: any value modulo 32 occurs
        slots = rng.randint(0, n_contig, rng.randint(1, 12)).tolist()
        mask0, acc = [], 0
        for c in slots:
            mask0.append(acc)
            acc += slice_words(edge_off[c], n_edge[c])
        owner = {}
        for s, c in enumerate(slots):
            for e in sorted({0, 1, n_edge[c] // 2, n_edge[c] - 1} | set(rng.randint(0, n_edge[c], 8).tolist())):
                w = writer_bit(mask0[s], edge_off[c], e)
                assert w == reader_bit(mask0[s], edge_off[c], e), (edge_off[c], e)
                assert mask0[s] <= w[0] < mask0[s] + slice_words(edge_off[c], n_edge[c])
                assert owner.setdefault(w, (s, e)) == (s, e)  # no two (slot, edge) pairs share a bit
        assert acc == sum(slice_words(edge_off[c], n_edge[c]) for c in slots)


def test_bit_positions_at_a_word_boundary():
    # edge_off = 95 (word 2, bit 31): edge 0 is the last bit of the slice's first word, edge 1 the first of the next
    assert writer_bit(10, 95, 0) == (10, 31) and writer_bit(10, 95, 1) == (11, 0)
    assert reader_bit(10, 95, 0) == (10, 31) and reader_bit(10, 95, 1) == (11, 0)
    assert slice_words(95, 1) == 3 and slice_words(0, 32) == 3 and slice_words(31, 33) == 4


# ---- tap order -> device ORF order ----
# phx_tap_orfs lists a contig's ORFs group by group in ascending DGrp.evkey; on the device a group's ORFs are contiguous from
# orf_begin.  A scenario's indices are tap indices: index t of the k-th group in tap order (first ORF at tap position p_k) is device ORF
# orf_begin + (t - p_k).

def tap_to_device(groups):
    """groups: [(evkey, orf_begin, n)] in device order -> list: tap index -> device index."""
    perm = []
    for _, begin, n in sorted(groups, key=lambda g: g[0]):
        perm.extend(range(begin, begin + n))
    return perm


def test_the_permutation_is_the_inverse_of_the_taps_order():
    rng = np.random.RandomState(5)
    for _ in range(100):
        sizes = rng.randint(1, 6, rng.randint(1, 40)).tolist()
        begins = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        keys = rng.permutation(len(sizes)).tolist()
        groups = [(keys[g], begins[g], sizes[g]) for g in range(len(sizes))]
        perm = tap_to_device(groups)
        assert sorted(perm) == list(range(begins[-1]))  # a permutation of the contig's ORFs
        # what the tap does: device ORFs listed group by group in key order
        tap = [d for g in sorted(range(len(sizes)), key=lambda g: keys[g]) for d in range(begins[g], begins[g] + sizes[g])]
        assert all(tap[t] == perm[t] for t in range(len(perm)))


# ---- Annotator.scenarios' argument handling ----

def test_scenario_arrays_and_their_index_errors():
    from phanotate_amd.api import Annotator

    oo = np.array([0, 10, 10, 25], np.int64)  # contig 1 has no ORFs
    contig, off, orf = Annotator._scenario_arrays([(0, [3, 3, 9]), (2, []), (2, np.array([14])), (1, None)], 3, oo)
    assert contig[:4].tolist() == [0, 2, 2, 1] and off.tolist() == [0, 3, 3, 4, 4] and orf[:4].tolist() == [3, 3, 9, 14]
    contig, off, orf = Annotator._scenario_arrays([], 3, oo)
    assert off.tolist() == [0] and len(orf) >= 1
    for bad in ([(3, [])], [(-1, [])], [(0, [10])], [(0, [-1])], [(1, [0])], [(2, [15])]):
        with pytest.raises(IndexError):
            Annotator._scenario_arrays(bad, 3, oo)
    with pytest.raises(ValueError):
        Annotator._scenario_arrays([5], 3, oo)


# ---- --start-drops ----

def test_start_drops_formatter_on_hand_made_records():
    from phanotate_amd import _lib
    from phanotate_amd.cli import format_start_drops

    rec = np.zeros(4, _lib.START_DT)
    rec[0] = (100, 402, 1, 7, 1.25, 9, 0, 130, 402)        # forward: restarted at 130, same stop
    rec[1] = (500, 900, -1, 11, 0.0, 12, 0, 500, 870)      # reverse: START is the right end
    rec[2] = (1000, 1300, 1, 20, np.inf, -1, 1, 0, 0)      # no path remains
    rec[3] = (50, 200, -1, 2, 3.0000000000000004, -1, 0, 0, 0)
    status = np.array([0, -2, 0], np.int32)
    offsets = np.array([0, 3, 3, 4], np.int64)
    text = format_start_drops(["a", "bad", "c"], status, offsets, rec)
    assert text.splitlines() == [
        "#id:\ta", "#START\tSTOP\tFRAME\tDROP\tRESTART",
        "100\t402\t+\t1.25\t130\t402",
        "900\t500\t-\t0.0\t870\t500",
        "1000\t1300\t+\tinf\t-",
        "#id:\tc", "#START\tSTOP\tFRAME\tDROP\tRESTART",
        "200\t50\t-\t3.0000000000000004\t-",
    ]
    assert format_start_drops([], np.zeros(0, np.int32), np.zeros(1, np.int64), rec[:0]) == ""
    for ln in text.splitlines():  # repr(drop) reads back to the same double
        if not ln.startswith("#"):
            assert repr(float(ln.split("\t")[3])) == ln.split("\t")[3]


def test_cli_refusals_of_start_drops_need_no_device(tmp_path):
    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    out = tmp_path / "o.txt"
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    for bad, word in ((["--start-drops", str(out), "-d"], b"--start-drops: not allowed with argument -d/--dump"),
                      (["--start-drops", str(out), "--gpus", "2"], b"--start-drops: not available with --gpus above 1")):
        r = subprocess.run(exe + bad, capture_output=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    r = subprocess.run(exe + ["--start-drops", str(out)], capture_output=True, timeout=120, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and b"--start-drops: not available under a multi-rank launch" in r.stderr
    assert not out.exists()


# ---- the entry points ----

def test_header_exports_and_annotator_methods():
    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    m = re.search(r"int phx_scenarios_flat\(([^;]*)\);", text)
    assert m is not None
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "n_scen", "scen_contig", "scen_off", "scen_orf", "orf_offsets", "flags", "genes", "cap", "offsets", "status",
                                                        "delta", "total"]
    assert re.search(r"#define PHX_VERSION 410\b", text)  # (callers probe for the symbol)
    for name in ("phx_scenarios_flat", "phx_scenarios_ms", "phx_scenario_chunks", "phx_tap_scenario_path"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, text), name
    L = _lib.lib()
    assert len(L.phx_scenarios_flat.argtypes) == 13
    # argument errors come before any device work: without a context, and without the arrays, PHX_E_ARG
    assert L.phx_scenarios_flat(None, 0, None, None, None, None, 0, None, 0, None, None, None, None) == -1
    assert L.phx_scenarios_ms(None, None) == -1
    assert L.phx_scenario_chunks(None) == -1
    assert L.phx_tap_scenario_path(None, 0, None, 0, None, None, 0) == -1
    for name in ("scenarios", "scenarios_ms", "scenario_chunks", "scenario_path", "start_drops"):
        assert callable(getattr(api.Annotator, name)), name
    assert _lib.START_DT.names[:7] == ("left", "right", "strand", "orf", "drop", "restart", "status")
