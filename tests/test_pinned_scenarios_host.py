"""Pinned scenario batches (phx_pinned_scenarios_flat), the parts that need no device: the layout arithmetic of a pinned
slot restated in plain Python, the triple -> arrays builder, the --alt-starts formatter and its argument refusals, and the new entry
points of the header, the binding and the Annotator."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


# ---- a pinned slot's slices ----
# The host lays a chunk's slots out in scenario order (scen_compute).  Every slot has a refused slice of
# ((edge_off & 31) + n_edge) / 32 + 2 words at mask0; a pinned slot has a required slice of the same size at req0 in the region behind
# all refused slices.  k_scp_mask sets in-edge slot e as bit (edge_off & 31) + e of the required slice; the solver reads bit
# edge_off + e of a pointer moved back by edge_off >> 5 words (scp_req, sc_view's rule).  A slot's distances are n_node x NL words, a
# pinned slot's n_node x (NL + 1), each rounded up to an even count so that every slice starts on 16 bytes.

def slice_words(edge_off, n_edge):
    return ((edge_off & 31) + n_edge) // 32 + 2


def dist_words(n_node, nl, pinned):
    return (n_node * (nl + (1 if pinned else 0)) + 1) & ~1


def writer_bit(base0, edge_off, e):  # k_sc_mask / k_scp_mask
    lo = edge_off & 31
    return base0 + ((lo + e) >> 5), (lo + e) & 31


def reader_bit(base0, edge_off, e):  # rs_refused / rs_required / inorder_contig behind sc_view and scp_req
    base = base0 - (edge_off >> 5)
    x = edge_off + e
    return base + (x >> 5), x & 31


def lay_out(slots, contigs):
    """slots: [(contig, pinned)]; contigs: [(edge_off, n_edge, n_node, nl)] -> per slot (dist0, mask0, req0 or None), totals."""
    words = mwords = rwords = 0
    out = []
    for c, pinned in slots:
        edge_off, n_edge, n_node, nl = contigs[c]
        out.append((words, mwords, rwords if pinned else None))
        words += dist_words(n_node, nl, pinned)
        mwords += slice_words(edge_off, n_edge)
        if pinned:
            rwords += slice_words(edge_off, n_edge)
    return out, words, mwords, rwords


def test_a_pinned_slots_slices_keep_edge_off_modulo_32_and_neighbours_never_overlap():
    rng = np.random.RandomState(18)
    for _ in range(300):
        n_contig = rng.randint(1, 6)
        n_edge = [int(rng.choice([1, 2, 31, 32, 33, 63, 64, 65, rng.randint(1, 5000)])) for _ in range(n_contig)]
        edge_off = np.concatenate([[0], np.cumsum(n_edge)]).tolist()
        contigs = [(edge_off[c], n_edge[c], int(rng.randint(3, 400)), int(rng.choice([2, 4, 8, 17]))) for c in range(n_contig)]
        slots = [(int(rng.randint(n_contig)), bool(rng.randint(2))) for _ in range(rng.randint(1, 12))]
        lay, words, mwords, rwords = lay_out(slots, contigs)
        req_base = mwords + 2  # the required slices follow the refused ones in one buffer
        owner, spans = {}, []
        for s, (c, pinned) in enumerate(slots):
            eo, ne, V, nl = contigs[c]
            dist0, mask0, req0 = lay[s]
            assert dist0 % 2 == 0
            need = V * (nl + 1 if pinned else nl)
            assert need <= dist_words(V, nl, pinned) <= need + 1 and dist_words(V, nl, pinned) % 2 == 0
            spans.append((dist0, dist0 + need))  # the last word the sweep writes: node V - 1, limb NL (+ 1) - 1
            for kind, base0 in (("F", mask0),) + ((("R", req_base + req0),) if pinned else ()):
                for e in sorted({0, 1, ne // 2, ne - 1} | set(rng.randint(0, ne, 8).tolist())):
                    w = writer_bit(base0, eo, e)
                    assert w == reader_bit(base0, eo, e), (eo, e)
                    assert base0 <= w[0] < base0 + slice_words(eo, ne)
                    assert owner.setdefault(w, (s, kind, e)) == (s, kind, e)  # no two (slot, slice, edge) share a bit
            if pinned:
                assert req_base + req0 + slice_words(eo, ne) <= mwords + 2 + rwords + 2  # inside the buffer the host allocates and clears
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a1 <= b0  # neighbouring slots' distances never overlap, whatever their widths
        assert spans[-1][1] <= words


def test_pinned_dist_words_reach_odd_counts_and_are_rounded_to_even():
    assert dist_words(5, 2, True) == 16 and dist_words(5, 2, False) == 10  # 15 words of 3 limbs -> 16
    assert dist_words(4, 2, True) == 12 and dist_words(3, 4, True) == 16 and dist_words(3, 8, True) == 28 and dist_words(3, 17, True) == 54
    # the slot-byte accounting grows by one limb per node and a second slice
    V, E, nl = 1001, 7777, 2
    plain = V * (nl * 8 + 4 + 4) + (E // 32 + 3) * 4
    pinned = plain + V * 8 + (E // 32 + 3) * 4 + 16
    assert pinned - plain >= V * 8 + E // 8


# ---- Annotator.pinned_scenarios' argument handling ----

def test_pinned_scenario_arrays_and_their_errors():
    from phanotate_amd.api import Annotator

    oo = np.array([0, 10, 10, 25], np.int64)  # contig 1 has no ORFs
    contig, foff, forf, roff, rorf = Annotator._pinned_scenario_arrays([(0, [3, 3, 9], None), (2, [], [14]), (2, None, np.array([0, 14, 14])), (1, None, None)], 3, oo)
    assert contig[:4].tolist() == [0, 2, 2, 1]
    assert foff.tolist() == [0, 3, 3, 3, 3] and forf[:3].tolist() == [3, 3, 9]
    assert roff.tolist() == [0, 0, 1, 4, 4] and rorf[:4].tolist() == [14, 0, 14, 14]
    assert forf.dtype == np.int32 and rorf.dtype == np.int32 and foff.dtype == np.int64 and roff.dtype == np.int64
    contig, foff, forf, roff, rorf = Annotator._pinned_scenario_arrays([], 3, oo)
    assert foff.tolist() == [0] and roff.tolist() == [0] and len(forf) >= 1 and len(rorf) >= 1
    for bad in ([(3, [], [])], [(-1, None, None)], [(0, [10], None)], [(0, None, [10])], [(0, None, [-1])], [(1, None, [0])], [(2, [15], [0])]):
        with pytest.raises(IndexError):
            Annotator._pinned_scenario_arrays(bad, 3, oo)
    for bad in ([5], [(0, [1])], [(0, [1], [2], [3])]):
        with pytest.raises(ValueError):
            Annotator._pinned_scenario_arrays(bad, 3, oo)


# ---- --alt-starts ----

def test_alt_starts_formatter_on_hand_made_records():
    from phanotate_amd import _lib
    from phanotate_amd.cli import format_alt_starts

    assert _lib.ALT_DT.names == ("left", "right", "strand", "orf", "alt", "alt_left", "alt_right", "status", "delta", "unmet", "n_removed", "n_added")
    rec = np.zeros(6, _lib.ALT_DT)
    rec[0] = (100, 402, 1, 7, 8, 130, 402, 0, 1.25, 0, 1, 1)               # forward: the alternative starts at 130
    rec[1] = (500, 900, -1, 11, 12, 500, 870, 0, 0.30000000000000004, 0, 2, 3)  # reverse: START is the right end
    rec[2] = (1000, 1300, 1, 20, 21, 1060, 1300, -9, np.inf, 1, 9, 0)      # the alternative's edge lies on a cycle
    rec[3] = (1000, 1300, 1, 20, 22, 1090, 1300, 0, 0.0, 1, 0, 0)          # the alternative cannot be called
    rec[4] = (1000, 1300, 1, 20, 23, 1120, 1300, 1, np.inf, 1, 9, 0)       # unmet goes before no path
    rec[5] = (50, 200, -1, 2, 3, 50, 170, 1, np.inf, 0, 4, 0)              # no path
    status = np.array([0, -2, 0], np.int32)
    offsets = np.array([0, 5, 5, 6], np.int64)
    text = format_alt_starts(["a", "bad", "c"], status, offsets, rec)
    head = "#START\tSTOP\tFRAME\tALT\tDELTA\tREMOVED\tADDED"
    assert text.splitlines() == [
        "#id:\ta", head,
        "100\t402\t+\t130\t1.25\t1\t1",
        "900\t500\t-\t870\t0.30000000000000004\t2\t3",
        "1000\t1300\t+\t1060\tcycle\t9\t0",
        "1000\t1300\t+\t1090\tunmet\t0\t0",
        "1000\t1300\t+\t1120\tunmet\t9\t0",
        "#id:\tc", head,
        "200\t50\t-\t170\tinf\t4\t0",
    ]
    assert format_alt_starts([], np.zeros(0, np.int32), np.zeros(1, np.int64), rec[:0]) == ""
    for ln in text.splitlines()[2:4]:  # repr(delta) reads back to the same double
        assert repr(float(ln.split("\t")[4])) == ln.split("\t")[4]


def test_cli_refusals_of_alt_starts_need_no_device(tmp_path):
    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    out = tmp_path / "o.txt"
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    for bad, word in ((["--alt-starts", str(out), "-d"], b"--alt-starts: not allowed with argument -d/--dump"),
                      (["--alt-starts", str(out), "--gpus", "2"], b"--alt-starts: not available with --gpus above 1")):
        r = subprocess.run(exe + bad, capture_output=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    r = subprocess.run(exe + ["--alt-starts", str(out)], capture_output=True, timeout=120, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and b"--alt-starts: not available under a multi-rank launch" in r.stderr
    assert not out.exists()


# ---- the entry points ----

def test_header_exports_and_annotator_methods():
    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    m = re.search(r"int phx_pinned_scenarios_flat\(([^;]*)\);", text)
    assert m is not None
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "n_scen", "scen_contig", "forbid_off", "forbid_orf", "require_off", "require_orf", "orf_offsets", "flags", "genes",
                                                        "cap", "offsets", "status", "delta", "unmet", "total"]
    assert re.search(r"#define PHX_VERSION 410\b", text)  # (callers probe for the symbol)
    assert "no required ORFs per scenario" not in text
    assert "phx_pinned_scenarios_flat" in _lib.EXPORTS
    L = _lib.lib()
    assert len(L.phx_pinned_scenarios_flat.argtypes) == 16 and len(L.phx_scenarios_flat.argtypes) == 13
    # argument errors come before any device work: without a context, PHX_E_ARG
    assert L.phx_pinned_scenarios_flat(None, 0, None, None, None, None, None, None, 0, None, 0, None, None, None, None, None) == -1
    for name in ("pinned_scenarios", "alt_starts", "scenarios", "scenario_path", "scenarios_ms", "scenario_chunks"):
        assert callable(getattr(api.Annotator, name)), name
