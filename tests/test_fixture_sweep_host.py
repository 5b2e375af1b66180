"""Host side of the fixture sweep (no GPU): which golden fixtures tests/test_fixture_sweep_gpu.py runs the newer re-annotation families on,
and — on the CPU oracle's graphs under each fixture's own parameters and tRNA hits — how the four solves of every draw end under
test_evidence_gpu.settle.  The GPU test hands the very same draws to the device and sets its floors by these counts."""
import pytest

from test_evidence_gpu import settle

import curate_draws as cd
import fixture_draws as fd

USABLE = ["edge_L1000", "edge_L200", "edge_L4001", "edge_L4002", "edge_bridge", "edge_bridge_left", "edge_iupac", "edge_nrun", "edge_upper",
          "param_16_starts", "param_codons", "param_minlen6", "param_minlen60", "param_minlen7", "param_minlen91", "param_minlen92",
          "param_negative_weight", "param_noatg", "param_one_stop", "param_repeated", "param_start_is_stop", "param_start_rc_stop",
          "param_stop_rc_stop", "param_weights_3_1", "param_zero_weight", "phiX174", "synth6k_100", "synth6k_101", "synth6k_102", "synth6k_103",
          "trna_gap", "trna_gap_left", "trna_phiX174", "trna_synth6k"]
TRNA = ["trna_gap", "trna_gap_left", "trna_phiX174", "trna_synth6k"]
BATCHED = USABLE[:9] + USABLE[25:]  # the default parameter set: one batch, each contig with its own hit list


@pytest.fixture(scope="module")
def sweep(oracle):
    return fd.usable(oracle)


def test_the_usable_and_the_degenerate_fixtures(oracle, sweep):
    assert [fx.case for fx, g in sweep] == USABLE
    assert [fx.case for fx, g in sweep if fx.trnas] == TRNA  # (trna_empty-like hit lists without a hit bring no node)
    assert [fx.case for fx, g in sweep if fd.default_params(fx)] == BATCHED
    assert len({tuple(sorted(fx.params.items())) for fx, g in sweep}) >= 15  # the parameter sets differ
    for fx, g in sweep:  # the oracle's graph read rightly under the fixture's parameters and hits: its own path's distance, its genes among the ORF edges
        dist, par = settle(g.V, g.edges, g.src)
        assert dist[g.tgt] == g.D and g.called <= set(g.orf_edge), fx.case
        assert (sum(abs(f) == 4 for f in g.frame) > 0) == bool(fx.trnas), fx.case  # tRNA nodes exactly where there are hits ...
        assert all(abs(g.frame[u]) <= 3 and abs(g.frame[v]) <= 3 for u, v in g.orf_edge.values())  # ... and none of them an ORF's
    deg = {fx.case: fx for fx in fd.degenerate()}
    assert sorted(deg) == ["edge_L5", "edge_L6", "edge_L80", "edge_badletter", "edge_huge", "param_minlen_gt_contig", "trna_duplicate"]
    status = {}
    for case, fx in deg.items():
        r = oracle.run(fx.seq, oracle.make_params(**fx.params), trnas=fx.trnas)
        status[case] = r["status"]
        assert not fx.graph(oracle).ok and (r["status"] != 0 or (len(r["node_type"]) == 2 and len(r["path"]) == 0)), case  # source and target only, or no graph
    assert status == dict(edge_L5=-3, edge_L6=0, edge_L80=0, edge_badletter=-2, edge_huge=-7, param_minlen_gt_contig=0, trna_duplicate=-6)
    assert not set(deg) & set(USABLE)


def test_how_the_draws_end_on_the_oracles_graphs(oracle, sweep):
    """Five seeded draws per fixture, four solves per draw.  Measured: mask and evidence 170 of 170 settle with a path; pin and full 153 settle
    with a path and 17 meet a negative cycle (a required ORF's edge on a cycle the source reaches), none is left without a path; the full
    solves keep 202 required ORFs.  Every fixture has at least 2 full draws that settle (param_codons has 2, param_start_rc_stop, synth6k_100
    and trna_synth6k 3).  On every tRNA fixture some settled solve's path holds a tRNA gene: on trna_gap and trna_gap_left every one, on
    trna_phiX174 and trna_synth6k — whose run calls none — the pin and full solves of one seeded draw each.

    The directed draws of the four tRNA fixtures (counted apart): all 16 solves settle with a path, each pin and full solve keeps its one
    required ORF.  trna_gap: (1836, 3011, +) refused, (1878, 3011, +) required, the bonus on (1938, 3011, +) — the starts of the refused
    gene's own stop, left of the four tRNA genes, which stay on the path.  trna_gap_left: (911, 1186, +) refused, (922, 1023, -) required,
    (924, 1337, +) biased; the three tRNA genes stay.  trna_phiX174 (leftmost hit 30..104, covered by the called 100..627): that gene
    refused, (9, 101, -) required, (55, 627, +) biased; the mask and evidence solves call the tRNA gene 30..104, the pin and full solves do
    not.  trna_synth6k (hit 2500..2572 inside the called 1307..3331): that gene refused, its starts at 1298 required and 1397 biased; no
    tRNA gene is called."""
    tot = {k: dict(draws=0, ok=0, cycle=0, nopath=0, kept=0) for k in fd.KINDS}
    per_fixture, with_trna, directed = {}, {}, {}
    for fx, g in sweep:
        ds = fd.draws(oracle, fx, g)
        assert len(ds) == cd.ROUNDS + bool(fx.trnas)
        for j, d in enumerate(ds):
            assert not set(d["require"]) & set(d["forbid"]) and not set(d["require"]) & g.called and set(d["bias"]) <= set(g.orf_edge)
            for kind in fd.KINDS:
                what, kept, trna = fd.oracle_outcome(g, d, kind, settle)
                with_trna[fx.case] = with_trna.get(fx.case, 0) + (trna > 0)
                if j >= cd.ROUNDS:
                    directed.setdefault(fx.case, []).append((kind, what, kept, trna))
                    continue
                t = tot[kind]
                t["draws"] += 1
                t[what] += 1
                t["kept"] += kept
                if kind == "full":
                    per_fixture[fx.case] = per_fixture.get(fx.case, 0) + (what == "ok")
    print("fixture draws on the oracle's graphs:", tot)
    print("full draws that settle, per fixture:", per_fixture)
    print("directed draws:", directed)
    assert tot["mask"] == dict(draws=170, ok=170, cycle=0, nopath=0, kept=0)
    assert tot["evidence"] == dict(draws=170, ok=170, cycle=0, nopath=0, kept=0)
    assert tot["pin"] == dict(draws=170, ok=153, cycle=17, nopath=0, kept=202)
    assert tot["full"] == dict(draws=170, ok=153, cycle=17, nopath=0, kept=202)
    assert min(per_fixture.values()) == 2 and [c for c, n in per_fixture.items() if n == 2] == ["param_codons"]
    assert all(with_trna[c] > 0 for c in TRNA) and all(with_trna[fx.case] == 0 for fx, g in sweep if not fx.trnas)
    assert sorted(directed) == TRNA
    n4 = {"trna_gap": (4, 4), "trna_gap_left": (3, 3), "trna_phiX174": (1, 0), "trna_synth6k": (0, 0)}  # tRNA genes called: (mask / evidence, pin / full)
    for case, rows in directed.items():
        assert rows == [("mask", "ok", 0, n4[case][0]), ("evidence", "ok", 0, n4[case][0]), ("pin", "ok", 1, n4[case][1]), ("full", "ok", 1, n4[case][1])], (case, rows)
