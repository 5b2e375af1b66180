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
REMOVED = ["trna_phiX174"]  # the tRNA fixtures with a second directed draw (fixture_draws.directed_removed)
SECOND_DROPS = ((2, 2, 14, 14, 2, 3), (1, 1, 2, 2))  # its drops: (solves, P' != P, records, bypass, tRNA pairs, tRNA splices), (records / tRNA genes removed, ... added)
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


def drop_counts(rows):
    """Of one solve's fd.drop_outcome rows: records, with bypass, with a drop of 0, tRNA pairs without a record, records whose removed /
    added / removed + added genes hold a tRNA gene, the tRNA genes on either side, records with more than one removed gene."""
    c = dict(records=0, bypass=0, zero=0, trna_pairs=0, trna_removed=0, trna_added=0, trna_splice=0, removed_genes=0, added_genes=0, multi=0)
    for r in rows:
        if r[0] == "trna":
            c["trna_pairs"] += 1
            continue
        nr, na = sum(abs(x[3]) == 4 for x in r[4]), sum(abs(x[3]) == 4 for x in r[5])
        assert r[0] == "cds" and abs(r[1][3]) <= 3 and (not r[2] or r[1] in r[4])  # the dropped gene is among the removed ones
        for key, x in (("records", 1), ("bypass", r[2]), ("zero", r[3] == 0), ("trna_removed", nr > 0), ("trna_added", na > 0), ("trna_splice", nr + na > 0),
                       ("removed_genes", nr), ("added_genes", na), ("multi", len(r[4]) > 1)):
            c[key] += int(x)
    return c


def test_how_the_drops_end_on_the_oracles_graphs(oracle, sweep):
    """redrops() and rereplacements() on the CPU: after the mask and the evidence solve of every draw, each CDS gene of P' is dropped by
    taking its stop node out of the oracle's graph (fixture_draws.drop_outcome, under test_evidence_gpu.settle).  Measured, and asserted
    to the unit:

                               solves  P' != P  records  with bypass  tRNA pairs on P'  records with a tRNA gene among removed + added
        mask, seeded              170       78     1080         1080                35                                             20
        evidence, seeded          170       86     1074         1074                35                                             20
        directed (both kinds)       8        8       64           64                16                                              6
        second directed (both)      2        2       14           14                 2                                              3

    No drop is 0.  Per tRNA fixture, its seeded and first directed draws (records / tRNA pairs without a record / records with a tRNA gene
    in the splice): trna_gap 84 / 48 / 0, trna_gap_left 92 / 36 / 0, trna_phiX174 84 / 2 / 22, trna_synth6k 114 / 0 / 24.  Every one of
    those 46 splices has its tRNA gene on the added side (46 tRNA genes, one per record) and none on the removed side: on the two gap
    fixtures no ORF lies over a hit, and where a seeded draw brings a tRNA gene in, it comes by the detour.  Records with more than one
    removed gene: 286 (mask), 278 (evidence), 22 (directed).  The second directed draw of trna_phiX174 (fixture_draws.directed_removed)
    reaches the removed side: (100, 627, +) refused, a bonus of 39159 units — its margin under that mask less one — on (9, 101, -), so
    that P' keeps the tRNA gene 30..104; without the next gene (283, 627, +) the best path calls (9, 101, -) and the tRNA gene goes:
    one record of the evidence solve with a tRNA gene on the removed side.  (The mask solve of that draw is the first directed draw's;
    in both solves the last record's detour brings the tRNA gene 5290..5370 in: two records with one on the added side.)  No other tRNA
    fixture has such a draw: on the gap fixtures no ORF lies over a called tRNA gene, and trna_synth6k's mask calls none."""
    kinds = ("mask", "evidence")
    zero = drop_counts([])
    tot = {k: dict(zero, solves=0, moved=0) for k in kinds + ("directed", "second")}
    per = {c: dict(zero) for c in TRNA}
    fewest = {}
    for fx, g in sweep:
        ds, extra = fd.draws(oracle, fx, g), fd.removed_draw(oracle, fx, g)
        assert (extra is not None) == (fx.case in REMOVED)
        for j, d in enumerate(ds + [extra] * (extra is not None)):
            for kind in kinds:
                moved, rows = fd.drop_outcome(g, d, kind, settle)
                c = drop_counts(rows)
                t = tot[kind if j < cd.ROUNDS else "directed" if j == cd.ROUNDS else "second"]
                t["solves"] += 1
                t["moved"] += moved
                for key, x in c.items():
                    t[key] += x
                    if fx.case in per and j <= cd.ROUNDS:
                        per[fx.case][key] += x
                if j < cd.ROUNDS:
                    fewest[fx.case] = fewest.get(fx.case, 0) + c["records"]
    print("drops on the oracle's graphs:", tot)
    print("per tRNA fixture:", per)
    row = lambda t: (t["solves"], t["moved"], t["records"], t["bypass"], t["trna_pairs"], t["trna_splice"])
    assert row(tot["mask"]) == (170, 78, 1080, 1080, 35, 20)
    assert row(tot["evidence"]) == (170, 86, 1074, 1074, 35, 20)
    assert row(tot["directed"]) == (8, 8, 64, 64, 16, 6)
    assert all(t["zero"] == 0 for t in tot.values())
    assert {c: (p["records"], p["trna_pairs"], p["trna_splice"]) for c, p in per.items()} == dict(trna_gap=(84, 48, 0), trna_gap_left=(92, 36, 0), trna_phiX174=(84, 2, 22), trna_synth6k=(114, 0, 24))
    assert min(fewest.values()) == 10 and max(fewest.values()) == 120 and fewest["param_stop_rc_stop"] == 10 and fewest["synth6k_102"] == 120
    # measured when this test was written: the side of the tRNA genes, and the records that remove more than their own gene
    side = lambda t: (t["trna_removed"], t["removed_genes"], t["trna_added"], t["added_genes"])
    assert side(tot["mask"]) == (0, 0, 20, 20) and side(tot["evidence"]) == (0, 0, 20, 20) and side(tot["directed"]) == (0, 0, 6, 6)
    assert (tot["mask"]["multi"], tot["evidence"]["multi"], tot["directed"]["multi"]) == (286, 278, 22)
    assert all(p["trna_removed"] == 0 for p in per.values())  # ... hence the second directed draw
    assert row(tot["second"]) == SECOND_DROPS[0] and side(tot["second"]) == SECOND_DROPS[1], tot["second"]
