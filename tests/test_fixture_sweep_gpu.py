"""The newer re-annotation families on the golden fixtures, on the device: evidence(), curate(), scenarios(), pinned_scenarios(),
evidence_scenarios(), remargins() / redist(), pinmargins() / pindist(), redrops(), rereplacements() / rereplacement_path(), start_drops(),
alt_starts() and evidence_scan() on graphs with tRNA nodes, IUPAC letters, bridged runs and under the fixtures' own codon sets, weights and
minlen.  Each usable fixture (tests/fixture_draws.py) is one context and one run; its draws are the ones tests/test_fixture_sweep_host.py
counts on the CPU oracle's graphs.  The yardsticks are the existing ones, over the device's own tapped edges: CuRef / check of
tests/test_curate_gpu.py, pin_ref / check_pin of tests/test_pinmargins_gpu.py, EvRef / check_contig (py_dt_in_R) of
tests/test_remargins_gpu.py, check_contig of tests/test_redrops_gpu.py and check_records of tests/test_rereplace_gpu.py — the last two on
every record of every mask and evidence solve, without sampling.  Every comparison is integer-exact or byte for byte."""
import numpy as np
import pytest

from test_constrain_gpu import gene_tuples, run_batch
from test_curate_gpu import CuRef, DeviceGraph, check, contig_bytes, curate, evidence
from test_evidence_gpu import NEGCYCLE, EvRef, score
from test_fixture_sweep_host import BATCHED, REMOVED, TRNA, USABLE
from test_pinmargins_gpu import check_pin
from test_remargins_gpu import check_contig

import fixture_draws as fd
import test_redrops_gpu as rd
import test_rereplace_gpu as rr

pytestmark = pytest.mark.gpu

S_NEGCYCLE, S_NOPATH = -9, 1
DEGENERATE = dict(edge_L5=-3, edge_L6=0, edge_L80=0, edge_badletter=-2, edge_huge=-7, param_minlen_gt_contig=0, trna_duplicate=-6)  # the run's status


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


class Yard(CuRef):
    """CuRef that solves each (refused, required, biased) triple once: the scenario and derived batches ask for the solves of the single
    calls again.  Nothing changes a solve it has handed out."""

    def __init__(self, ann, i):
        super().__init__(ann, i)
        self.memo = {}

    def solve(self, forbid=(), require=(), bias=None):
        key = (tuple(forbid), tuple(require), tuple(sorted((bias or {}).items())))
        if key not in self.memo:
            self.memo[key] = super().solve(forbid, require, bias)
        return self.memo[key]


def outcome(sol):
    return "cycle" if sol["cycle"] else "nopath" if sol["S"] is None else "ok"


def indexed(ref, d):
    """A draw by ORF index on this contig: (forbid, require, {ORF: B})."""
    by = ref.by_ends
    return [by[k] for k in d["forbid"]], [by[k] for k in d["require"]], {by[k]: B for k, B in d["bias"].items()}


def margin_bytes(out, i):
    """(status, record bytes, lost bytes) of contig i from remargins() or pinmargins()."""
    st, offs, rec = out[:3]
    return int(st[i]), rec[offs[i]:offs[i + 1]].tobytes(), out[3][offs[i]:offs[i + 1]].tobytes() if len(out) > 3 else b""


def scenario_bytes(ann, res, j, contig):
    """contig_bytes of scenario j."""
    st, offs, genes, delta = res[:4]
    p, S = ann.scenario_path(j, contig)
    return int(st[j]), genes[offs[j]:offs[j + 1]].tobytes(), delta[j].tobytes(), int(res[4][j]) if len(res) > 4 else 0, p.tobytes(), S


def check_scenario(ann, res, j, contig, sol, nreq, D):
    """Scenario j against the yardstick's solve, as test_curate_gpu.check holds a single call against it."""
    st, offs, genes, delta = res[:4]
    unmet = int(res[4][j]) if len(res) > 4 else 0
    g = genes[offs[j]:offs[j + 1]]
    path, S = ann.scenario_path(j, contig)
    if sol["cycle"] or sol["S"] is None:
        assert st[j] == (S_NEGCYCLE if sol["cycle"] else S_NOPATH) and delta[j] == np.inf and len(g) == 0 and unmet == nreq and len(path) == 0, (j, int(st[j]), unmet)
        return
    assert st[j] == 0, (j, int(st[j]))
    assert S == sol["S"] and path.tolist() == sol["path"], (j, S, sol["S"])
    assert gene_tuples(g) == sol["genes"], j
    assert float(delta[j]) == float(sol["S"] - D) / 1000.0 and unmet == nreq - sol["count"], (j, float(delta[j]), unmet)


def check_record(sol, nreq, status, delta, unmet, genes, D, what):
    """One record of a derived batch (its scenario's status, delta, unmet and genes) against the yardstick's solve."""
    if sol["cycle"] or sol["S"] is None:
        assert status == (S_NEGCYCLE if sol["cycle"] else S_NOPATH) and delta == np.inf and unmet == nreq and len(genes) == 0, (what, int(status))
        return
    assert status == 0 and float(delta) == float(sol["S"] - D) / 1000.0 and unmet == nreq - sol["count"], (what, int(status), float(delta), sol["S"] - D)
    assert gene_tuples(genes) == sol["genes"], what


class Lone:
    """What one fixture's sweep leaves for the batch test and the floors."""

    def __init__(self):
        self.count = {k: dict(ok=0, cycle=0, nopath=0, kept=0) for k in fd.KINDS}
        self.with_trna = 0  # checked solves whose path holds a tRNA gene
        self.single = {}  # (kind, draw) -> (contig_bytes, margin_bytes)
        self.drops = {}  # ("mask" | "evidence", draw) -> check_drops' counts
        self.drop_bytes = {}  # ("mask" | "evidence", draw) -> drop_bytes
        self.refused = 0  # pin and full solves after which redrops() and rereplacements() raised PHX_E_STATE
        self.draws = []


def drop_bytes(ann, dr, rp, i):
    """Contig i of redrops() and rereplacements(): the records' bytes of both and every record's witness path."""
    return rd.out_bytes(dr, i), rr.contig_bytes(rp, i), [ann.rereplacement_path(i, k).tobytes() for k in range(int(rp[1][i + 1] - rp[1][i]))]


def check_drops(ann, ev, F, bias, genes, j):
    """redrops() and rereplacements() of the lone contig's resident mask or evidence solve — the drops first on an even draw, the
    replacements first on an odd one, where they build the trees themselves.  Every field of every drop record against
    test_redrops_gpu.check_contig (drop: the yardstick's solve with the gene's stop group refused on top, integer-exact), every
    replacement record, its witness path and its genes against test_rereplace_gpu.check_records without sampling.  Returns the counts
    the floors read and drop_bytes."""
    calls = (ann.redrops, ann.rereplacements)
    got = [call() for call in (calls if j % 2 == 0 else calls[::-1])]
    dr, rp = got if j % 2 == 0 else got[::-1]
    assert rp[0].tobytes() == dr[0].tobytes() and rp[1].tobytes() == dr[1].tobytes() and dr[1].tolist() == [0, len(dr[2])] and len(rp[2]) == len(dr[2])
    res = rd.check_contig(ann, ev, F, bias, int(dr[0][0]), dr[2], genes)
    c = dict(status=int(dr[0][0]), records=len(dr[2]), compared=0, bypass=0, exact=0, trna_pairs=0, removed=0, added=0, splice=0)
    if res not in (NEGCYCLE, None):
        c["compared"], path = res[1], res[2]
        c["trna_pairs"] = sum(abs(int(ev.frame[path[2 * k + 1]])) > 3 for k in range((len(path) - 1) // 2))
        c["exact"], c["bypass"] = rr.check_records(ann, ev, F, bias, dr[2], rp[2], rp[3])
        assert c["trna_pairs"] + c["compared"] == (len(path) - 1) // 2  # every pair of P' is a record or a tRNA pair
        for r in rp[2]:
            g = rp[3][int(r["gene_off"]): int(r["gene_off"]) + int(r["n_removed"]) + int(r["n_added"])]["frame"]
            nr, na = int((np.abs(g[:int(r["n_removed"])]) == 4).sum()), int((np.abs(g[int(r["n_removed"]):]) == 4).sum())
            c["removed"] += nr > 0
            c["added"] += na > 0
            c["splice"] += nr + na > 0
    else:
        assert len(rp[2]) == len(rp[3]) == 0
    return c, drop_bytes(ann, dr, rp, 0)


DONE = {}


def sweep(pa, oracle, case):
    """The whole sweep of one fixture, once per session: the per-fixture case runs it, the batch test and the floors read what it left."""
    if case not in DONE:
        DONE[case] = run_fixture(pa, oracle, case)
    return DONE[case]


def run_fixture(pa, oracle, case):
    fx = fd.Fixture(case)
    og = fx.graph(oracle)
    assert not fx.error and len(fx.seq) <= fd.MAX_LEN and fd.enough(og), case  # usable, by the host test's rule
    out = Lone()
    ann = pa.Annotator(pa.make_params(**fx.params))
    try:
        st0, offs0, genes0 = run_batch(ann, [fx.seq], None if fx.trnas is None else [fx.trnas])
        assert st0[0] == 0
        ref, ev = Yard(ann, 0), EvRef(ann, 0)
        called = ref.called(genes0)
        dg = DeviceGraph(ref, called)
        # the device's graph is the oracle's: the draws solved here are the very ones the host test counted
        assert sorted(dg.orf_edge) == sorted(og.orf_edge) and dg.called == og.called, case
        assert sum(abs(int(f)) == 4 for f in ref.frame) == sum(abs(f) == 4 for f in og.frame) and (sum(abs(int(f)) == 4 for f in ref.frame) > 0) == bool(fx.trnas)
        D = ann.path(0)[1]
        out.draws = fd.draws(oracle, fx, og)
        run_bytes = (0, genes0.tobytes(), np.float64(0.0).tobytes(), 0, ann.path(0)[0].tobytes(), D)

        def note(kind, j, sol, res, margins):
            c = out.count[kind]
            c[outcome(sol)] += 1
            c["kept"] += sol["count"]
            genes = res[2][res[1][0]:res[1][1]]
            out.with_trna += outcome(sol) == "ok" and any(abs(int(f)) == 4 for f in genes["frame"])
            out.single[(kind, j)] = (contig_bytes(ann, res, 0), margin_bytes(margins, 0))

        def masked(j, F, B, counted=True):
            """Refused only, then refused + biased: remargins() and redist() both ways, then the drops and replacements of that solve, every
            record; they disturb nothing resident."""
            for kind, call, bias in (("mask", lambda: ann.reannotate([F]), None), ("evidence", lambda: evidence(ann, [B], [F]), B)):
                res = call()
                st, offs, genes, delta = res
                sol = check(ann, ref, F, None, bias, int(st[0]), genes, delta[0], 0, D)
                mg = ann.remargins()
                assert int(mg[0][0]) == int(st[0])
                check_contig(ann, ev, F, bias, int(mg[0][0]), mg[2], genes, nodes=True)
                if counted:
                    note(kind, j, sol, res, mg)
                first = [x.tobytes() for x in mg]
                out.drops[(kind, j)], out.drop_bytes[(kind, j)] = check_drops(ann, ev, F, bias, genes, j)
                assert out.drops[(kind, j)]["status"] == int(st[0])
                assert [x.tobytes() for x in ann.remargins()] == first, (kind, j)

        for j, d in enumerate(out.draws):
            F, R, B = indexed(ref, d)
            masked(j, F, B)
            # refused + required, then all three: pinmargins() and pindist() both ways
            for kind, call, bias in (("pin", lambda: ann.constrain([F], [R]), None), ("full", lambda: curate(ann, [B], [F], [R]), B)):
                res = call()
                st, offs, genes, delta, unmet = res
                sol = check(ann, ref, F, R, bias, int(st[0]), genes, delta[0], int(unmet[0]), D)
                pm = ann.pinmargins()
                assert int(pm[0][0]) == int(st[0])
                check_pin(ann, ref, F, R, bias, int(pm[0][0]), pm[2], pm[3], genes, nodes=True)
                note(kind, j, sol, res, pm)
                if R:  # under required ORFs the drops are another definition: PHX_E_STATE, and nothing resident moves
                    first = [x.tobytes() for x in pm]
                    for refuses in (ann.redrops, ann.rereplacements):
                        with pytest.raises(pa.PhxError) as e:
                            refuses()
                        assert e.value.code == -13 and "required" in str(e.value), (kind, j)
                    assert [x.tobytes() for x in ann.pinmargins()] == first, (kind, j)
                    out.refused += 1
        extra = fd.removed_draw(oracle, fx, og)  # the second directed draw: a tRNA gene on the removed side of a drop
        assert (extra is not None) == (case in REMOVED)
        if extra is not None:
            F, R, B = indexed(ref, extra)
            masked(len(out.draws), F, B, counted=False)
        check_scenario_batches(ann, ref, out, D, run_bytes)
        check_derived_batches(ann, ref, out, called, D)
    finally:
        ann.close()
        rd._solved.clear()  # (the yardstick's solves of this fixture, shared by check_contig and check_records)
    return out


def check_scenario_batches(ann, ref, out, D, run_bytes):
    """One call per family: the fixture's draws, an empty scenario and the first draw again."""
    idx = [indexed(ref, d) for d in out.draws]
    n = len(idx)
    order = list(range(n)) + [None, 0]  # (None: the empty scenario)
    pick = lambda j, x: (0,) + (tuple(None for _ in x(idx[0])) if j is None else x(idx[j]))
    families = (("mask", ann.scenarios, lambda t: (t[0],), lambda t: (t[0], (), None)),
                ("pin", ann.pinned_scenarios, lambda t: (t[0], t[1]), lambda t: (t[0], t[1], None)),
                ("evidence", ann.evidence_scenarios, lambda t: ([(k, score(B)) for k, B in t[2].items()], t[0]), lambda t: (t[0], (), t[2])))
    for kind, call, args, solve in families:
        res = call([pick(j, args) for j in order])
        assert len(res[0]) == n + 2
        for x, j in enumerate(order):
            F, R, B = ([], [], None) if j is None else solve(idx[j])
            check_scenario(ann, res, x, 0, ref.solve(F, R, B), len(R), D)
            want = run_bytes if j is None else out.single[(kind, j)][0]
            assert scenario_bytes(ann, res, x, 0) == want, (kind, x, j)  # the single call's bytes


def check_derived_batches(ann, ref, out, called, D):
    orfs = ref.orfs
    same_stop = lambda a, b: orfs[a]["stop"] == orfs[b]["stop"] and (orfs[a]["frame"] > 0) == (orfs[b]["frame"] > 0)
    # start_drops(): every called gene's own ORF refused
    dst, doffs, drec = ann.drop_margins()
    st, offs, rec, soffs, genes = ann.start_drops()
    assert st[0] == dst[0] == 0 and offs.tolist() == doffs.tolist() and [int(r["orf"]) for r in rec] == called
    for x, r in enumerate(rec):
        k, new = int(r["orf"]), genes[soffs[x]:soffs[x + 1]]
        sol = ref.solve([k])
        check_record(sol, 0, r["status"], r["drop"], 0, new, D, ("start_drops", k))
        again = [a for a in ref.called(new) if same_stop(a, k)]
        assert k not in ref.called(new) and len(again) <= 1 and int(r["restart"]) == (again[0] if again else -1), ("start_drops", k, int(r["restart"]))
    # alt_starts(max_alts=2): every other ORF of a called gene's stop group required, the first two of each
    st, offs, rec, soffs, genes = ann.alt_starts(max_alts=2)
    want = [(k, int(a)) for k in called for a in [a for a in np.nonzero(orfs["group"] == orfs["group"][k])[0] if a != k][:2]]
    assert st[0] == 0 and [(int(r["orf"]), int(r["alt"])) for r in rec] == want
    for x, r in enumerate(rec):
        assert same_stop(int(r["alt"]), int(r["orf"]))
        check_record(ref.solve((), [int(r["alt"])]), 1, r["status"], r["delta"], int(r["unmet"]), genes[soffs[x]:soffs[x + 1]], D, ("alt_starts", int(r["alt"])))
    # evidence_scan(): three of the draws' biased ORFs, each on its own
    hits = []
    for d in out.draws:
        for k, B in indexed(ref, d)[2].items():
            if len(hits) < 3 and k not in [h[0] for h in hits]:
                hits.append((k, B))
    assert len(hits) == 3
    st, offs, rec, soffs, genes = ann.evidence_scan([[(k, score(B)) for k, B in hits]])
    assert st[0] == 0 and offs.tolist() == [0, 3] and len(rec) == 3
    for x, (k, B) in enumerate(hits):
        r, new = rec[x], genes[soffs[x]:soffs[x + 1]]
        assert int(r["orf"]) == k and int(r["was_called"]) == (k in called)
        check_record(ref.solve((), (), {k: B}), 0, r["status"], r["delta"], 0, new, D, ("evidence_scan", k, B))
        assert int(r["called"]) == (k in ref.called(new))


# ---- 1. one fixture, one context, one run ----
@pytest.mark.parametrize("case", USABLE)
def test_every_family_on_a_fixture_against_the_yardstick(pa, oracle, case):
    out = sweep(pa, oracle, case)
    n = len(out.draws)
    assert n == 5 + (case in TRNA) and all(sum(c[w] for w in ("ok", "cycle", "nopath")) == n for c in out.count.values())  # no draw is left out
    print("%s: %s, %d solves with a tRNA gene on the path" % (case, {k: (c["ok"], c["cycle"], c["kept"]) for k, c in out.count.items()}, out.with_trna))
    assert sorted(out.drops) == sorted((kind, j) for kind in ("mask", "evidence") for j in range(n + (case in REMOVED))) and out.refused == 2 * n
    drops = {k: sum(c[k] for c in out.drops.values()) for k in ("records", "compared", "bypass", "exact", "trna_pairs", "removed", "added", "splice")}
    print("%s: drops and replacements %s" % (case, drops))
    assert drops["records"] == drops["compared"] and drops["bypass"] == drops["exact"]  # no record, and no witness' length, went unchecked


# ---- 2. one batch, each contig with its own hit list ----
def test_one_batch_with_trna_hits_equals_the_lone_fixtures(pa, oracle):
    """The fixtures of the default parameter set side by side: tRNA nodes at a non-zero node and edge offset under BatchView, SlotView and
    MgDrop, whose refused and biased bits of small neighbours (edge_L200 has 14 edges) share 32-bit words."""
    lone = {case: sweep(pa, oracle, case) for case in BATCHED}
    fxs = [fd.Fixture(case) for case in BATCHED]
    assert all(fx.params == fxs[0].params for fx in fxs) and [fx.case for fx in fxs if fx.trnas] == TRNA
    ann = pa.Annotator(pa.make_params(**fxs[0].params))
    st0, offs0, genes0 = run_batch(ann, [fx.seq for fx in fxs], [fx.trnas or [] for fx in fxs])
    n = ann.n
    assert st0.tolist() == [0] * n
    assert [i for i in range(n) if (np.abs(ann.nodes(i)["frame"]) == 4).any()] == [BATCHED.index(c) for c in TRNA] and BATCHED.index(TRNA[0]) > 0
    refs = [CuRef(ann, i) for i in range(n)]
    idx = [[indexed(refs[i], d) for d in lone[fx.case].draws] for i, fx in enumerate(fxs)]
    col = lambda j, x: [idx[i][j][x] for i in range(n)]
    # round 0 through curate() + pinmargins(), round 1 through evidence() + remargins()
    res = curate(ann, col(0, 2), col(0, 0), col(0, 1))
    pm = ann.pinmargins()
    for i, fx in enumerate(fxs):
        assert (contig_bytes(ann, res, i), margin_bytes(pm, i)) == lone[fx.case].single[("full", 0)], fx.case
    res = evidence(ann, col(1, 2), col(1, 0))
    mg = ann.remargins()
    for i, fx in enumerate(fxs):
        assert (contig_bytes(ann, res, i), margin_bytes(mg, i)) == lone[fx.case].single[("evidence", 1)], fx.case
    # ... and its drops and replacements under MgDrop: the bitmap words of neighbouring small contigs are shared; then draw 2's masks
    dr, rp = ann.redrops(), ann.rereplacements()
    for i, fx in enumerate(fxs):
        assert drop_bytes(ann, dr, rp, i) == lone[fx.case].drop_bytes[("evidence", 1)], fx.case
    assert [x.tobytes() for x in ann.remargins()] == [x.tobytes() for x in mg]
    res = ann.reannotate(col(2, 0))
    rp, dr = ann.rereplacements(), ann.redrops()
    for i, fx in enumerate(fxs):
        assert contig_bytes(ann, res, i) == lone[fx.case].single[("mask", 2)][0], fx.case
        assert drop_bytes(ann, dr, rp, i) == lone[fx.case].drop_bytes[("mask", 2)], fx.case
    assert sum(len(lone[fx.case].drop_bytes[("mask", 2)][2]) for fx in fxs) == len(dr[2]) >= n
    # one pinned and one evidence scenario call across all contigs, every draw of every fixture
    slots = [(i, j) for i in range(n) for j in range(len(idx[i]))]
    res = ann.pinned_scenarios([(i, idx[i][j][0], idx[i][j][1]) for i, j in slots])
    for x, (i, j) in enumerate(slots):
        assert scenario_bytes(ann, res, x, i) == lone[fxs[i].case].single[("pin", j)][0], (fxs[i].case, j)
    res = ann.evidence_scenarios([(i, [(k, score(B)) for k, B in idx[i][j][2].items()], idx[i][j][0]) for i, j in slots])
    for x, (i, j) in enumerate(slots):
        assert scenario_bytes(ann, res, x, i) == lone[fxs[i].case].single[("evidence", j)][0], (fxs[i].case, j)
    assert len(slots) == 5 * n + len(TRNA)
    ann.close()


# ---- 3. nothing to do ----
@pytest.mark.parametrize("case", sorted(DEGENERATE))
def test_every_family_with_nothing_to_do_on_a_degenerate_fixture(pa, case):
    """An empty graph, a status without a path, a run error: every family returns the run's status, no genes and no records."""
    fx = fd.Fixture(case)
    assert case in [f.case for f in fd.degenerate()]
    ann = pa.Annotator(pa.make_params(**fx.params))
    st0, offs0, genes0 = run_batch(ann, [fx.seq], None if fx.trnas is None else [fx.trnas])
    want = DEGENERATE[case]
    assert st0.tolist() == [want] and len(genes0) == 0
    delta = 0.0 if want == 0 else np.inf
    none = [None]

    def plain(res):
        assert res[0].tolist() == [want] and res[1].tolist() == [0, 0] and len(res[2]) == 0 and res[3].tolist() == [delta], (case, res[0].tolist(), res[3].tolist())
        assert len(res) == 4 or res[4].tolist() == [0]

    def no_records(out):
        assert out[0].tolist() == [want] and int(out[1][-1]) == 0 and all(len(x) == 0 for x in out[2:]), (case, out[0].tolist())

    for call in (lambda: ann.reannotate(none), lambda: ann.evidence(none, none), lambda: ann.constrain(none, none), lambda: ann.curate(none, none, none),
                 lambda: ann.constrain(), lambda: ann.curate()):
        plain(call())
        no_records(ann.remargins())
        no_records(ann.pinmargins())
        for out in (ann.redrops(), ann.rereplacements()):  # (none of these calls requires an ORF)
            no_records(out)
            assert out[1].tolist() == [0, 0]
        V = max(int(ann.globals(0).n_node), 0)
        for to_target in (False, True):
            assert len(ann.redist(0, to_target=to_target)) == len(ann.pindist(0, to_target=to_target)) == V
    for call in (lambda: ann.scenarios([(0, None)]), lambda: ann.pinned_scenarios([(0, None, None)]), lambda: ann.evidence_scenarios([(0, None, None)]),
                 lambda: ann.scenarios([(0, [])]), lambda: ann.pinned_scenarios([(0, [], [])]), lambda: ann.evidence_scenarios([(0, [], [])])):
        plain(call())
    for out in (ann.start_drops(), ann.alt_starts(max_alts=2), ann.evidence_scan(none), ann.evidence_scan([[]])):
        assert out[0].tolist() == [want] and out[1].tolist() == [0, 0] and len(out[2]) == 0 and out[3].tolist() == [0] and len(out[4]) == 0, (case, out[0].tolist())
    ann.close()


# ---- 4. the floors ----
def test_the_sweep_meets_its_floors(pa, oracle):
    """Conditions, not measurements: tests/test_fixture_sweep_host.py proves on the CPU that the yardstick alone meets them (170 draws of
    each kind; mask and evidence all settle; pin and full 153 settle and 17 meet a negative cycle; 202 required ORFs kept; at least 2 full
    draws settle on every fixture).  The directed draws of the tRNA fixtures come on top.  The floors of redrops() and rereplacements()
    sit a little below the host's counts, as 150 sits below 153: a tie the device breaks otherwise cannot fail them, and they hide nothing —
    every record returned is compared in full whatever their number."""
    done = {case: sweep(pa, oracle, case) for case in USABLE}
    assert sorted(done) == sorted(USABLE) and len(done) == 34
    tot = {k: {w: sum(d.count[k][w] for d in done.values()) for w in ("ok", "cycle", "nopath", "kept")} for k in fd.KINDS}
    print("fixture sweep on the device:", tot, "solves with a tRNA gene on the path:", {c: done[c].with_trna for c in TRNA})
    assert tot["full"]["ok"] >= 150 and tot["full"]["cycle"] >= 15 and tot["full"]["kept"] >= 200
    assert all(d.count["full"]["ok"] >= 2 for d in done.values())
    for kind in ("mask", "evidence"):  # every draw is checked with status 0
        assert tot[kind]["ok"] == 170 + len(TRNA) and tot[kind]["cycle"] == tot[kind]["nopath"] == 0
    assert all(done[c].with_trna >= 1 for c in TRNA)
    # redrops() and rereplacements().  The host test's counts, over the seeded and the first directed draws: 1080 mask and 1074 evidence
    # records (seeded), at least 10 per fixture, 86 tRNA pairs on a P' without a record (trna_gap 48, trna_gap_left 36), 46 records whose
    # genes hold a tRNA gene (trna_phiX174 22, trna_synth6k 24), all on the added side; the second directed draw has one on the removed side.
    upto = lambda d, kinds, last, key: sum(c[key] for (kind, j), c in d.drops.items() if kind in kinds and j <= last)
    both = ("mask", "evidence")
    dtot = {kind: sum(upto(d, (kind,), 4, "compared") for d in done.values()) for kind in both}
    pairs = {c: upto(done[c], both, 5, "trna_pairs") for c in TRNA}
    splice = {c: upto(done[c], both, 5, "splice") for c in TRNA}
    removed = {c: upto(done[c], both, 6, "removed") for c in TRNA}
    print("drops and replacements on the device: records compared %s, tRNA pairs without a record %s, records with a tRNA gene %s, on the removed side %s"
          % (dtot, pairs, splice, removed))
    assert dtot["mask"] >= 1000 and dtot["evidence"] >= 1000
    assert all(upto(d, both, 4, "compared") >= 10 for d in done.values())
    assert all(c["status"] == 0 for d in done.values() for c in d.drops.values())
    assert sum(pairs.values()) >= 80 and pairs["trna_gap"] >= 40 and pairs["trna_gap_left"] >= 30
    assert sum(splice.values()) >= 40 and splice["trna_phiX174"] >= 20 and splice["trna_synth6k"] >= 20
    assert all(removed[c] >= 1 for c in REMOVED)
    assert all(c["records"] == c["compared"] and c["bypass"] == c["exact"] for d in done.values() for c in d.drops.values())  # no record went unchecked
    assert all(len(d.drops) == 2 * (len(d.draws) + (c in REMOVED)) and d.refused == 2 * len(d.draws) for c, d in done.items())
