"""Combined scenario batches on the device (phx_curate_scenarios_flat, Annotator.curate_scenarios / curated_scan).  Every
scenario is compared with its definition — Annotator.curate(..., solve_all=True) of its contig with exactly that bias and those two sets,
byte for byte, tapped path included — with the sibling scenario call it reduces to, or with the yardstick of tests/test_curate_gpu.py
(CuRef: python integers over the device's own tapped edges), never with the code under test."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from ambiguous_contig import TIE_SCRATCH_INITIAL, copies_that_outgrow, large_ambiguous_contig, tie_scratch_need
from test_constrain_gpu import fuzz, run_batch, wide_cases, wide_contig
from test_curate_gpu import Batch, CuRef, DeviceGraph, NoGraph, contig_bytes, curate, sets_of
from test_evidence_gpu import score
from test_fixture_sweep_gpu import check_scenario, indexed, outcome, scenario_bytes
from test_fixture_sweep_host import TRNA, USABLE
from test_scenarios_gpu import result_digest

import curate_draws as cd
import fixture_draws as fd

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE, S_NEGCYCLE, S_NOPATH, S_OVERFLOW = -1, -13, -9, 1, -7
B_MAX = 1 << 52


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def as_scen(i, bias=None, F=None, R=None):
    """(contig, bias, forbid, require) as Annotator.curate_scenarios takes it; bias: None, {ORF: integer B} or (ORF, integer B) pairs."""
    pairs = None if bias is None else [(k, score(B)) for k, B in (bias.items() if hasattr(bias, "items") else bias)]
    return (i, pairs, None if F is None else list(F), None if R is None else list(R))


def lone(ann, s):
    """contig_bytes of the scenario's contig from curate(..., solve_all=True) with its bias and its sets on that contig alone: the definition."""
    i, bias, F, R = s
    b, f, r = [None] * ann.n, [None] * ann.n, [None] * ann.n
    b[i], f[i], r[i] = bias, F, R
    return contig_bytes(ann, ann.curate(b, f, r, solve_all=True), i)


def all_bytes(ann, res, scen):
    return [scenario_bytes(ann, res, j, s[0]) for j, s in enumerate(scen)]


def equal_lone(ann, scen):
    """One call of `scen`; every scenario against its lone curate().  Returns (result, bytes per scenario)."""
    res = ann.curate_scenarios(scen)
    got = all_bytes(ann, res, scen)  # (the taps first: the chunk stays resident through the lone calls, which own other buffers)
    for j, s in enumerate(scen):
        assert got[j] == lone(ann, s), (j, s)
    return res, got


def small_scen(b):
    """The 45 seeded draws of curate_draws.mixes over the small batch, by ORF index: [(contig, {ORF: B}, forbid, require)] round by round."""
    graphs = [DeviceGraph(b.refs[i], b.called[i]) if i in b.refs else NoGraph() for i in range(b.n)]
    out = []
    for row in cd.mixes(graphs):
        for i, d in enumerate(row):
            if d is not None:
                by = b.refs[i].by_ends
                out.append((i, {by[k]: B for k, B in d["bias"].items()}, [by[k] for k in d["forbid"]], [by[k] for k in d["require"]]))
    return out


def run_small(pa):
    ann = pa.Annotator()
    b = Batch(ann, cd.mix_seqs(pa))
    draws = small_scen(b)
    scen = [as_scen(*d) for d in draws]
    res = ann.curate_scenarios(scen)
    return ann, b, draws, scen, res


@pytest.fixture(scope="module")
def small(pa):
    ann, b, draws, scen, res = run_small(pa)
    yield ann, b, draws, scen, [x.copy() for x in res], ann.scenario_chunks()
    ann.close()


def child_main():
    """Case 6's child process: the one call of case 1 under the PHX_SCEN_BYTES of the environment; prints the chunk count, a digest, and
    what scenario_path says of the first and the last scenario."""
    import phanotate_amd as pa

    ann, b, draws, scen, res = run_small(pa)
    try:
        ann.scenario_path(0, scen[0][0])
        first = 0
    except pa.PhxError as e:
        first = e.code
    last = len(ann.scenario_path(len(scen) - 1, scen[-1][0])[0])
    print("SCEN %d %d %s %d %d" % (len(scen), ann.scenario_chunks(), result_digest(res), first, last))
    ann.close()


# ---- 1. the definition ----
def test_the_45_draws_in_one_call_equal_lone_curate_and_the_yardstick(small, oracle):
    ann, b, draws, scen, res, chunks = small
    for g, seq in zip([DeviceGraph(b.refs[i], b.called[i]) if i in b.refs else NoGraph() for i in range(b.n)], b.seqs):  # the draws are the ones the host test counts
        og = cd.OracleGraph(oracle, seq)
        assert g.ok == og.ok and (not g.ok or (sorted(g.orf_edge) == sorted(og.orf_edge) and g.called == og.called))
    assert len(scen) == 45 and chunks == 1 and len(res) == 5
    st, offs, genes, delta, unmet = res
    assert offs[0] == 0 and offs[-1] == len(genes) and (np.diff(offs) >= 0).all()
    assert st.tolist() == [0] * 45
    got = all_bytes(ann, res, scen)
    kept = 0
    for j, (i, bias, F, R) in enumerate(draws):
        sol = b.refs[i].solve(F, R, bias)
        check_scenario(ann, res, j, i, sol, len(R), b.D[i])
        kept += sol["count"]
    for j, s in enumerate(scen):
        assert got[j] == lone(ann, s), (j, draws[j])
    assert kept >= 30 and len({float(d) for d in delta}) >= 30


# ---- 2. the reductions ----
def test_one_chunk_of_all_four_kinds_equals_the_sibling_calls(small):
    ann, b, draws, scen0, res0, chunks = small
    forbid, require, bias = sets_of(b, 2710)
    full = [i for i in b.idx if require[i]]
    assert len(full) >= 5
    scen, kind = [], []
    for i in full:  # plain, pinned, biased, both — interleaved contig by contig
        scen += [as_scen(i, None, forbid[i], None), as_scen(i, None, forbid[i], require[i]), as_scen(i, bias[i], forbid[i], None), as_scen(i, bias[i], forbid[i], require[i])]
        kind += [0, 1, 2, 3]
    res = ann.curate_scenarios(scen)
    assert ann.scenario_chunks() == 1
    got = all_bytes(ann, res, scen)
    assert res[4][[k for k, x in enumerate(kind) if x in (0, 2)]].tolist() == [0] * (2 * len(full))  # no required list: unmet 0
    for j, (s, x) in enumerate(zip(scen, kind)):
        i, bb, F, R = s
        one = ann.scenarios([(i, F)]) if x == 0 else ann.pinned_scenarios([(i, F, R)]) if x == 1 else ann.evidence_scenarios([(i, bb, F)]) if x == 2 else None
        want = lone(ann, s) if one is None else scenario_bytes(ann, one, 0, i)
        assert got[j] == want, (j, x, s)
    assert len({got[j][2] for j in range(4)}) >= 3  # (the kinds differ from one another: the test means something)
    # biases that sum to zero, and a bias on a refused ORF only: the pinned range — the bytes of pinned_scenarios(), and its cached result
    i = full[0]
    k = next(iter(bias[i]))
    zero = [(i, [(k, 1.0), (k, -2.5), (k, 1.5)], forbid[i], require[i]), (i, [(forbid[i][0], -40.0)], forbid[i], require[i]), (i, [(k, 0.0009)], forbid[i], require[i])]
    pinned = [(i, forbid[i], require[i])] * 3
    ann.curate_scenarios([as_scen(i, bias[i], forbid[i], require[i])])  # (another solve in between)
    want = [np.ascontiguousarray(x).tobytes() for x in ann.pinned_scenarios(pinned)]
    ms = ann.scenarios_ms()
    path = ann.scenario_path(1, i)[0].tobytes()
    assert [np.ascontiguousarray(x).tobytes() for x in ann.curate_scenarios(zero)] == want and ann.scenarios_ms() == ms  # served from the sibling's cache: no kernel ran
    ann.curate_scenarios([as_scen(i, bias[i], forbid[i], require[i])])
    assert [np.ascontiguousarray(x).tobytes() for x in ann.curate_scenarios(zero)] == want and ann.scenario_path(1, i)[0].tobytes() == path  # ... and solved afresh
    ms = ann.scenarios_ms()
    assert [np.ascontiguousarray(x).tobytes() for x in ann.pinned_scenarios(pinned)] == want and ann.scenarios_ms() == ms  # the cache serves the sibling the other way round
    # R empty, and both empty, likewise
    ev = [(i, [(k, -3.0)], forbid[i])]
    want = [np.ascontiguousarray(x).tobytes() for x in ann.evidence_scenarios(ev)]
    ms = ann.scenarios_ms()
    for rq in (None, []):
        got4 = ann.curate_scenarios([(i, [(k, -3.0)], forbid[i], rq)])
        assert [np.ascontiguousarray(x).tobytes() for x in got4[:4]] == want and got4[4].tolist() == [0] and ann.scenarios_ms() == ms
    want = [np.ascontiguousarray(x).tobytes() for x in ann.scenarios([(i, forbid[i])])]
    ms = ann.scenarios_ms()
    got4 = ann.curate_scenarios([(i, None, forbid[i], None)])
    assert [np.ascontiguousarray(x).tobytes() for x in got4[:4]] == want and got4[4].tolist() == [0] and ann.scenarios_ms() == ms


# ---- 3. the tile path ----
SW_ADV, SW_MAX, SW_THREADS, ECAP = 32, 64, 512, 1024


def window_plan(nodes, in_off):
    """lds_sweep's plan restated: window k starts at node 32 k and holds its 32 nodes plus the nodes of the next 500 bp while the tile holds their in-edges."""
    V = len(nodes)
    ncds = V - 2
    pos = nodes["pos"]
    plan = []
    for v0 in range(0, V, SW_ADV):
        vadv = min(v0 + SW_ADV, V)
        cnt = 0
        for idx in range(v0, v0 + SW_MAX):
            ok = idx < V
            if ok and idx >= vadv:
                ok = idx < ncds and vadv - 1 < ncds and pos[idx] < pos[vadv - 1] + 500 and in_off[idx + 1] - in_off[v0] <= ECAP
            if not ok:
                break
            cnt += 1
        plan.append(cnt)
    return plan


def slots_of(ann, i, ref):
    """({in-edge slot of the contig: its ORF}, in_off) of contig i: the tapped edges come in the order of the in-edge slots."""
    ed = ann.edges(i)
    of_edge = {e: k for k, e in enumerate(ref.orf_edge) if e is not None}
    slot_orf = {x: of_edge[(int(u), int(v))] for x, (u, v) in enumerate(zip(ed["src"], ed["dst"])) if (int(u), int(v)) in of_edge}
    assert len(slot_orf) == len(of_edge) and (np.diff(ed["dst"]) >= 0).all()
    return slot_orf, np.searchsorted(ed["dst"], np.arange(ref.V + 1))


def same_thread_pairs(ann, i, ref):
    """Pairs of ORFs whose rows one thread prefetches for one tile: in-edge slots SW_THREADS apart inside one tiled window."""
    slot_orf, in_off = slots_of(ann, i, ref)
    out, widest = [], 0
    for k, nwin in enumerate(window_plan(ann.nodes(i), in_off)):
        e0, e1 = int(in_off[k * SW_ADV]), int(in_off[k * SW_ADV + nwin])
        if e1 - e0 > ECAP:
            continue
        widest = max(widest, e1 - e0)
        out += [(slot_orf[x], slot_orf[x + SW_THREADS]) for x in range(e0, e1 - SW_THREADS) if x in slot_orf and x + SW_THREADS in slot_orf]
    return sorted(set(out)), widest


def test_a_required_and_a_biased_row_in_one_threads_part_of_a_tile(pa):
    """A stop with between 512 and 1024 starts: its rows fill one tiled window, and rows 512 slots apart are one thread's two rows."""
    found = None
    for ncodons in (3000, 3600, 2400, 4200, 1800):
        ann = pa.Annotator(flags=("solver_no_wave",))
        st0, offs0, genes0 = run_batch(ann, [wide_contig(pa, ncodons, 6000, density=0.2)])
        ref = CuRef(ann, 0) if st0[0] == 0 else None
        pairs, widest = same_thread_pairs(ann, 0, ref) if ref is not None else ([], 0)
        print("wide_contig(%d): widest tiled window %d rows, %d pairs of rows of one thread" % (ncodons, widest, len(pairs)))
        if pairs:
            found = ncodons
            break
        ann.close()
    assert found is not None, "no candidate contig has a tiled window with two ORF rows 512 slots apart"
    mst, moffs, mrec = ann.margins()
    live = [(a, c) for a, c in pairs if mrec[a]["through"] and mrec[c]["through"] and not mrec[a]["called"] and not mrec[c]["called"]]
    assert live
    D = ann.path(0)[1]
    (a, c), (a2, c2) = live[0], live[-1]
    spec = (([a], {c: -2500}), ([c], {a: -2500}), ([a2, c2], {a2: -700, c2: 900}), ([a], {a: 400, c: -300}))
    scen = [as_scen(0, bias, None, req) for req, bias in spec]
    res, got = equal_lone(ann, scen)
    ok = 0
    for j, (req, bias) in enumerate(spec):
        sol = ref.solve((), req, bias)
        check_scenario(ann, res, j, 0, sol, len(req), D)
        ok += outcome(sol) == "ok"
    ann.close()
    assert ok >= 3


def test_rows_of_one_stop_the_ends_of_the_slots_and_long_lists(small):
    ann, b, draws, scen0, res0, chunks = small
    i = 0  # the 20 kb contig
    ref = b.refs[i]
    assert int(ann.globals(i).n_limbs) == 2 and len(b.seqs[i]) == 20000
    slot_orf, in_off = slots_of(ann, i, ref)
    of_edge = {e: k for k, e in enumerate(ref.orf_edge) if e is not None}
    pool = set(b.reachable(i))
    # a required and a biased row of one stop group (adjacent rows of one node), reachable both
    orfs = ann.orfs(i)
    grp = {}
    for k in sorted(pool):
        grp.setdefault(int(orfs["group"][k]), []).append(k)
    same = [ks for ks in grp.values() if len(ks) >= 2]
    assert same
    a, c = same[len(same) // 2][:2]
    slots = [slot_orf[x] for x in sorted(slot_orf)]
    first, last = slots[0], slots[-1]
    cg = b.called[i]
    have = sorted(of_edge.values())
    r0 = next(k for k in sorted(pool)[len(pool) // 2:] if k not in have[:8] and k not in (first, last))
    f0 = next(k for k in cg if k not in (first, last))
    many = [(int(k), 3) for k in have[:300]]
    assert len(many) > 257
    scen = [as_scen(i, {c: -2500}, None, [a]), as_scen(i, {a: -2500}, None, [c]),          # the two rows of one node, either way
            as_scen(i, {a: -700, c: 900}, None, [a, c]),                                     # ... and both required and biased
            as_scen(i, {r0: -1200}, None, [r0]),                                             # one row both required and biased
            as_scen(i, {cg[1]: -5000, r0: 300}, [cg[1]], [r0]),                              # a row refused and biased
            as_scen(i, {first: -2000}, None, [last]), as_scen(i, {last: -2000}, None, [first]),  # the first and the last explicit in-edge slot
            as_scen(i, {first: 900, last: -900}, [f0], [first, last]),
            as_scen(i, {have[7]: -400}, None, [r0]),                                         # lists of 1, 2 and more than NT pairs
            as_scen(i, {have[7]: -400, have[-3]: 650}, None, [r0]),
            as_scen(i, many, None, [r0]), as_scen(i, list(reversed(many)) + [(r0, -3000)], [have[5]], [r0, have[5 + 1]])]
    res, got = equal_lone(ann, scen)
    for j, s in enumerate(scen[:8]):  # the yardstick as well, where the lists are short
        bias = {k: int(round(v * 1000)) for k, v in s[1]}
        check_scenario(ann, res, j, i, ref.solve(s[2] or (), s[3], bias), len(s[3]), b.D[i])
    assert len({g[2] for g in got}) >= 5


def test_a_bias_flips_which_of_two_required_starts_is_kept_in_one_call(small):
    ann, b, draws, scen0, res0, chunks = small
    pairs = []
    for i in b.idx:
        orfs, rec = ann.orfs(i), b.rec(i)
        ok = np.nonzero((rec["through"] == 1) & np.isfinite(rec["margin"]))[0]
        grp = {}
        for k in ok:
            grp.setdefault(int(orfs["group"][k]), []).append(int(k))
        cand = [(a, c) for ks in grp.values() for a in ks for c in ks if a < c and 0 < abs(float(rec["margin"][a]) - float(rec["margin"][c])) < 2.0 ** 30]
        pairs += [(i,) + p for p in cand[:3]]
    assert len(pairs) >= 8
    base = ann.curate_scenarios([as_scen(i, None, None, [a, c]) for i, a, c in pairs])
    scen, meta = [], []
    for x, (i, a, c) in enumerate(pairs):
        if base[0][x] != 0 or base[4][x] != 1:
            continue
        called = b.refs[i].called(base[2][base[1][x]:base[1][x + 1]])
        cheap, dear = (a, c) if a in called else (c, a)
        assert cheap in called and dear not in called
        rec = b.rec(i)
        gap = int(round((float(rec["margin"][dear]) - float(rec["margin"][cheap])) * 1000.0))
        scen.append(as_scen(i, {dear: -gap - 1000}, None, [a, c]))  # one SCORE unit past the tie
        meta.append((i, cheap, dear))
    assert len(scen) >= 6
    res, got = equal_lone(ann, scen)
    flipped = 0
    for x, (i, cheap, dear) in enumerate(meta):
        if res[0][x] != 0:
            continue
        called = b.refs[i].called(res[2][res[1][x]:res[1][x + 1]])
        assert res[4][x] == 1 and dear in called and cheap not in called, (i, cheap, dear)
        flipped += 1
    assert flipped >= 5, (flipped, len(scen))


def test_required_and_biased_rows_in_an_untiled_window(pa):
    ann = pa.Annotator(flags=("solver_no_wave",))
    st0, offs0, genes0 = run_batch(ann, [wide_contig(pa, 6000, 6000, density=0.2)])
    assert st0[0] == 0
    ed = ann.edges(0)
    indeg = np.bincount(ed["dst"])
    big = int(indeg.argmax())
    assert indeg[big] > 1024, int(indeg[big])  # more in-edges than the tile holds: that window is relaxed from global memory row by row
    ref = CuRef(ann, 0)
    mst, moffs, mrec = ann.margins()
    into = [k for k, e in enumerate(ref.orf_edge) if e is not None and e[1] == big and not mrec[k]["called"] and mrec[k]["through"]]
    assert len(into) > 1000
    D = ann.path(0)[1]
    a, m, z = into[0], into[len(into) // 2], into[-1]
    own = ref.called([g for g in genes0 if abs(int(g["frame"])) <= 3 and int(g["strand"]) == 1 and int(g["right"]) == int(ref.pos[big]) + 2])
    spec = (([a], {m: -3000}, None), ([m], {m: 500, z: -300}, None), ([a, z], {into[1]: -5000, m: 250}, None), ([into[1]], {a: -700}, own))
    scen = [as_scen(0, bias, fb, req) for req, bias, fb in spec]
    res, got = equal_lone(ann, scen)
    ok = 0
    for j, (req, bias, fb) in enumerate(spec):
        sol = ref.solve(fb or (), req, bias)
        check_scenario(ann, res, j, 0, sol, len(req), D)
        ok += outcome(sol) == "ok"
    ann.close()
    assert ok >= 3


# ---- 4. the four limb classes ----
@pytest.mark.parametrize("case", range(4))
def test_one_both_scenario_in_the_wide_classes(pa, case):
    seqs, nl = wide_cases(pa)[case]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    want = (4, 8, 8, 17)[case]  # 256 (solved in 320), 512 (576) twice and 1088 (1152) bits
    c = next(i for i in range(len(seqs)) if st0[i] == 0 and int(ann.globals(i).n_limbs) == want)
    mst, moffs, mrec = ann.margins()
    assert mst[c] == 0
    ref = CuRef(ann, c)
    rec = mrec[moffs[c]:moffs[c + 1]]
    pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0]
    long_one = int(pool[np.argmax(ref.orfs["length"][pool])])  # the widest ORF weights sit in the long ORF's group
    other = int(pool[np.random.RandomState(2716 + case).randint(len(pool))])
    cg = ref.called(genes0[offs0[c]:offs0[c + 1]])
    D = ann.path(c)[1]
    spec = (([long_one], {other: -2500, cg[0]: 4000}), ([other], {long_one: -(10 ** 6)}), ([long_one], {long_one: 999}))
    scen = [as_scen(c, bias, None, req) for req, bias in spec]
    res, got = equal_lone(ann, scen)
    seen = 0
    for j, (req, bias) in enumerate(spec):
        sol = ref.solve((), req, bias)
        check_scenario(ann, res, j, c, sol, len(req), D)
        seen += outcome(sol) == "ok"
    ann.close()
    assert seen >= 2


# ---- 5. negative cycles, and the statuses without a result, in one call ----
def test_negative_cycles_of_both_kinds_beside_clean_scenarios(pa):
    from phanotate_amd.fasta import read_fasta

    seqs = [seq for name, seq in read_fasta(os.path.join(ROOT, "tests", "golden", "constrain_cycle.fasta"))]
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops  # no path: what lies behind the first stops is out of the source's reach
    rng = np.random.RandomState(12)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    huge = pa.synth_contig(320, 2000).decode() + "atg" + "".join(sense[i] for i in rng.randint(0, len(sense), 24000)) + "taa" + pa.synth_contig(321, 2000).decode()
    seqs = seqs + [pa.synth_contig(61, 9000), unreachable, huge]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    assert st0.tolist()[:4] == [0, 0, 0, 1]
    scen, want = [], []
    for i in (0, 1):
        ref = CuRef(ann, i)
        cyc = [k for k, e in enumerate(ref.orf_edge) if e is not None and ref.on_cycle({e})]
        free = [k for k, e in enumerate(ref.orf_edge) if e is not None and k not in cyc]
        assert cyc and len(free) >= 2
        for k in (cyc[0], cyc[-1]):
            scen += [as_scen(i, {free[0]: 500}, None, [free[1]]),            # clean
                     as_scen(i, {free[0]: 500}, None, [k]),                  # a required edge on a cycle the source reaches
                     as_scen(i, {k: -(10 ** 9)}, None, [free[1]]),           # a bonus that turns that cycle negative, the required ORF elsewhere
                     as_scen(i, {k: -(10 ** 9)}, [k], [free[1]])]            # refusing the ORF takes either cycle away
            want += ["clean", S_NEGCYCLE, S_NEGCYCLE, "clean"]
    # a cycle the source cannot reach is no cycle of the solve: the contig without a path stays without one
    ref3 = CuRef(ann, 3)
    quiet = [k for k, e in enumerate(ref3.orf_edge) if e is None or not ref3.on_cycle({e})]
    apart = [k for k in quiet if ref3.orf_edge[k] is not None and ref3.on_cycle({ref3.orf_edge[k]}, anywhere=True)]
    assert len(apart) >= 2
    R3 = sorted({apart[0], quiet[0]})
    scen.append(as_scen(3, {apart[1]: -(10 ** 9), apart[0]: -700}, None, R3))
    want.append(S_NOPATH)
    # PHX_S_OVERFLOW beside a clean scenario: a contig without device distances.  (The limb test's own PHX_S_OVERFLOW cannot be produced on
    # the device — with |B| <= 2^52 a contig's biases add less than 2^83, DESIGN.md §19 — so the status that passes through stands in for it.)
    scen.append((4, None, None, None))
    want.append(S_OVERFLOW)
    scen.append(as_scen(2, None, None, None))
    want.append("clean")
    res, got = equal_lone(ann, scen)
    st, offs, genes, delta, unmet = res
    for j, w in enumerate(want):
        nreq = len(scen[j][3] or [])
        if w == "clean":
            assert st[j] in (0, S_NEGCYCLE), (j, int(st[j]))  # (the sets of a clean scenario may meet another cycle: lone curate() above says which)
            continue
        assert st[j] == w and offs[j + 1] == offs[j] and delta[j] == np.inf and unmet[j] == nreq and len(ann.scenario_path(j, scen[j][0])[0]) == 0, (j, int(st[j]), w)
    assert sum(st[j] == 0 for j, w in enumerate(want) if w == "clean") >= 6
    sol = ref3.solve((), R3, {apart[1]: -(10 ** 9), apart[0]: -700})
    assert not sol["cycle"] and sol["S"] is None
    ann.close()


# ---- 6. chunking does not matter ----
def test_three_or_more_chunks_give_the_same_bytes(small):
    ann, b, draws, scen, res, chunks = small
    code = "import sys; sys.path.insert(0, %r); import test_curate_scenarios_gpu as t; t.child_main()" % HERE
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=600, env=dict(os.environ, PHX_SCEN_BYTES="300000"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("SCEN ")][-1].split()
    assert int(line[1]) == len(scen) and int(line[2]) >= 3, line
    assert line[3] == result_digest(res)
    assert int(line[4]) == E_STATE and int(line[5]) > 0  # scenario_path: an earlier chunk's slices have been reused, the last chunk's serve


# ---- 7. state and arguments ----
def raw_call(ann, contig, foff, forf, roff, rorf, boff, borf, bval, oo=None, unmet=True):
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    contig, bval = np.ascontiguousarray(contig, np.int32), np.ascontiguousarray(bval, np.int64)
    foff, roff, boff = (None if x is None else np.ascontiguousarray(x, np.int64) for x in (foff, roff, boff))
    forf, rorf, borf = (np.ascontiguousarray(x, np.int32) for x in (forf, rorf, borf))
    oo = np.ascontiguousarray(ann.orf_offsets() if oo is None else oo, np.int64)
    S = len(contig)
    offs, st, delta, um, total = np.zeros(S + 1, np.int64), np.zeros(S + 1, np.int32), np.zeros(S + 1), np.zeros(S + 1, np.int32), C.c_int64()
    opt = lambda x: None if x is None else vp(x)
    return ann.L.phx_curate_scenarios_flat(ann.h, S, vp(contig), opt(foff), vp(forf), opt(roff), vp(rorf), opt(boff), vp(borf), vp(bval), vp(oo), 0, None, 0, vp(offs), vp(st), vp(delta),
                                           vp(um) if unmet else None, C.byref(total))


def test_the_call_disturbs_nothing_is_cached_and_refuses_bad_state_and_arguments(pa):
    ann = pa.Annotator()
    ann.upload([pa.synth_contig(5, 5000)])
    with pytest.raises(pa.PhxError) as e:  # before a run
        ann.curate_scenarios([(0, None, None, None)])
    assert e.value.code == E_STATE
    assert raw_call(ann, [0], [0, 0], [0], [0, 0], [0], [0, 0], [0], [0], oo=[0, 0]) == E_STATE
    b = Batch(ann, fuzz(31, 12))
    forbid, require, bias = sets_of(b, 2715)
    full = [i for i in b.idx if require[i]]
    assert len(full) >= 5

    def everything():
        cu = curate(ann, bias, forbid, require)  # (the cached combined re-annotation: a repeated call runs no kernel)
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in cu], ann.reannotate_ms(),
                [x.tobytes() for x in ann.pinmargins()], [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n)])

    before = everything()
    scen = [as_scen(i, bias[i], forbid[i], require[i]) for i in full] + [as_scen(i, None, None, None) for i in range(ann.n)]
    res = ann.curate_scenarios(scen)
    assert [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n)] == before[5]  # curate()'s cached result stands: no solve of its own ran since
    assert everything() == before
    ms = ann.scenarios_ms()
    assert ms["solve"] > 0 and ann.scenario_chunks() == 1
    assert result_digest(ann.curate_scenarios(scen)) == result_digest(res) and ann.scenarios_ms() == ms  # the second identical call reuses the solve
    # the key holds all three lists: another bias, another required list and another refused list are other solves; the same sums in other pairs are not
    i0 = next(i for x, i in enumerate(full) if res[0][x] == 0)
    x0 = full.index(i0)
    scen = [scen[x0]] + scen[:x0] + scen[x0 + 1:]
    res = ann.curate_scenarios(scen)
    g0 = next(k for k in b.refs[i0].called(res[2][res[1][0]:res[1][1]]) if k not in require[i0])
    assert result_digest(ann.curate_scenarios([as_scen(i0, {g0: 10 ** 6}, forbid[i0], require[i0])] + scen[1:])) != result_digest(res)  # (a penalty on a gene the result calls: paid or avoided, S moves)
    assert result_digest(ann.curate_scenarios([as_scen(i0, bias[i0], forbid[i0], require[i0][:1])] + scen[1:])) != result_digest(res)
    split = [as_scen(i0, [(k, B // 2) for k, B in bias[i0].items()] + [(k, B - B // 2) for k, B in reversed(list(bias[i0].items()))], forbid[i0], require[i0] * 2)] + scen[1:]
    assert result_digest(ann.curate_scenarios(scen)) == result_digest(res)
    ms = ann.scenarios_ms()
    assert result_digest(ann.curate_scenarios(split)) == result_digest(res) and ann.scenarios_ms() == ms
    # ---- argument errors, all before any kernel ----
    oo = ann.orf_offsets()
    i = i0
    n_i = int(oo[i + 1] - oo[i])
    r0, r1 = require[i][0], require[i][1]
    ok = lambda **kw: raw_call(ann, **dict(dict(contig=[i], foff=[0, 0], forf=[0], roff=[0, 1], rorf=[r0], boff=[0, 1], borf=[r1], bval=[-500]), **kw))
    assert ok() == 0
    assert ok(boff=[0, 2], borf=[r1, r1], bval=[B_MAX + 7, -7]) == 0                          # the sum counts, not the parts
    assert ok(roff=[0, 3], rorf=[r0, r0, r1]) == 0                                           # duplicates in a required list
    ms_ok = ann.scenarios_ms()
    assert ok(foff=[0, 1], forf=[r0]) == E_ARG                                               # an ORF both refused and required
    assert "both refused and required" in ann.L.phx_last_error(ann.h).decode()
    assert ok(foff=[0, 1], forf=[r1]) == 0                                                   # ... refused and biased is fine: the refusal wins
    ms_ok = ann.scenarios_ms()
    assert ok(boff=[0, 2], borf=[r1, r1], bval=[(1 << 51) + 1, 1 << 51]) == E_ARG            # |B| > 2^52 after merging
    assert ok(bval=[-B_MAX - 1]) == E_ARG
    assert ok(contig=[ann.n]) == E_ARG and ok(contig=[-1]) == E_ARG                          # a contig outside the batch
    assert ok(borf=[n_i]) == E_ARG and ok(borf=[-1]) == E_ARG                                # an index outside its contig, each list
    assert ok(rorf=[n_i]) == E_ARG and ok(rorf=[-1]) == E_ARG
    assert ok(foff=[0, 1], forf=[n_i]) == E_ARG
    two = dict(contig=[i, i], foff=[0, 0, 0], roff=[0, 1, 1], boff=[0, 1, 1])
    assert ok(**two) == 0
    ms_ok = ann.scenarios_ms()
    for name in ("foff", "roff", "boff"):
        assert ok(**dict(two, **{name: [0, 1, 0]})) == E_ARG, name                           # offsets that decrease
        assert ok(**dict(two, **{name: [1, 1, 1]})) == E_ARG, name                           # ... or do not start at 0
    assert ok(roff=None) == E_ARG and ok(boff=None) == E_ARG and ok(unmet=False) == E_ARG    # require_off, bias_off and unmet must not be NULL
    assert ok(oo=oo + 1) == E_ARG
    assert ann.scenarios_ms() == ms_ok and ann.scenario_chunks() == 1                          # no kernel ran for a refused call
    with pytest.raises(pa.PhxError) as e:
        ann.curate_scenarios([(i, None, [r0], [r0])])
    assert e.value.code == E_ARG
    assert result_digest(ann.curate_scenarios(scen)) == result_digest(res) and everything() == before  # the refused calls left nothing behind
    # ---- the next upload invalidates the result ----
    ann.scenario_path(0, scen[0][0])
    ann.upload(b.seqs[:3])
    with pytest.raises(pa.PhxError) as e:
        ann.scenario_path(0, 0)
    assert e.value.code == E_STATE
    ann.close()


# ---- 8. the tie-scratch retry on a chunk of "both" slots ----
def test_both_slots_outgrow_the_tie_scratch(pa):
    found = large_ambiguous_contig()
    assert found is not None, "no large ambiguous contig among the candidates"
    seq, n_node, n_edge = found
    K = copies_that_outgrow(n_node, n_edge)
    assert K * tie_scratch_need(n_node, n_edge) >= 2 * TIE_SCRATCH_INITIAL
    ann = pa.Annotator()
    ann.upload([seq])
    ann.run()
    mst, moffs, mrec = ann.margins()
    pool = np.nonzero((mrec["called"] == 0) & (mrec["through"] == 1) & np.isfinite(mrec["margin"]))[0]
    assert len(pool) >= 2
    r, k = int(pool[0]), int(pool[-1])
    s = (0, [(k, 0.004)], None, [r])  # a required ORF and a penalty of four units on an uncalled one: a "both" slot that keeps the contig's ties
    one = ann.curate_scenarios([s])
    want = scenario_bytes(ann, one, 0, 0)
    assert want == lone(ann, s) and want[0] == 0
    fresh = pa.Annotator()  # (its scratch starts at the initial size)
    fresh.upload([seq])
    fresh.run()
    res = fresh.curate_scenarios([s] * K)
    assert fresh.scenario_chunks() == 1
    for j in range(K):
        assert scenario_bytes(fresh, res, j, 0) == want, j
    fresh.close()
    ann.close()


# ---- 9. curated_scan() and the CLI ----
def scan_expectation(ann, i, k, b, F, R):
    """One record of curated_scan() from two lone curate() calls."""
    def solve(bias):
        bb, f, r = [None] * ann.n, [None] * ann.n, [None] * ann.n
        bb[i], f[i], r[i] = bias, F, R
        st, offs, genes, delta, unmet = ann.curate(bb, f, r, solve_all=True)
        return int(st[i]), genes[offs[i]:offs[i + 1]].copy(), float(delta[i]), int(unmet[i])

    key = lambda g: (int(g["left"]), int(g["right"]), int(g["strand"]), int(g["frame"]))
    bst, bgenes, bdelta, bunmet = solve(None)
    st, genes, delta, unmet = solve([(k, b)])
    have, new = {key(g) for g in bgenes}, {key(g) for g in genes}
    o = ann.orfs(i)[k]
    fwd = o["frame"] > 0
    left, right = (int(o["start"]), int(o["stop"]) + 2) if fwd else (int(o["stop"]), int(o["start"]) + 2)
    me = lambda gs: int(any((int(g["left"]), int(g["right"]), g["strand"] > 0) == (left, right, bool(fwd)) and abs(int(g["frame"])) <= 3 for g in gs))
    return dict(left=left, right=right, strand=1 if fwd else -1, orf=k, bias=b, status=st, delta=delta, was_called=me(bgenes), called=me(genes), n_removed=len(have - new),
                n_added=len(new - have), unmet=unmet, base_status=bst, base_delta=bdelta, base_unmet=bunmet), genes.tobytes(), bgenes.tobytes()


def test_curated_scan_records_equal_lone_curate_calls(small):
    ann, b, draws, scen0, res0, chunks = small
    forbid, require, bias = sets_of(b, 2717)
    full = [i for i in b.idx if require[i]][:3]
    hits = [None] * b.n
    for i in full:
        pool, cg = b.reachable(i), b.called[i]
        hits[i] = [(pool[0], -25.0), (cg[-1], 3.5), (require[i][0], -1.0), (pool[-1], -400.0), (cg[0], -0.0004)]
    F = [forbid[i] if i in full else None for i in range(b.n)]
    R = [require[i] if i in full else None for i in range(b.n)]
    st, offs, rec, soffs, genes, boffs = ann.curated_scan(hits, F, R)
    assert st.tolist() == b.st0.tolist() and offs.tolist() == np.concatenate([[0], np.cumsum([len(h or []) for h in hits])]).tolist()
    assert len(rec) == offs[-1] and len(soffs) == len(rec) + 1 and len(boffs) == b.n + 1 and boffs[0] == soffs[-1] and boffs[-1] == len(genes)
    x = 0
    for i, h in enumerate(hits):
        if not h:
            assert boffs[i + 1] == boffs[i]
        for k, bb in h or []:
            want, gbytes, base_bytes = scan_expectation(ann, i, k, bb, F[i], R[i])
            got = {name: (float(rec[x][name]) if name in ("bias", "delta", "base_delta") else int(rec[x][name])) for name in rec.dtype.names}
            assert got == want, (i, k, bb)
            assert genes[soffs[x]:soffs[x + 1]].tobytes() == gbytes and genes[boffs[i]:boffs[i + 1]].tobytes() == base_bytes
            x += 1
    assert (rec["called"] != rec["was_called"]).any() and (rec["n_added"] > 0).any() and (rec["base_delta"] != 0).all()
    with pytest.raises(ValueError):
        ann.curated_scan(hits[:-1], F, R)


def test_cli_curated_scan(pa, tmp_path):
    from phanotate_amd.cli import format_curated_scan

    g, name, phix = load_golden("phiX174")
    fasta = tmp_path / "phix.fasta"
    fasta.write_text(">%s\n%s\n" % (name, phix))
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    ann = pa.Annotator()
    b = Batch(ann, [phix])
    orfs = ann.orfs(0)
    line = lambda k: "%d\t%d\t%s\t%s" % ((int(orfs[k]["start"]), int(orfs[k]["stop"]) + 2, "+", name) if orfs[k]["frame"] > 0 else (int(orfs[k]["start"]) + 2, int(orfs[k]["stop"]), "-", name))
    pool, cg = b.reachable(0), b.called[0]
    R, F = [pool[len(pool) // 2]], [cg[1]]
    ks = [pool[0], pool[-1], cg[0], R[0], pool[len(pool) // 3]]
    vals = [-30.0, -2.5, 1.25, -8.0, -600.0]
    ev, rq, fb = tmp_path / "ev.txt", tmp_path / "rq.txt", tmp_path / "fb.txt"
    ev.write_text("# hits\n" + "".join("%s\t%r\n" % (line(k), v) for k, v in zip(ks, vals)))
    rq.write_text(line(R[0]) + "\n")
    fb.write_text(line(F[0]) + "\n")
    out, re_out = tmp_path / "scan.txt", tmp_path / "re.txt"
    run = subprocess.run(exe + ["--require", str(rq), "--forbid", str(fb), "--reannotation", str(re_out), "--curated-scan", str(ev), str(out)], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    st, offs, rec, soffs, genes, boffs = ann.curated_scan([list(zip(ks, vals))], [F], [R])
    text = out.read_text()
    assert text == format_curated_scan([name], st, offs, rec)
    rows = text.splitlines()
    assert rows[0] == "#id:\t" + name and rows[1].startswith("#base:\t") and rows[2].endswith("\tUNMET") and len(rows) == 3 + len(ks)
    assert [r.split("\t")[:3] for r in rows[3:]] == [line(k).split("\t")[:3] for k in ks]
    cst, coffs, cgenes, cdelta, cunmet = ann.constrain([F], [R])
    assert cst[0] in (0, S_NEGCYCLE)
    assert rows[1] == "#base:\t%s\t%d" % (repr(float(cdelta[0])) if cst[0] == 0 else "cycle", int(cunmet[0]))
    assert cst[0] != 0 or "#delta:\t%r" % float(cdelta[0]) in re_out.read_text()
    ann.close()


# ---- 10. the golden fixtures ----
FIX = {}


@pytest.mark.parametrize("case", USABLE)
def test_the_combined_draws_of_a_fixture_in_one_call(pa, oracle, case):
    fx = fd.Fixture(case)
    og = fx.graph(oracle)
    ann = pa.Annotator(pa.make_params(**fx.params))
    try:
        st0, offs0, genes0 = run_batch(ann, [fx.seq], None if fx.trnas is None else [fx.trnas])
        assert st0[0] == 0
        ref = CuRef(ann, 0)
        D = ann.path(0)[1]
        draws = fd.draws(oracle, fx, og)
        assert len(draws) == 5 + (case in TRNA)
        idx = [indexed(ref, d) for d in draws]
        scen = [as_scen(0, B, F, R) for F, R, B in idx]
        res, got = equal_lone(ann, scen)
        count = dict(ok=0, cycle=0, nopath=0)
        for j, (F, R, B) in enumerate(idx):
            sol = ref.solve(F, R, B)
            check_scenario(ann, res, j, 0, sol, len(R), D)
            what = outcome(sol) if j < 5 else "directed_" + outcome(sol)  # (the sixth draw of a tRNA fixture is its directed one, counted apart)
            count[what] = count.get(what, 0) + 1
        FIX[case] = count
    finally:
        ann.close()


def test_the_fixtures_settle_as_the_host_test_counts():
    """tests/test_fixture_sweep_host.py, for the combined solve: of the 170 seeded draws 153 settle with a path and 17 meet a negative
    cycle, none is left without a path; the four directed draws of the tRNA fixtures settle."""
    assert sorted(FIX) == sorted(USABLE) and len(FIX) == 34
    tot = {w: sum(c.get(w, 0) for c in FIX.values()) for w in ("ok", "cycle", "nopath", "directed_ok", "directed_cycle", "directed_nopath")}
    assert tot == dict(ok=153, cycle=17, nopath=0, directed_ok=len(TRNA), directed_cycle=0, directed_nopath=0), tot
