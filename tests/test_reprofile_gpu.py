"""Re-annotation profiles on the device (phx_reprofile_flat) against python integers.  The yardstick is EvRef.solve(forbid,
bias) of tests/test_evidence_gpu.py: its `dist` is d_s', its `edges` are G''s edges with W + B, d_t' comes from py_dt_in_R of
tests/test_remargins_gpu.py; track and slot range per edge follow test_profile_gpu.edge_deltas, and the per-slot minimum (paint_min) is
compared bit for bit with the record, lo / hi included.  No tolerance enters.  Then the invariants, the wide classes, statuses, the
identity with profile(), isolation and the cache, and an inequality through the solver itself."""
import numpy as np
import pytest

from test_evidence_gpu import NEGCYCLE, EvRef, called_orfs, draw_orfs, evidence, solved_contigs
from test_profile_gpu import TRACKS, check_bounds, check_invariants, is_open, paint_min, rank
from test_reannotate_gpu import fuzz, mask_rounds, run_batch, wide_cases
from test_remargins_gpu import cycle_orf, draw_penalties, py_dt_in_R, some_evidence
from test_scenarios_gpu import case1_seqs

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def cells(n):
    return n * n.bit_length()  # n (floor(log2 n) + 1): one track's table


def out_bytes(out, i=None):
    st, offs, rec = out
    if i is None:
        return st.tobytes(), offs.tobytes(), rec.tobytes()
    return int(st[i]), rec[offs[i]:offs[i + 1]].tobytes()


def edge_deltas_cond(ref, DB, dist, dt, edges):
    """test_profile_gpu.edge_deltas on G': [(track, Delta', a, z)] of every edge that takes part (u and v reached on their sides)"""
    V, nd = ref.V, ref.nd
    out = []
    for u, v, w in edges:
        ou, ov = is_open(nd, u, V), is_open(nd, v, V)
        assert ou != ov and u != V - 1 and v != V - 2, (ref.i, u, v)
        if dist[u] is None or dt[v] is None:
            continue
        track = 2 if not ou else (0 if int(nd["frame"][u]) > 0 else 1)
        delta = dist[u] + w + dt[v] - DB
        assert delta >= 0, (ref.i, u, v, delta)  # inside R (§21's lemma)
        out.append((track, delta, rank(u, V) + 1, rank(v, V)))
    return out


def check_contig(ann, ref, L, forbid, bias, st, rec):
    """One contig's records against the yardstick, every value of every slot bit for bit; returns NEGCYCLE, None (no path) or D'."""
    i = ref.i
    sol = ref.solve(forbid or [], bias)
    if sol == NEGCYCLE:
        assert st == -9 and len(rec) == 0, (i, forbid, bias, st)
        return NEGCYCLE
    DB, path, genes, dist, edges = sol
    check_bounds(ann, i, L, rec)  # V - 1 records, lo / hi
    n = ref.V - 1
    if DB is None:
        assert st == 1 and all(np.isinf(rec[k]).all() for k in TRACKS), (i, forbid, bias, st)
        return None
    assert st == 0, (i, forbid, bias, st)
    dt = py_dt_in_R(ref.V, edges, dist)
    items = ([], [], [])
    for track, delta, a, z in edge_deltas_cond(ref, DB, dist, dt, edges):
        if a <= z:
            items[track].append((delta, a, z))
    for t, name in enumerate(TRACKS):
        want = np.array([INF if d is None else float(d) / 1000.0 for d in paint_min(n, items[t])])
        assert want.tobytes() == rec[name].astype(np.float64).tobytes(), (i, name, forbid, bias, np.flatnonzero(want != rec[name])[:5])
    return DB


def check_batch(ann, refs, lens, forbid, bias, run_profile=None):
    """evidence(bias, forbid) — reannotate(forbid) where there is no bias —, reprofile(), every contig of refs with a refusal or a bias
    against the yardstick; with run_profile, the others against the run's records."""
    n = ann.n
    if bias is None:
        st, offs, genes, delta = ann.reannotate(forbid)
    else:
        st, offs, genes, delta = evidence(ann, bias, forbid)
    out = ann.reprofile()
    pst, poffs, prec = out
    assert poffs[0] == 0 and poffs[-1] == len(prec)
    got = {}
    for i in range(n):
        f = None if forbid is None else forbid[i]
        b = None if bias is None else bias[i]
        if f is None and b is None:
            if run_profile is not None:
                assert out_bytes(out, i) == out_bytes(run_profile, i), i  # not solved again: the run's records, byte for byte
            continue
        if i not in refs:
            continue
        got[i] = check_contig(ann, refs[i], lens[i], f, b, int(pst[i]), prec[poffs[i]:poffs[i + 1]])
        assert int(pst[i]) == int(st[i]), i
    return got


@pytest.fixture(scope="module")
def big(pa):
    """§21's batch, case1_seqs + fuzz(11, 6), run once (179 to 1004 nodes): tables in LDS and in global memory.  (ann, lengths, yardsticks,
    the run's D, the called ORFs, the run's profile.)  The tests leave the batch resident."""
    ann = pa.Annotator()
    seqs = case1_seqs(pa) + fuzz(11, 6)
    dl = run_batch(ann, seqs)
    idx = solved_contigs(ann, dl[0])
    V = {i: int(ann.globals(i).n_node) for i in idx}
    print("nodes per contig:", sorted(V.items()))
    assert any(cells(v - 1) <= 4096 for v in V.values()) and any(cells(v - 1) > 4096 for v in V.values()), sorted(V.items())  # both table placements occur
    refs = {i: EvRef(ann, i) for i in idx}
    called = {i: called_orfs(ann, i, dl[2][dl[1][i]:dl[1][i + 1]]) for i in idx}
    run_profile = tuple(np.copy(x) for x in ann.profile())
    yield ann, [len(s) for s in seqs], refs, {i: ann.path(i)[1] for i in idx}, called, run_profile
    ann.close()


# ---- 1. the batch: masks, penalties alone and with a mask, bonuses ----
def test_masks_against_the_yardstick(big):
    ann, lens, refs, D, called, run_profile = big
    n = ann.n
    rng = np.random.RandomState(2101)
    order = sorted(refs)
    plans = dict(zip(order, mask_rounds([refs[i] for i in order], [called[i] for i in order], rng)))
    have = [i for i in order if called[i]]
    assert len(have) >= len(order) - 1 and all(plans[i] for i in have)
    few = [sorted(rng.choice(called[i], min(len(called[i]), int(rng.randint(1, 4))), replace=False).tolist()) if i in have else None for i in range(n)]
    sets = [plans[i][-1] if i in have else None for i in range(n)]
    seen = 0
    for forbid in (few, sets):  # 1-3 called genes; mask_rounds' draw: 1-5 % of the ORFs with a called gene among them
        got = check_batch(ann, refs, lens, forbid, None, run_profile)
        assert set(got) == set(have) and NEGCYCLE not in got.values()  # no drawn point is skipped
        seen += sum(g is not None for g in got.values())
        for i, g in got.items():
            assert g is None or g >= D[i]
    assert seen >= 2 * len(refs) - 2, seen


def test_penalties_alone_and_with_a_mask(big):
    ann, lens, refs, D, called, run_profile = big
    bias, forbid = draw_penalties(ann, refs, called, np.random.RandomState(2102))
    assert any(f for f in forbid)
    for fb in (None, forbid):
        got = check_batch(ann, refs, lens, fb, bias, run_profile)
        assert set(got) == set(refs) and NEGCYCLE not in got.values()  # a penalty cannot make a cycle negative: no drawn point is skipped
        assert all(g is None or g >= D[i] for i, g in got.items())
        assert sum(g is not None for g in got.values()) >= len(refs) - 1


def test_bonuses_of_the_titration_draw(big):
    ann, lens, refs, D, called, run_profile = big
    n = ann.n
    idx = sorted(refs)
    mst, moffs, mrec = ann.margins()
    rng = np.random.RandomState(1904)
    picks = {}
    for i in idx:
        rec = mrec[moffs[i]:moffs[i + 1]]
        ok = [k for k in range(len(rec)) if rec["through"][k] == 1 and rec["called"][k] == 0 and np.isfinite(rec["margin"][k]) and round(float(rec["margin"][k]) * 1000) < 1 << 50]
        take = sorted(rng.choice(ok, min(len(ok), 10 if i >= 3 else 4), replace=False).tolist())
        picks[i] = [(k, int(round(float(rec["margin"][k]) * 1000))) for k in take]
    points = 0
    for r in range(max(len(p) for p in picks.values())):
        bias = [{picks[i][r][0]: -picks[i][r][1] - 1} if i in picks and r < len(picks[i]) else None for i in range(n)]
        got = check_batch(ann, refs, lens, None, bias, run_profile)
        assert NEGCYCLE not in got.values() and None not in got.values(), (r, got)  # (none of the draw's points lies on a negative cycle)
        for i, DB in got.items():
            assert DB == D[i] - 1, (i, r)  # the bonus wins by one unit
        points += len(got)
    print("bonuses: %d points of the titration draw" % points)
    assert points == sum(len(p) for p in picks.values()) >= 60  # no drawn point is skipped


# ---- 2. invariants ----
def test_invariants_on_every_solved_contig(big):
    ann, lens, refs, D, called, run_profile = big
    bias, forbid = draw_penalties(ann, refs, called, np.random.RandomState(2105))
    st, offs, genes, delta = evidence(ann, bias, forbid)
    pst, poffs, prec = ann.reprofile()
    mst, moffs, mrec = ann.remargins()
    assert pst.tolist() == mst.tolist() == st.tolist()
    seen = genes_refused = rose = 0
    for i in refs:
        if pst[i] != 0:
            continue
        rec, mr = prec[poffs[i]:poffs[i + 1]], mrec[moffs[i]:moffs[i + 1]]
        # values >= 0, min over the tracks 0 on every slot, the gene tracks the slice minima of the remargins() records with through == 1
        check_invariants(ann, i, lens[i], 0, rec, mr)
        seen += 1
        # a refused called gene gives its strand's track nothing: where the track is still 0 inside the gene another ORF of the strand
        # with margin 0 covers the slot, and nowhere else
        ref = refs[i]
        for k in forbid[i] or []:
            e = ref.orf_edge[k]
            if e is None or k not in called[i]:
                continue
            assert mr["through"][k] == 0
            s = 1 if ref.orfs[k]["frame"] > 0 else -1
            name = "fwd" if s > 0 else "rev"
            a, z = e[0] + 1, e[1]  # its slots
            before = run_profile[2][run_profile[1][i]:run_profile[1][i + 1]][name][a:z + 1]
            assert (before == 0.0).all(), (i, k)  # the run called it
            others = np.zeros(z + 1 - a, bool)
            for k2 in np.flatnonzero((mr["through"] == 1) & (mr["margin"] == 0.0) & (mr["strand"] == s)).tolist():
                e2 = ref.orf_edge[k2]
                if e2 is None:
                    continue
                lo, hi = max(a, e2[0] + 1), min(z, e2[1])
                if lo <= hi:
                    others[lo - a:hi + 1 - a] = True
            assert ((rec[name][a:z + 1] == 0.0) == others).all(), (i, k)
            genes_refused += 1
            rose += bool((rec[name][a:z + 1] > 0.0).any())
    print("invariants: %d contigs, %d refused called genes, %d of them with a slot whose track rose above 0" % (seen, genes_refused, rose))
    # every second contig of the draw has a refused called gene (every fourth call, the biased ones left out).  A replacement covers each
    # of a refused gene's slots on the same strand at margin 0 only by a tie or by a longer variant of the same stop: over the batch's
    # refused genes at least one loses a slot
    assert seen >= len(refs) - 1 and genes_refused >= len(refs) // 2 and rose >= 1


# ---- 3. the wide classes ----
@pytest.mark.parametrize("case", range(4))
def test_a_mask_and_a_penalty_in_the_wide_classes(pa, case):
    seqs, nl = wide_cases(pa)[case]
    ann = pa.Annotator()
    dl = run_batch(ann, seqs)
    want = (4, 8, 8, 17)[case]  # 256, 512, 512 and 1088 bits
    i = next(i for i in range(len(seqs)) if dl[0][i] == 0 and int(ann.globals(i).n_limbs) == want)
    refs = {i: EvRef(ann, i)}
    lens = [len(s) for s in seqs]
    cg = called_orfs(ann, i, dl[2][dl[1][i]:dl[1][i + 1]])
    rng = np.random.RandomState(2106 + case)
    forbid = [None] * len(seqs)
    forbid[i] = [cg[int(rng.randint(len(cg)))]]
    run_profile = tuple(np.copy(x) for x in ann.profile())
    got = check_batch(ann, refs, lens, forbid, None, run_profile)
    assert got[i] is not NEGCYCLE
    bias = [None] * len(seqs)
    bias[i] = {k: int(10 ** rng.uniform(1, 6)) for k in draw_orfs(refs[i], cg, rng, 6)}
    got = check_batch(ann, refs, lens, None, bias, run_profile)
    assert got[i] not in (NEGCYCLE, None)
    ann.close()


# ---- 4. statuses ----
def test_statuses_in_one_mixed_batch(pa):
    cand = fuzz(11, 12)
    probe = pa.Annotator()
    st0 = run_batch(probe, cand)[0]
    rng = np.random.RandomState(1905)
    neg = None
    for i in rng.permutation(solved_contigs(probe, st0)).tolist():
        k = cycle_orf(EvRef(probe, i))
        if k is not None:
            neg = (cand[i], k)
            break
    probe.close()
    assert neg is not None
    good = [pa.synth_contig(322, 9000).decode(), pa.synth_contig(323, 7000).decode()]
    bad = pa.synth_contig(324, 3000).decode()[:1500] + "x" + pa.synth_contig(324, 3000).decode()[1500:]
    seqs = [bad, "acg", pa.synth_contig(410, 6000), neg[0], good[0], good[1]]  # a bad letter, too short, a mask that leaves no path, a negative cycle, two plain
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    with pytest.raises(pa.PhxError) as e:  # before any re-annotation of the run
        ann.reprofile()
    assert e.value.code == -13
    assert st0.tolist() == [-2, -3, 0, 0, 0, 0]
    forbid = [None, None, np.arange(len(ann.orfs(2))), None, None, None]
    bias = [None, None, None, {neg[1]: -10 ** 9}, None, None]
    for i in (4, 5):
        bias[i] = {called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])[0]: 4000, 3: -2500}
    st, offs, genes, delta = evidence(ann, bias, forbid)
    assert st.tolist() == [-2, -3, 1, -9, 0, 0]
    pst, poffs, prec = ann.reprofile()
    assert pst.tolist() == [-2, -3, 1, -9, 0, 0]
    V = [int(ann.globals(i).n_node) for i in range(6)]
    assert np.diff(poffs).tolist() == [0, 0, V[2] - 1, 0, V[4] - 1, V[5] - 1] and V[2] > 2
    nopath = prec[poffs[2]:poffs[3]]
    assert all(np.isinf(nopath[k]).all() for k in TRACKS)  # no path: V - 1 records, every value +inf ...
    check_bounds(ann, 2, len(seqs[2]), nopath)  # ... with their bounds
    for k, i in enumerate((4, 5)):  # the neighbours are unaffected
        assert check_contig(ann, EvRef(ann, i), len(seqs[i]), None, bias[i], int(pst[i]), prec[poffs[i]:poffs[i + 1]]) not in (None, NEGCYCLE)
        lone = pa.Annotator()
        run_batch(lone, [good[k]])
        evidence(lone, [bias[i]])
        assert out_bytes(lone.reprofile(), 0) == out_bytes((pst, poffs, prec), i)
        lone.close()
    # not solved again: the run's records, byte for byte
    ann.reannotate([None] * 6)
    got, want = ann.reprofile(), ann.profile()
    assert got[0].tolist() == want[0].tolist() == [-2, -3, 0, 0, 0, 0]
    assert out_bytes(got) == out_bytes(want) and len(got[2]) == sum(v - 1 for v in V[2:])
    # required ORFs on any contig: PHX_E_STATE, and the text says why
    req = [None] * 6
    req[5] = [called_orfs(ann, 5, genes0[offs0[5]:offs0[6]])[0]]
    ann.constrain(require=req)
    with pytest.raises(pa.PhxError) as e:
        ann.reprofile()
    assert e.value.code == -13 and "required" in str(e.value)
    ann.constrain(forbid=req)  # nothing required: phx_constrain_flat serves too
    assert ann.reprofile()[0].tolist() == [-2, -3, 0, 0, 0, 0]
    ann.close()


# ---- 5. identity ----
def test_nothing_refused_no_bias_is_profile_byte_for_byte(big):
    ann, lens, refs, D, called, run_profile = big
    n = ann.n
    cert = ann.certified()
    ann.reannotate([None] * n, solve_all=True)  # every contig is solved again
    got = ann.reprofile()
    assert got[0].tolist() == run_profile[0].tolist() and got[1].tolist() == run_profile[1].tolist()
    seen = 0
    for i in range(n):
        if cert[i] == 1 and run_profile[0][i] >= 0:
            assert out_bytes(got, i) == out_bytes(run_profile, i), i
            seen += run_profile[1][i + 1] > run_profile[1][i]
    assert seen >= len(refs) // 2, seen
    assert ann.reprofile_ms()["tables"] > 0  # (the conditioned kernels computed them: nothing was copied from the run's set)


# ---- 6. isolation and the cache ----
def test_reprofile_disturbs_nothing_is_cached_and_invalidated(pa):
    seqs = fuzz(31, 20)
    a, b = pa.Annotator(), pa.Annotator()
    for x in (a, b):
        run_batch(x, seqs)
    bias, forbid = some_evidence(a, 2108)

    def others(ann):
        return [out_bytes(f()) for f in (ann.profile, ann.margins, ann.remargins, ann.redrops)]

    # a: everything else first, then reprofile(); b: reprofile() first
    evidence(a, bias, forbid)
    assert a.reprofile_ms() == dict(tables=0.0, records=0.0, download=0.0)
    before = others(a)
    r1 = out_bytes(a.reprofile())
    ms = a.reprofile_ms()
    assert ms["tables"] > 0
    assert others(a) == before  # the same bytes after it
    assert out_bytes(a.reprofile()) == r1 and a.reprofile_ms() == ms  # the cached records: nothing was computed again
    evidence(b, bias, forbid)
    assert out_bytes(b.reprofile()) == r1 and others(b) == before  # ... whichever runs first
    evidence(a, bias, forbid)  # the same re-annotation hits its cache and keeps the profile
    assert out_bytes(a.reprofile()) == r1 and a.reprofile_ms() == ms
    assert r1 != out_bytes(a.profile())
    # a new evidence() invalidates it
    bias2, forbid2 = some_evidence(a, 2109)
    evidence(a, bias2, forbid2)
    evidence(b, bias2, forbid2)
    r2 = out_bytes(a.reprofile())
    assert r2 != r1 and r2 == out_bytes(b.reprofile())
    b.close()
    # ... and so does a new run
    other = fuzz(32, 6)
    a.upload(other)
    with pytest.raises(pa.PhxError) as e:
        a.reprofile()
    assert e.value.code == -13
    a.run()
    with pytest.raises(pa.PhxError) as e:
        a.reprofile()
    assert e.value.code == -13
    fresh = pa.Annotator()
    run_batch(fresh, other)
    bias, forbid = some_evidence(fresh, 2110)
    evidence(a, bias, forbid)
    evidence(fresh, bias, forbid)
    assert out_bytes(a.reprofile()) == out_bytes(fresh.reprofile())
    for x in (a, fresh):
        x.close()


# ---- 7. through the solver ----
def test_refusing_every_gene_over_a_slot_costs_at_least_its_gap_value(big):
    """With every ORF whose gene edge covers slot s refused on top of the re-annotation, the best path crosses s by a connector (the batch
    has no tRNA edges), so D'' - D' >= the slot's minimum connector Delta' — the record's gap, in integer units.  A walk may cross a slot
    more than once, so equality is not a law."""
    ann, lens, refs, D, called, run_profile = big
    n = ann.n
    idx = sorted(refs)
    B0, F0 = draw_penalties(ann, refs, called, np.random.RandomState(2102))
    st, offs, genes, delta = evidence(ann, B0, F0)
    ok = [i for i in idx if st[i] == 0]
    assert len(ok) >= len(idx) - 1
    D1 = {i: ann.reannotated_path(i)[1] for i in ok}
    pst, poffs, prec = ann.reprofile()
    gap = {i: np.copy(prec[poffs[i]:poffs[i + 1]]["gap"]) for i in ok}
    for i in ok:
        assert not (np.abs(refs[i].nd["frame"][: refs[i].V - 2].astype(int)) == 4).any()  # no tRNA nodes: every gene edge is an ORF edge
    rng = np.random.RandomState(3607)
    points = equal = nopath = 0
    for r in range(3):
        slot = {i: int(rng.randint(len(gap[i]))) for i in ok}
        forbid = []
        for i in range(n):
            if i not in slot:
                forbid.append(F0[i])
                continue
            V = refs[i].V
            over = [k for k, e in enumerate(refs[i].orf_edge) if e is not None and rank(e[0], V) + 1 <= slot[i] <= rank(e[1], V)]
            forbid.append(sorted(set(F0[i] or []) | set(over)))
        st2, offs2, genes2, delta2 = evidence(ann, B0, forbid)
        for i, s in slot.items():
            g = float(gap[i][s])
            points += 1
            assert st2[i] in (0, 1), (i, s, st2[i])  # (removing edges makes no cycle negative)
            if st2[i] == 1:
                nopath += 1
                continue
            assert np.isfinite(g), (i, s)  # a path of G'' crosses s by a connector both of whose ends G' reaches
            if round(g * 1000) >= 1 << 50:
                continue
            D2 = ann.reannotated_path(i)[1]
            assert D2 - D1[i] >= int(round(g * 1000)), (i, s, D2 - D1[i], g)
            equal += D2 - D1[i] == int(round(g * 1000))
    print("through the solver: %d points, %d equalities, %d without a path" % (points, equal, nopath))
    assert points >= 3 * (len(idx) - 1) and points - nopath >= points // 2
