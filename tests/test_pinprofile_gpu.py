"""Pinned profiles on the device (phx_pinprofile_flat, Annotator.pinprofile) against python integers.  The yardstick is
pin_ref's construction (tests/test_pinmargins_gpu.py): CuRef's edges with W + B - M·[required], test_evidence_gpu.settle for d_s', then
py_dt_in_R for d_t' — applied to EVERY edge, with track and slot range per edge as test_reprofile_gpu.edge_deltas_cond has them, and a
lexicographic paint_min on (lost, s).  `value` is compared bit for bit, `lost` entry by entry, lo / hi included.  No tolerance enters.
Then the invariants, the wide classes, both reductions, statuses, isolation and the cache, and an inequality through the solver itself."""
import os

import numpy as np
import pytest

from conftest import ROOT
from test_constrain_gpu import bytes_of, fuzz, run_batch, wide_cases
from test_curate_gpu import Batch, CuRef, DeviceGraph, NoGraph, curate, evidence, sets_of
from test_evidence_gpu import settle
from test_pinmargins_gpu import split
from test_pinprofile_host import mu_of, neighbour_pins
from test_profile_gpu import TRACKS, check_bounds, is_open, paint_min, rank
from test_remargins_gpu import py_dt_in_R

import curate_draws as cd

pytestmark = pytest.mark.gpu

E_STATE, S_NEGCYCLE, S_NOPATH = -13, -9, 1
INF = float("inf")


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def cells(n):
    return n * n.bit_length()  # n (floor(log2 n) + 1): one track's table


@pytest.fixture(scope="module")
def small(pa):
    """curate_draws.mix_seqs, run once, as tests/test_pinmargins_gpu.py has it: one contig of 179 nodes, the others 272-1004 — a table in
    LDS and tables in global memory, a reverse pass of one chunk and of several.  The tests leave the batch resident."""
    ann = pa.Annotator()
    b = Batch(ann, cd.mix_seqs(pa))
    V = sorted(int(ann.globals(i).n_node) for i in b.idx)
    print("nodes per contig:", V)
    assert len(b.idx) >= 8 and V[0] <= 256 and V[-1] > 768
    assert any(cells(v - 1) <= 4096 for v in V) and any(cells(v - 1) > 4096 for v in V), V  # both table placements occur
    b.run_profile = tuple(np.copy(x) for x in ann.profile())
    yield b
    ann.close()


# ---- the yardstick ----
def prof_ref(ref, forbid, require, bias):
    """dict(cycle=True), dict(cycle=False, D=None), or per track and slot the lexicographic minimum (lost, s) over the covering edges of
    G' that take part (None: none), with the solve's (count, S)."""
    gone = {ref.orf_edge[k] for k in forbid or ()} - {None}
    pinned = {ref.orf_edge[k] for k in require or ()} - {None} - gone
    add = {}
    for k, B in (bias or {}).items():
        if ref.orf_edge[k] is not None:
            add[ref.orf_edge[k]] = add.get(ref.orf_edge[k], 0) + B
    M = 1 << ((sum(abs(w) for _, _, w in ref.edges) + sum(abs(B) for B in add.values())).bit_length() + 2)
    edges = [(u, v, w + add.get((u, v), 0) - (M if (u, v) in pinned else 0)) for u, v, w in ref.edges if (u, v) not in gone]
    V, nd = ref.V, ref.nd
    dist, par = settle(V, edges, V - 2)
    if dist is None:
        return dict(cycle=True)
    if dist[V - 1] is None:
        return dict(cycle=False, D=None)
    dt = py_dt_in_R(V, edges, dist)
    assert dt[V - 2] == dist[V - 1]
    D = dist[V - 1]
    items = ([], [], [])
    for u, v, w in edges:
        ou, ov = is_open(nd, u, V), is_open(nd, v, V)
        assert ou != ov and u != V - 1 and v != V - 2, (ref.i, u, v)
        if dist[u] is None or dt[v] is None:  # unreached on its side: no part
            continue
        x = dist[u] + w + dt[v] - D
        assert x >= 0, (ref.i, u, v, x)  # inside R_n, connectors included
        s, c = split(x, M)
        a, z = rank(u, V) + 1, rank(v, V)
        if a <= z:
            items[2 if not ou else (0 if int(nd["frame"][u]) > 0 else 1)].append(((-c, s), a, z))
    S, count = split(D, M)
    return dict(cycle=False, D=D, S=S, count=count, M=M, tracks=[paint_min(V - 1, it) for it in items])


def check_prof(ann, ref, L, forbid, require, bias, st, rec, lost):
    """One pinned contig's records and `lost` against the yardstick, every value of every slot bit for bit; returns the yardstick's dict."""
    i = ref.i
    what = (i, list(forbid or ()), list(require or ()), bias)
    sol = prof_ref(ref, forbid, require, bias)
    if sol["cycle"]:
        assert st == S_NEGCYCLE and len(rec) == 0 and len(lost) == 0, (what, st)
        return sol
    check_bounds(ann, i, L, rec)  # V - 1 records, lo / hi
    assert lost.shape == (ref.V - 1, 3), what
    if sol["D"] is None:
        assert st == S_NOPATH and all(np.isinf(rec[k]).all() for k in TRACKS) and not lost.any(), (what, st)
        return sol
    assert st == 0, (what, st)
    for t, name in enumerate(TRACKS):
        want = np.array([INF if p is None else mu_of(p[1]) for p in sol["tracks"][t]])
        wl = np.array([0 if p is None else p[0] for p in sol["tracks"][t]], np.int32)
        assert want.tobytes() == rec[name].astype(np.float64).tobytes(), (what, name, np.flatnonzero((want != rec[name]) | (wl != lost[:, t]))[:5])
        assert np.array_equal(wl, lost[:, t]), (what, name, np.flatnonzero(wl != lost[:, t])[:5])
    return sol


def prof_batch(b, bias, forbid, require):
    """curate(), pinprofile(), every contig with a required ORF against the yardstick: {contig: the yardstick's dict}, the two results."""
    ann = b.ann
    res = curate(ann, bias, forbid, require)
    st = res[0]
    pp = pst, poffs, prec, lost = ann.pinprofile()
    assert poffs[0] == 0 and poffs[-1] == len(prec) == len(lost)
    out = {}
    for i in b.idx:
        if not (require and require[i]):
            continue
        out[i] = check_prof(ann, b.refs[i], len(b.seqs[i]), forbid and forbid[i], require[i], bias and bias[i], int(pst[i]), prec[poffs[i]:poffs[i + 1]], lost[poffs[i]:poffs[i + 1]])
        assert int(pst[i]) == int(st[i]), i
    return out, res, pp


def settled(sol):
    return not sol["cycle"] and sol["D"] is not None


def part(out, i):
    """what one contig got: its status, records and `lost`, as bytes"""
    st, offs, rec = out[:3]
    return int(st[i]), rec[offs[i]:offs[i + 1]].tobytes(), out[3][offs[i]:offs[i + 1]].tobytes() if len(out) > 3 else None


# ---- 1. the seeded mixes and this file's own draw ----
@pytest.fixture(scope="module")
def mixed(small):
    """The 45 seeded mixes, round by round, and the host file's own draw (neighbour_pins) as a sixth round: every draw checked against
    the yardstick, then per settled contig what the invariants need.  [(round, contig, yardstick, draw's index lists, records, lost,
    the contig's pinmargins() records and lost)]"""
    b, ann = small, small.ann
    graphs = [DeviceGraph(b.refs[i], b.called[i]) if i in b.refs else NoGraph() for i in range(b.n)]
    rows = cd.mixes(graphs) + [[neighbour_pins(g) if g.ok else None for g in graphs]]
    assert len(rows) == cd.ROUNDS + 1
    out = []
    for rnd, row in enumerate(rows):
        forbid, require, bias = [None] * b.n, [None] * b.n, [None] * b.n
        for i, d in enumerate(row):
            if d is not None:
                by = b.refs[i].by_ends
                forbid[i], require[i], bias[i] = [by[k] for k in d["forbid"]], [by[k] for k in d["require"]], {by[k]: B for k, B in d["bias"].items()}
        sols, res, (pst, poffs, prec, lost) = prof_batch(b, bias, forbid, require)
        assert len(sols) == sum(d is not None for d in row)  # no drawn point is skipped
        mst, moffs, mrec, mlost = ann.pinmargins()
        for i, sol in sols.items():
            out.append((rnd, i, sol, (forbid[i], require[i], bias[i]), np.copy(prec[poffs[i]:poffs[i + 1]]), np.copy(lost[poffs[i]:poffs[i + 1]]),
                        np.copy(mrec[moffs[i]:moffs[i + 1]]), np.copy(mlost[moffs[i]:moffs[i + 1]])))
    return out


def test_the_seeded_mixes_against_the_yardstick(mixed):
    """Every draw was compared field by field or, with a required ORF on a reachable cycle, checked as PHX_S_NEGCYCLE without records
    (check_prof).  tests/test_pinprofile_host.py counts 45 of 45 that settle on the oracle's graphs."""
    seeded = [m for m in mixed if m[0] < cd.ROUNDS]
    assert len(seeded) == 45
    compared = sum(settled(m[2]) for m in seeded)
    cycles = sum(m[2]["cycle"] for m in seeded)
    print("seeded mixes: %d draws, %d compared field by field, %d on a cycle" % (len(seeded), compared, cycles))
    assert compared >= 40
    own = [m for m in mixed if m[0] == cd.ROUNDS]
    assert len(own) >= 5 and sum(settled(m[2]) for m in own) >= 5


def test_histogram_of_lost_on_the_devices_graphs(mixed):
    hist, negative, two = [{}, {}, {}], 0, 0
    for rnd, i, sol, sets, rec, lost, mrec, mlost in mixed:
        if not settled(sol):
            continue
        for t, name in enumerate(TRACKS):
            have = np.isfinite(rec[name]) | (lost[:, t] > 0)
            for l, c in zip(*np.unique(lost[have, t], return_counts=True)):
                hist[t][int(l)] = hist[t].get(int(l), 0) + int(c)
            negative += int((rec[name] < 0).sum())
            two += int((lost[:, t] >= 2).sum())
    print("slots by their minimum lost, fwd: %s rev: %s gap: %s; %d with a negative value, %d with lost >= 2" % (*[sorted(h.items()) for h in hist], negative, two))
    assert all(h.get(1, 0) > 0 for h in hist), hist  # lost = 1 on each of the three tracks
    assert negative > 0 and two > 0, (negative, two)
    assert all(max(h) >= 2 for h in hist), hist  # (with the host file's own draw: on each track)


# ---- 2. invariants ----
def test_invariants_on_every_settled_pinned_contig(small, mixed):
    b, ann = small, small.ann
    seen = kept_pins = 0
    for rnd, i, sol, (forbid, require, bias), rec, lost, mrec, mlost in mixed:
        if not settled(sol):
            continue
        seen += 1
        vals = np.stack([rec[k] for k in TRACKS])
        assert not np.isnan(vals).any() and (lost >= 0).all() and (vals[lost.T == 0] >= 0).all(), (rnd, i)
        # the minimum over the tracks is (0, 0.0): the re-annotation's path crosses every slot
        pairs = [min((int(lost[x, t]), float(vals[t, x])) for t in range(3)) for x in range(len(rec))]
        assert all(p == (0, 0.0) for p in pairs), (rnd, i)
        # the gene tracks are the lexicographic slice minima of the pinmargins() records with through == 1 (no tRNA nodes in this batch)
        ref = b.refs[i]
        V, nd = ref.V, ref.nd
        assert not (np.abs(nd["frame"][: V - 2].astype(int)) == 4).any()
        want = [[None] * (V - 1) for _ in range(2)]
        for k in np.flatnonzero(mrec["through"] == 1).tolist():
            u, v = ref.orf_edge[k]
            row, p = want[0 if mrec["strand"][k] > 0 else 1], (int(mlost[k]), float(mrec["margin"][k]))
            for x in range(u + 1, v + 1):
                if row[x] is None or p < row[x]:
                    row[x] = p
        for t in range(2):
            got = [None if np.isinf(vals[t, x]) and lost[x, t] == 0 else (int(lost[x, t]), float(vals[t, x])) for x in range(V - 1)]
            assert got == want[t], (rnd, i, t, [x for x in range(V - 1) if got[x] != want[t][x]][:5])
        # the slots inside a kept required gene have (0, 0.0) on its own strand's track
        for k in require:
            if mrec["called"][k] == 1:
                u, v = ref.orf_edge[k]
                t = 0 if mrec["strand"][k] > 0 else 1
                assert (vals[t, u + 1:v + 1] == 0.0).all() and not lost[u + 1:v + 1, t].any(), (rnd, i, k)
                kept_pins += 1
    print("invariants: %d settled pinned contigs, %d kept required genes" % (seen, kept_pins))
    assert seen >= 45 and kept_pins >= seen // 2  # (40 of the seeded mixes and 5 of the own draw at least; the own draw alone pins two called genes per contig)


# ---- 3. constrain() alone, curate() with a bias ----
def test_constrain_alone_and_curate_with_a_bias(small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 3710)
    assert sum(r is not None for r in require) >= 6
    ann.constrain(forbid, require)  # mode 2
    pst, poffs, prec, lost = ann.pinprofile()
    seen = 0
    for i in b.idx:
        if require[i]:
            seen += settled(check_prof(ann, b.refs[i], len(b.seqs[i]), forbid[i], require[i], None, int(pst[i]), prec[poffs[i]:poffs[i + 1]], lost[poffs[i]:poffs[i + 1]]))
        else:  # the run's result stands: profile()'s records, lost 0
            assert part((pst, poffs, prec, lost), i)[:2] == part(b.run_profile, i)[:2] and not lost[poffs[i]:poffs[i + 1]].any()
    assert seen >= 5
    sols, _, _ = prof_batch(b, bias, forbid, require)  # mode 4
    assert sum(settled(s) for s in sols.values()) >= 5


# ---- 4. a batch of modes 0 - 4, both reductions, and reprofile()'s refusal ----
def test_a_batch_of_every_mode_and_both_reductions(pa, small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 3711)
    full = [i for i in b.idx if require[i]]
    assert len(full) >= 6
    role = {full[0]: 0, full[1]: 1, full[2]: 2, full[3]: 3}  # the run's result, refused only, required only, biased only; the others all three
    F = [forbid[i] if role.get(i, 4) in (1, 4) and i in full else None for i in range(b.n)]
    R = [require[i] if role.get(i, 4) in (2, 4) and i in full else None for i in range(b.n)]
    Bs = [bias[i] if role.get(i, 4) in (3, 4) and i in full else None for i in range(b.n)]
    sols, res, pp = prof_batch(b, Bs, F, R)
    assert sorted(sols) == sorted(i for i in full if role.get(i, 4) in (2, 4))
    pp = [x.copy() for x in pp]
    with pytest.raises(pa.PhxError) as e:  # reprofile() keeps refusing a solve with required ORFs
        ann.reprofile()
    assert e.value.code == E_STATE and "required" in str(e.value)
    # mode 0: profile()'s records
    assert part(pp, full[0])[:2] == part(b.run_profile, full[0])[:2]
    # second reduction: a contig of mode 0, 1 or 3 has what reprofile() gives once every required list is emptied
    curate(ann, Bs, F, None)
    want = ann.reprofile()
    for i in range(b.n):
        if not R[i]:
            assert part(pp, i)[:2] == part(want, i)[:2], (i, role.get(i))
            assert not pp[3][pp[1][i]:pp[1][i + 1]].any()
    assert any(part(want, i) != part(b.run_profile, i) for i in (full[1], full[3]))  # (the refused / biased contigs differ from the run)
    # first reduction: no contig pinned — reprofile()'s three arrays byte for byte, lost all 0
    got = ann.pinprofile()
    assert [x.tobytes() for x in got[:3]] == [x.tobytes() for x in want] and got[3].shape == (len(want[2]), 3) and not got[3].any()
    assert ann.pinprofile_stats() == dict(contigs=0, rounds=0, lost_slots=0)
    # ... and the pinned solve once more gives the same bytes
    curate(ann, Bs, F, R)
    assert [part(ann.pinprofile(), i) for i in range(b.n)] == [part(pp, i) for i in range(b.n)]


# ---- 5. the wide classes ----
@pytest.mark.parametrize("case", range(4))
def test_a_mask_a_pin_and_a_penalty_in_the_wide_classes(pa, case):
    seqs = wide_cases(pa)[case][0]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    want = (4, 8, 8, 17)[case]  # 320, 576 twice and 1152 bits under MgPinProf
    c = next(i for i in range(len(seqs)) if st0[i] == 0 and int(ann.globals(i).n_limbs) == want)
    mst, moffs, mrec = ann.margins()
    assert mst[c] == 0
    run_profile = tuple(np.copy(x) for x in ann.profile())
    ref = CuRef(ann, c)
    rec = mrec[moffs[c]:moffs[c + 1]]
    pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0]
    long_one = int(pool[np.argmax(ref.orfs["length"][pool])])  # the widest ORF weights sit in the long ORF's group
    cg = ref.called(genes0[offs0[c]:offs0[c + 1]])
    other = int(pool[np.random.RandomState(3730 + case).randint(len(pool))])
    seen = 0
    for req in ([long_one], [other]):
        require, forbid, bias = [None] * len(seqs), [None] * len(seqs), [None] * len(seqs)
        require[c], forbid[c], bias[c] = req, [cg[len(cg) // 2]], {cg[0]: 4000}
        curate(ann, bias, forbid, require)
        pst, poffs, prec, lost = ann.pinprofile()
        seen += settled(check_prof(ann, ref, len(seqs[c]), forbid[c], require[c], bias[c], int(pst[c]), prec[poffs[c]:poffs[c + 1]], lost[poffs[c]:poffs[c + 1]]))
        for j in range(len(seqs)):  # neighbours keep the run's records
            if j != c:
                assert part((pst, poffs, prec, lost), j)[:2] == part(run_profile, j)[:2] and not lost[poffs[j]:poffs[j + 1]].any()
    ann.close()
    assert seen >= 1  # (a required ORF on a reachable cycle is checked as PHX_S_NEGCYCLE; one of the two at least settles)


# ---- 6. statuses ----
def test_no_path_and_negative_cycles_beside_clean_contigs(pa):
    from phanotate_amd.fasta import read_fasta

    seqs = [seq for name, seq in read_fasta(os.path.join(ROOT, "tests", "golden", "constrain_cycle.fasta"))]
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops  # no path: what lies behind the first stops is out of the source's reach
    clean = [pa.synth_contig(61, 9000), pa.synth_contig(62, 7000)]
    seqs = seqs + [clean[0], unreachable, clean[1]]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    assert st0.tolist() == [0, 0, 0, 1, 0]
    with pytest.raises(pa.PhxError) as e:  # before any re-annotation of the run, and before any kernel
        ann.pinprofile()
    assert e.value.code == E_STATE
    refs = {i: CuRef(ann, i) for i in range(5)}
    cyc = {i: [k for k, e in enumerate(refs[i].orf_edge) if e is not None and refs[i].on_cycle({e})] for i in (0, 1)}
    quiet = [k for k, e in enumerate(refs[3].orf_edge) if e is None or not refs[3].on_cycle({e})]
    mst, moffs, mrec = ann.margins()
    free = {2: [k for k, e in enumerate(refs[2].orf_edge) if e is not None][:2]}
    pool = np.flatnonzero((mrec[moffs[4]:moffs[5]]["called"] == 0) & (mrec[moffs[4]:moffs[5]]["through"] == 1))
    free[4] = [int(pool[len(pool) // 3]), int(pool[2 * len(pool) // 3])]  # two uncalled ORFs some path runs through
    require = [[cyc[0][0]], [cyc[1][-1]], free[2], quiet[:1], free[4]]
    st = ann.constrain(None, require)[0]
    assert st.tolist() == [S_NEGCYCLE, S_NEGCYCLE, 0, S_NOPATH, 0]
    out = pst, poffs, prec, lost = ann.pinprofile()
    assert pst.tolist() == st.tolist()
    V = [int(ann.globals(i).n_node) for i in range(5)]
    assert np.diff(poffs).tolist() == [0, 0, V[2] - 1, V[3] - 1, V[4] - 1] and V[3] > 2  # PHX_S_NEGCYCLE: no records
    sol = check_prof(ann, refs[3], len(seqs[3]), None, require[3], None, int(pst[3]), prec[poffs[3]:poffs[4]], lost[poffs[3]:poffs[4]])
    assert sol["D"] is None  # PHX_S_NOPATH: every value +inf, lost 0, lo / hi filled
    for k, i in enumerate((2, 4)):  # the neighbours are unaffected: the yardstick's values, and the bytes of a lone upload
        assert settled(check_prof(ann, refs[i], len(seqs[i]), None, require[i], None, int(pst[i]), prec[poffs[i]:poffs[i + 1]], lost[poffs[i]:poffs[i + 1]]))
        lone = pa.Annotator()
        run_batch(lone, [clean[k]])
        lone.constrain(None, [require[i]])
        assert part(lone.pinprofile(), 0) == part(out, i)
        lone.close()
    ann.close()


# ---- 7. isolation, the cache, the counters, invalidation ----
def test_pinprofile_disturbs_nothing_is_cached_and_invalidated(pa):
    seqs, nxt = fuzz(31, 12), fuzz(32, 6)
    a, o = pa.Annotator(), pa.Annotator()
    b = Batch(a, seqs)
    run_batch(o, seqs)
    forbid, require, bias = sets_of(b, 3740)
    pinned = [i for i in b.idx if require[i]]
    assert len(pinned) >= 5

    def others(ann):
        return [bytes_of(f()) for f in (ann.profile, ann.margins, ann.pinmargins, ann.pindrops)]

    # a: everything else first, then pinprofile(); o: pinprofile() first
    curate(a, bias, forbid, require)
    assert a.pinprofile_ms() == dict(tables=0.0, records=0.0, download=0.0) and a.pinprofile_stats() == dict(contigs=0, rounds=0, lost_slots=0)
    before = others(a)
    p1 = bytes_of(a.pinprofile())
    ms, stats = a.pinprofile_ms(), a.pinprofile_stats()
    st = a.pinprofile()[0]
    covered = [i for i in pinned if st[i] in (0, S_NOPATH)]
    print("pinprofile: %s ms, %s" % (ms, stats))
    assert ms["tables"] > 0 and stats["contigs"] == len(covered) >= 4
    assert stats["rounds"] > 3 * stats["contigs"] and stats["lost_slots"] > 0  # three rounds per contig and a level round somewhere
    assert others(a) == before  # the same bytes after it
    assert bytes_of(a.pinprofile()) == p1 and a.pinprofile_ms() == ms and a.pinprofile_stats() == stats  # the cached records: nothing was computed again
    curate(o, bias, forbid, require)
    assert bytes_of(o.pinprofile()) == p1 and others(o) == before  # ... whichever runs first
    curate(a, bias, forbid, require)  # the same re-annotation hits its cache and keeps the profile
    assert bytes_of(a.pinprofile()) == p1 and a.pinprofile_ms() == ms
    # reprofile() on a solve without pins: the same bytes before and after pinprofile(), and whichever runs first
    evidence(a, bias, forbid)
    evidence(o, bias, forbid)
    r1 = bytes_of(a.reprofile())
    g = o.pinprofile()
    assert bytes_of(g[:3]) == r1 and not g[3].any() and bytes_of(o.reprofile()) == r1
    assert bytes_of(a.pinprofile()[:3]) == r1 and bytes_of(a.reprofile()) == r1
    o.close()
    # a different solve invalidates it
    a.constrain(forbid, require)
    p2 = bytes_of(a.pinprofile())
    assert p2 != p1
    curate(a, bias, forbid, require)
    assert bytes_of(a.pinprofile()) == p1
    # ... and so does the next batch
    a.upload(nxt)
    with pytest.raises(pa.PhxError) as e:
        a.pinprofile()
    assert e.value.code == E_STATE
    a.run()
    with pytest.raises(pa.PhxError) as e:
        a.pinprofile()
    assert e.value.code == E_STATE
    a.curate(None, None, None)
    got = a.pinprofile()
    assert bytes_of(got[:3]) == bytes_of(a.profile()) and not got[3].any()
    a.close()


# ---- 8. through the solver ----
def test_refusing_every_gene_over_a_slot_costs_at_least_its_gap_pair(small):
    """With every ORF whose gene edge covers slot x refused on top of the re-annotation, the best path crosses x by a connector (the batch
    has no tRNA edges).  Where the slot's gap is (0, g), the new (unmet, D) minus the re-annotation's own is >= (0, g): D in integer units,
    compared through the rounding that made g, which is monotone.
    The points are drawn among the slots with gap = (0, g), g finite, that no required ORF covers (a refused ORF cannot be required).  A
    walk may cross a slot more than once, so equality is no law (§36)."""
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 3750)
    st, offs, genes, delta, unmet = [x.copy() for x in curate(ann, bias, forbid, require)]
    ok = [i for i in b.idx if require[i] and st[i] == 0][:8]  # 3 rounds: up to 24 points
    assert len(ok) >= 6
    D1 = {i: ann.reannotated_path(i)[1] for i in ok}
    pst, poffs, prec, lost = ann.pinprofile()
    rng = np.random.RandomState(3751)
    pool = {}
    for i in ok:
        ref = b.refs[i]
        V = ref.V
        rec, lo = prec[poffs[i]:poffs[i + 1]], lost[poffs[i]:poffs[i + 1]]
        under_pin = np.zeros(V - 1, bool)
        for k in require[i]:
            if ref.orf_edge[k] is not None:
                under_pin[ref.orf_edge[k][0] + 1:ref.orf_edge[k][1] + 1] = True
        pool[i] = (np.flatnonzero((lo[:, 2] == 0) & np.isfinite(rec["gap"]) & ~under_pin), np.copy(rec["gap"]))
        assert len(pool[i][0]) > 0, i
    points = equal = nopath = more_unmet = 0
    for r in range(3):
        slot = {i: int(pool[i][0][rng.randint(len(pool[i][0]))]) for i in ok}
        fb = []
        for i in range(b.n):
            if i not in slot:
                fb.append(forbid[i])
                continue
            V = b.refs[i].V
            over = [k for k, e in enumerate(b.refs[i].orf_edge) if e is not None and rank(e[0], V) + 1 <= slot[i] <= rank(e[1], V)]
            assert not set(over) & set(require[i])
            fb.append(sorted(set(forbid[i] or []) | set(over)))
        st2, offs2, genes2, delta2, unmet2 = curate(ann, bias, fb, require)
        for i, x in slot.items():
            g = float(pool[i][1][x])
            points += 1
            assert st2[i] in (0, S_NOPATH), (i, x, st2[i])  # (removing edges makes no cycle negative)
            if st2[i] == S_NOPATH:
                nopath += 1
                continue
            D2 = ann.reannotated_path(i)[1]
            got = (int(unmet2[i]) - int(unmet[i]), mu_of(D2 - D1[i]))  # (rounding is monotone: D2 - D1 >= s gives float(D2 - D1) / 1000 >= g)
            assert g >= 0.0 and got >= (0, g), (i, x, got, g)
            more_unmet += got[0] > 0
            equal += got == (0, g)
    print("through the solver: %d points, %d equalities, %d give up a pin, %d without a path" % (points, equal, more_unmet, nopath))
    assert 18 <= points <= 24 and points - nopath >= points // 2
