"""Pinned margins on the device (phx_pinmargins_flat, Annotator.pinmargins / pindist) against python integers.  The yardstick
is CuRef's weights (tests/test_curate_gpu.py) — the device's own tapped edges without the refused ORF edges, W + B on the biased ones and
- M on the required ones — through test_evidence_gpu.settle for d_s' and py_dt_in_R (tests/test_remargins_gpu.py) for d_t'.  Expected per
ORF: Delta'' = d_s'(u) + W' + d_t'(v) - D' = lost * M + s with |s| < M / 2, margin = float(s) / 1000.0.  Records are compared field by
field, `lost` entry by entry, pindist() node for node in both directions."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_constrain_gpu import bytes_of, fuzz, run_batch, wide_cases
from test_curate_gpu import Batch, CuRef, DeviceGraph, NoGraph, curate, keyed, sets_of
from test_evidence_gpu import settle
from test_remargins_gpu import check_called, py_dt_in_R, rec_bytes

import curate_draws as cd

pytestmark = pytest.mark.gpu

E_STATE, S_NEGCYCLE, S_NOPATH = -13, -9, 1


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


@pytest.fixture(scope="module")
def small(pa):
    """curate_draws.mix_seqs, run once: one contig of 179 nodes (one chunk of the reverse pass), the others 272-1004 nodes (several chunks,
    overlap edges re-opening an earlier chunk).  The tests leave the batch resident."""
    ann = pa.Annotator()
    b = Batch(ann, cd.mix_seqs(pa))
    V = sorted(int(ann.globals(i).n_node) for i in b.idx)
    print("nodes per contig:", V)
    assert len(b.idx) >= 8 and V[0] <= 256 and V[-1] > 768
    yield b
    ann.close()


# ---- the yardstick ----
def split(x, M):
    """(S, count) of a distance x = S - count * M with |S| < M / 2."""
    c = (-x + M // 2) // M
    return x + c * M, c


def pin_ref(ref, forbid, require, bias):
    """dict(cycle) or dict(cycle=False, D=None) or the definition's vectors and per-ORF (lost, s) (None: no path through the ORF)."""
    gone = {ref.orf_edge[k] for k in forbid or ()} - {None}
    pinned = {ref.orf_edge[k] for k in require or ()} - {None} - gone
    add = {}
    for k, B in (bias or {}).items():
        if ref.orf_edge[k] is not None:
            add[ref.orf_edge[k]] = add.get(ref.orf_edge[k], 0) + B
    M = 1 << ((sum(abs(w) for _, _, w in ref.edges) + sum(abs(B) for B in add.values())).bit_length() + 2)
    edges = [(u, v, w + add.get((u, v), 0) - (M if (u, v) in pinned else 0)) for u, v, w in ref.edges if (u, v) not in gone]
    V = ref.V
    dist, par = settle(V, edges, V - 2)
    if dist is None:
        return dict(cycle=True)
    if dist[V - 1] is None:
        return dict(cycle=False, D=None)
    dt = py_dt_in_R(V, edges, dist)
    assert dt[V - 2] == dist[V - 1]
    wmap = {(u, v): w for u, v, w in edges}
    D = dist[V - 1]
    per = []
    for k, e in enumerate(ref.orf_edge):
        if e is None or e not in wmap or dist[e[0]] is None or dt[e[1]] is None:
            per.append(None)
            continue
        x = dist[e[0]] + wmap[e] + dt[e[1]] - D
        assert x >= 0, (ref.i, k, x)
        s, c = split(x, M)
        per.append((-c, s))
    S, count = split(D, M)
    return dict(cycle=False, D=D, S=S, count=count, M=M, per=per,
                ds=[None if x is None else split(x, M) for x in dist], dt=[None if x is None else split(x, M) for x in dt])


def check_pin(ann, ref, forbid, require, bias, st, rec, lost, genes, nodes=True):
    """One pinned contig's records, `lost` and distances against the yardstick; returns the yardstick's dict."""
    i = ref.i
    what = (i, list(forbid or ()), list(require or ()), bias)
    sol = pin_ref(ref, forbid, require, bias)
    if sol["cycle"]:
        assert st == S_NEGCYCLE and len(rec) == 0 and len(lost) == 0, (what, st)
        return sol
    orfs = ref.orfs
    assert len(rec) == len(orfs) == len(lost), what
    if sol["D"] is None:
        assert st == S_NOPATH and not rec["through"].any() and (rec["margin"] == np.inf).all() and not rec["called"].any() and not lost.any(), (what, st)
        return sol
    assert st == 0, (what, st)
    if nodes:
        assert ann.pindist(i) == sol["ds"], what
        assert ann.pindist(i, to_target=True) == sol["dt"], what
    for k, (o, r) in enumerate(zip(orfs, rec)):
        fwd = o["frame"] > 0
        assert (int(r["left"]), int(r["right"])) == ((int(o["start"]), int(o["stop"]) + 2) if fwd else (int(o["stop"]), int(o["start"]) + 2))
        assert int(r["frame"]) == int(o["frame"]) and int(r["strand"]) == (1 if fwd else -1) and float(r["score"]) == float(o["weight"])
        p = sol["per"][k]
        if p is None:
            assert r["through"] == 0 and r["margin"] == np.inf and lost[k] == 0, (what, k)
            continue
        assert r["through"] == 1 and int(lost[k]) == p[0] and float(r["margin"]) == float(p[1]) / 1000.0, (what, k, p, int(lost[k]), float(r["margin"]))
        assert (p[0], p[1]) >= (0, 0)
    check_called(ann, i, rec, genes)
    on = rec["called"] == 1
    assert (rec["margin"][on] == 0.0).all() and (rec["through"][on] == 1).all() and not lost[on].any(), what
    return sol


def pin_batch(b, bias, forbid, require, nodes=True, solve_all=False):
    """curate(), pinmargins(), every contig with a required ORF against the yardstick: {contig: the yardstick's dict}, the two results."""
    ann = b.ann
    res = curate(ann, bias, forbid, require, solve_all)
    st, offs, genes, delta, unmet = res
    pm = mst, moffs, mrec, lost = ann.pinmargins()
    out = {}
    for i in b.idx:
        if not (require and require[i]):
            continue
        out[i] = check_pin(ann, b.refs[i], forbid and forbid[i], require[i], bias and bias[i], int(mst[i]), mrec[moffs[i]:moffs[i + 1]], lost[moffs[i]:moffs[i + 1]],
                           genes[offs[i]:offs[i + 1]], nodes)
        assert int(mst[i]) == int(st[i]), i
        if not out[i]["cycle"] and out[i]["D"] is not None:
            assert int(unmet[i]) == len(require[i]) - out[i]["count"]
    return out, res, pm


# ---- 1. the seeded mixes ----
@pytest.mark.parametrize("rnd", range(cd.ROUNDS))
def test_the_seeded_mixes_against_the_yardstick(small, rnd):
    """Every draw of the round is checked; tests/test_pinmargins_host.py counts 45 of 45 that settle, so each round brings at least 8."""
    b = small
    graphs = [DeviceGraph(b.refs[i], b.called[i]) if i in b.refs else NoGraph() for i in range(b.n)]
    row = cd.mixes(graphs)[rnd]
    forbid, require, bias = [None] * b.n, [None] * b.n, [None] * b.n
    for i, d in enumerate(row):
        if d is not None:
            by = b.refs[i].by_ends
            forbid[i], require[i], bias[i] = [by[k] for k in d["forbid"]], [by[k] for k in d["require"]], {by[k]: B for k, B in d["bias"].items()}
    sols, res, pm = pin_batch(b, bias, forbid, require)
    ok = [s for s in sols.values() if not s["cycle"] and s["D"] is not None]
    gave_up = sum(p is not None and p[0] > 0 for s in ok for p in s["per"])
    cheaper = sum(p is not None and p[0] > 0 and p[1] < 0 for s in ok for p in s["per"])
    print("round %d: %d draws, %d settle with a path; %d records give up a pin, %d of them with a negative margin" % (rnd, len(sols), len(ok), gave_up, cheaper))
    assert len(sols) == sum(d is not None for d in row) and len(ok) >= 8 and gave_up > 0 and cheaper > 0


# ---- 2. constrain() alone, curate(), and a batch of every mode; the reductions ----
def test_constrain_alone_and_curate_each_against_the_yardstick(small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 2410)
    assert sum(r is not None for r in require) >= 6
    res = ann.constrain(forbid, require)  # mode 2
    mst, moffs, mrec, lost = ann.pinmargins()
    seen = 0
    for i in b.idx:
        if require[i]:
            sol = check_pin(ann, b.refs[i], forbid[i], require[i], None, int(mst[i]), mrec[moffs[i]:moffs[i + 1]], lost[moffs[i]:moffs[i + 1]], res[2][res[1][i]:res[1][i + 1]])
            seen += not sol["cycle"] and sol["D"] is not None
        else:  # the run's result stands: margins()' records, lost 0
            assert rec_bytes((mst, moffs, mrec), i) == rec_bytes((b.mst, b.moffs, b.mrec), i) and not lost[moffs[i]:moffs[i + 1]].any()
    assert seen >= 5
    sols, _, _ = pin_batch(b, bias, forbid, require)  # mode 4
    assert sum(not s["cycle"] and s["D"] is not None for s in sols.values()) >= 5


def test_a_batch_of_every_mode_and_both_reductions(pa, small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 2411)
    full = [i for i in b.idx if require[i]]
    assert len(full) >= 6
    role = {full[0]: 0, full[1]: 1, full[2]: 2, full[3]: 3}  # the run's result, refused only, required only, biased only; the others all three
    F = [forbid[i] if role.get(i, 4) in (1, 4) and i in full else None for i in range(b.n)]
    R = [require[i] if role.get(i, 4) in (2, 4) and i in full else None for i in range(b.n)]
    Bs = [bias[i] if role.get(i, 4) in (3, 4) and i in full else None for i in range(b.n)]
    sols, res, pm = pin_batch(b, Bs, F, R)
    assert sorted(sols) == sorted(i for i in full if role.get(i, 4) in (2, 4))
    mst, moffs, mrec, lost = [x.copy() for x in pm]
    # second reduction: a contig of mode 0, 1 or 3 has what remargins() gives once every required list is emptied
    curate(ann, Bs, F, None)
    want = ann.remargins()
    rd = ann.redist(full[1]), ann.redist(full[1], to_target=True)
    for i in range(b.n):
        if not R[i]:
            assert rec_bytes((mst, moffs, mrec), i) == rec_bytes(want, i), (i, role.get(i))
            assert not lost[moffs[i]:moffs[i + 1]].any()
    assert any(rec_bytes(want, i) != rec_bytes((b.mst, b.moffs, b.mrec), i) for i in (full[1], full[3]))  # (the refused / biased contigs differ from the run)
    # first reduction: no contig pinned — remargins()' three arrays byte for byte, lost all 0
    got = ann.pinmargins()
    assert rec_bytes(got[:3]) == rec_bytes(want) and len(got[3]) == len(want[2]) and not got[3].any()
    # ... and after a solve that pinned a contig remargins() and redist() keep refusing
    curate(ann, Bs, F, R)
    for call in (ann.remargins, lambda: ann.redist(full[1])):
        with pytest.raises(pa.PhxError) as e:
            call()
        assert e.value.code == E_STATE and "required" in str(e.value)
    assert (ann.pindist(full[1]), ann.pindist(full[1], to_target=True)) == rd  # a refused-only contig beside pinned ones: redist()'s plain integers
    assert ann.pindist(full[0]) == ann.dist(full[0]) and ann.pindist(full[0], to_target=True) == ann.dist_to_target(full[0])
    assert [rec_bytes(ann.pinmargins()[:3], i) for i in range(b.n)] == [rec_bytes((mst, moffs, mrec), i) for i in range(b.n)]


# ---- 3. an unmet required ORF; two required starts of one stop group ----
def test_two_required_starts_of_one_stop_group_and_the_unmet_ones_record(small):
    b, ann = small, small.ann
    require, pairs = [None] * b.n, {}
    for i in b.idx:
        orfs = ann.orfs(i)
        grp = {}
        for k in b.reachable(i):
            grp.setdefault(int(orfs["group"][k]), []).append(int(k))
        same = [ks for ks in grp.values() if len(ks) >= 2]
        if same:
            pairs[i] = tuple(same[len(same) // 2][:2])
            require[i] = list(pairs[i])
    assert len(pairs) >= 6
    sols, res, pm = pin_batch(b, None, None, require)
    st, offs, genes, delta, unmet = res
    mst, moffs, mrec, lost = pm
    seen = 0
    for i, sol in sols.items():
        if sol["cycle"] or sol["D"] is None:
            continue
        called = b.refs[i].called(genes[offs[i]:offs[i + 1]])
        kept = [k for k in pairs[i] if k in called]
        assert unmet[i] == 1 and len(kept) == 1 and sol["count"] == 1  # a path takes one start per stop
        out = [k for k in pairs[i] if k not in called][0]
        r, lo = mrec[moffs[i] + out], int(lost[moffs[i] + out])
        # the unmet one: a path through it keeps as many pins as the best one (itself instead of its sibling) and cannot be cheaper
        assert r["through"] == 1 and r["called"] == 0 and lo == 0 and r["margin"] >= 0.0, (i, out, lo, float(r["margin"]))
        seen += 1
    assert seen >= 5


# ---- 4. pin one more, through the solver ----
def pin_one_more(b, seed, kind):
    """One ORF more per contig on top of sets_of(b, seed) — an uncalled one with lost = 0 (kind "lost0") or lost >= 1 ("lost1") —, all
    contigs in one call: (points, those the yardstick finds on a cycle)."""
    ann = b.ann
    forbid, require, bias = sets_of(b, seed)
    res = [x.copy() for x in curate(ann, bias, forbid, require)]
    st, offs, genes, delta, unmet = res
    mst, moffs, mrec, lost = [x.copy() for x in ann.pinmargins()]
    rng = np.random.RandomState(seed)
    more, pick, base = [r and list(r) for r in require], {}, {}
    for i in b.idx:
        if not require[i] or st[i] != 0:
            continue
        rec, lo = mrec[moffs[i]:moffs[i + 1]], lost[moffs[i]:moffs[i + 1]]
        free = (rec["through"] == 1) & (rec["called"] == 0)
        free[list(require[i]) + list(forbid[i] or [])] = False
        pool = np.nonzero(free & ((lo == 0) if kind == "lost0" else (lo >= 1)))[0]
        if len(pool) == 0:
            continue
        k = int(pool[rng.randint(len(pool))])
        # the yardstick's exact s behind the record (check_pin-style: the margin is its float)
        sol = pin_ref(b.refs[i], forbid[i], require[i], bias[i])
        assert float(rec["margin"][k]) == float(sol["per"][k][1]) / 1000.0 and int(lo[k]) == sol["per"][k][0]
        pick[i], base[i] = (k, int(lo[k]), sol["per"][k][1]), (sol["count"], sol["S"])
        more[i] = list(require[i]) + [k]
    assert len(pick) >= 4, (kind, len(pick))
    st2, offs2, genes2, delta2, unmet2 = curate(ann, bias, forbid, more)
    points = cycles = 0
    for i, (k, lo, s) in pick.items():
        points += 1
        if b.refs[i].solve(forbid[i] or (), more[i], bias[i])["cycle"]:  # the yardstick: k lies on a cycle the source reaches
            assert st2[i] == S_NEGCYCLE
            cycles += 1
            continue
        c0, S0 = base[i]
        want = min((-c0, S0), (-(c0 - lo + 1), S0 + s))
        assert st2[i] == 0
        S2 = ann.reannotated_path(i)[1]
        c2 = len(more[i]) - int(unmet2[i])
        assert (-c2, S2) == want, (kind, i, k, lo, s, (c2, S2), want)
        assert float(delta2[i]) == float(want[1] - b.D[i]) / 1000.0
        called = b.refs[i].called(genes2[offs2[i]:offs2[i + 1]])
        if lo == 0:  # an uncalled ORF that gives up no pin gets called, unmet does not grow, the sum grows by exactly s
            assert k in called and int(unmet2[i]) == int(unmet[i]) and S2 == S0 + s, (i, k)
        else:
            assert (k in called) == (want != (-c0, S0)), (i, k)
    return points, cycles


def test_pin_one_more_through_the_solver(small):
    """The theorem of §24 through constrain() / curate() themselves.  tests/test_pinmargins_host.py saw 7 of 218 such points on a cycle."""
    total = {"lost0": [0, 0], "lost1": [0, 0]}
    for n, kind in enumerate(["lost0"] * 7 + ["lost1"] * 4):
        points, cycles = pin_one_more(small, 2420 + n, kind)
        total[kind][0] += points
        total[kind][1] += cycles
    print("pin one more: (points, on a cycle) %s" % total)
    points, cycles = (total["lost0"][k] + total["lost1"][k] for k in (0, 1))
    assert total["lost0"][0] >= 40 and total["lost1"][0] >= 20
    assert cycles * 10 <= points, total


# ---- 5. the wide classes ----
@pytest.mark.parametrize("case", range(4))
def test_the_wide_classes(pa, case):
    seqs = wide_cases(pa)[case][0]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    want = (4, 8, 8, 17)[case]  # 320, 576 twice and 1152 bits under MgPin
    c = next(i for i in range(len(seqs)) if st0[i] == 0 and int(ann.globals(i).n_limbs) == want)
    mst, moffs, mrec = ann.margins()
    assert mst[c] == 0
    ref = CuRef(ann, c)
    rec = mrec[moffs[c]:moffs[c + 1]]
    pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0]
    long_one = int(pool[np.argmax(ref.orfs["length"][pool])])  # the widest ORF weights sit in the long ORF's group
    rng = np.random.RandomState(2430 + case)
    other = int(pool[rng.randint(len(pool))])
    cg = ref.called(genes0[offs0[c]:offs0[c + 1]])
    seen = 0
    for req, bias in (([long_one], {other: -2500, cg[0]: 4000}), ([other], None)):
        require, bb = [None] * len(seqs), [None] * len(seqs)
        require[c], bb[c] = req, bias
        st, offs, genes, delta, unmet = curate(ann, bb, None, require)
        pst, poffs, prec, lost = ann.pinmargins()
        sol = check_pin(ann, ref, None, req, bias, int(pst[c]), prec[poffs[c]:poffs[c + 1]], lost[poffs[c]:poffs[c + 1]], genes[offs[c]:offs[c + 1]])
        seen += not sol["cycle"] and sol["D"] is not None
        assert len(ann.pindist(c)) == ref.V
        for j in range(len(seqs)):  # neighbours keep the run's records
            if j != c:
                assert rec_bytes((pst, poffs, prec), j) == rec_bytes((mst, moffs, mrec), j) and not lost[poffs[j]:poffs[j + 1]].any()
    ann.close()
    assert seen >= 1


# ---- 6. statuses ----
def test_a_negative_cycle_has_no_records_and_no_path_has_records_without_a_path(pa):
    from phanotate_amd.fasta import read_fasta

    seqs = [seq for name, seq in read_fasta(os.path.join(ROOT, "tests", "golden", "constrain_cycle.fasta"))]
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops  # no path: what lies behind the first stops is out of the source's reach
    seqs = seqs + [pa.synth_contig(61, 9000), unreachable]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    assert st0.tolist() == [0, 0, 0, 1]
    m0 = ann.margins()
    refs = {i: CuRef(ann, i) for i in range(4)}
    cyc = {i: [k for k, e in enumerate(refs[i].orf_edge) if e is not None and refs[i].on_cycle({e})] for i in (0, 1)}
    free = [k for k, e in enumerate(refs[2].orf_edge) if e is not None][:2]
    quiet = [k for k, e in enumerate(refs[3].orf_edge) if e is None or not refs[3].on_cycle({e})]
    require = [[cyc[0][0]], [cyc[1][-1]], free, quiet[:1]]
    st, offs, genes, delta, unmet = ann.constrain(None, require)
    assert st.tolist()[:2] == [S_NEGCYCLE, S_NEGCYCLE] and st[3] == S_NOPATH
    pst, poffs, prec, lost = ann.pinmargins()
    assert pst.tolist() == st.tolist()
    assert poffs[1] == poffs[0] and poffs[2] == poffs[1]  # PHX_S_NEGCYCLE: no records
    for i in (0, 1):
        assert ann.pindist(i) == [None] * refs[i].V and ann.pindist(i, to_target=True) == [None] * refs[i].V
    check_pin(ann, refs[2], None, require[2], None, int(pst[2]), prec[poffs[2]:poffs[3]], lost[poffs[2]:poffs[3]], genes[offs[2]:offs[3]])
    sol = check_pin(ann, refs[3], None, require[3], None, int(pst[3]), prec[poffs[3]:poffs[4]], lost[poffs[3]:poffs[4]], genes[offs[3]:offs[4]])
    assert sol["D"] is None and poffs[4] - poffs[3] == len(refs[3].orfs) > 0  # PHX_S_NOPATH: every record through = 0
    assert ann.pindist(3, to_target=True) == [None] * refs[3].V
    ann.close()


# ---- 7. side effects, the cache, a lone contig ----
def test_pinmargins_disturb_nothing_are_cached_and_invalidated(pa):
    a, nxt = fuzz(31, 12), fuzz(32, 12)
    ann = pa.Annotator()
    b = Batch(ann, a)

    def everything():
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()], [ann.path(i)[0].tobytes() for i in range(ann.n)])

    forbid, require, bias = sets_of(b, 2440)
    assert sum(r is not None for r in require) >= 5
    before = everything()
    with pytest.raises(pa.PhxError) as e:  # no re-annotation of this run yet
        ann.pinmargins()
    assert e.value.code == E_STATE
    r0 = bytes_of(curate(ann, bias, forbid, require))
    assert ann.pinmargins_ms() == dict(apply=0.0, reverse=0.0, margins=0.0, download=0.0)
    p1 = bytes_of(ann.pinmargins())
    ms = ann.pinmargins_ms()
    assert ms["reverse"] > 0 and ms["margins"] > 0
    assert bytes_of(ann.pinmargins()) == p1 and ann.pinmargins_ms() == ms  # the second call launches nothing
    assert everything() == before
    assert bytes_of(curate(ann, bias, forbid, require)) == r0  # (the same re-annotation hits its cache ...)
    assert bytes_of(ann.pinmargins()) == p1 and ann.pinmargins_ms() == ms  # ... and keeps the margins
    with pytest.raises(pa.PhxError) as e:
        ann.remargins()
    assert e.value.code == E_STATE
    other = pa.Annotator()  # the pinned margins first, everything else behind them
    run_batch(other, a)
    curate(other, bias, forbid, require)
    assert bytes_of(other.pinmargins()) == p1 and [x.tobytes() for x in other.margins()] == before[1]
    other.close()
    # a different solve invalidates them
    c1 = bytes_of(ann.constrain(forbid, require))
    p2 = bytes_of(ann.pinmargins())
    assert p2 != p1
    curate(ann, bias, forbid, require)
    assert bytes_of(ann.pinmargins()) == p1
    # a lone contig against the same contig in the batch
    pm = ann.pinmargins()
    full = [i for i in b.idx if require[i]]
    for i in full[::3]:
        lone = pa.Annotator()
        run_batch(lone, [a[i]])
        where = {key: k for k, key in enumerate(keyed(lone, 0, range(len(lone.orfs(0)))))}
        at = lambda ks: [where[key] for key in keyed(ann, i, ks)]
        curate(lone, [dict(zip(at(list(bias[i])), bias[i].values()))], [at(forbid[i])], [at(require[i])])
        got = lone.pinmargins()
        assert rec_bytes(got[:3], 0) == rec_bytes(pm[:3], i) and got[3].tobytes() == pm[3][pm[1][i]:pm[1][i + 1]].tobytes(), i
        assert lone.pindist(0) == ann.pindist(i) and lone.pindist(0, to_target=True) == ann.pindist(i, to_target=True)
        lone.close()
    # ... and so does the next batch
    ann.upload(nxt)
    with pytest.raises(pa.PhxError) as e:
        ann.pinmargins()
    assert e.value.code == E_STATE
    ann.run()
    for call in (ann.pinmargins, lambda: ann.pindist(0)):
        with pytest.raises(pa.PhxError) as e:
            call()
        assert e.value.code == E_STATE
    ann.curate(None, None, None)
    got = ann.pinmargins()
    assert rec_bytes(got[:3]) == rec_bytes(ann.margins()) and not got[3].any()
    ann.close()


# ---- 8. the CLI ----
def test_cli_pin_margins(pa, tmp_path):
    from phanotate_amd.cli import format_pin_margins

    g, name, phix = load_golden("phiX174")
    seqs = {name: phix, "c2": pa.synth_contig(72, 9000).decode()}
    fasta = tmp_path / "two.fasta"
    fasta.write_text("".join(">%s\n%s\n" % kv for kv in seqs.items()))
    ann = pa.Annotator()
    b = Batch(ann, list(seqs.values()))
    rq_lines, fb_lines, require, forbid = [], [], [None, None], [None, None]
    for i, nm in enumerate(seqs):
        orfs = ann.orfs(i)
        line = lambda k: "%d\t%d\t%s\t%s" % ((int(orfs[k]["start"]), int(orfs[k]["stop"]) + 2, "+", nm) if orfs[k]["frame"] > 0 else (int(orfs[k]["start"]) + 2, int(orfs[k]["stop"]), "-", nm))
        pool = b.reachable(i)
        require[i] = [pool[len(pool) // 3], pool[2 * len(pool) // 3]]
        forbid[i] = [b.called[i][1]]
        rq_lines += [line(k) for k in require[i]]
        fb_lines += [line(k) for k in forbid[i]]
    rq, fb, out, pm = tmp_path / "rq.txt", tmp_path / "fb.txt", tmp_path / "out.txt", tmp_path / "pm.txt"
    rq.write_text("\n".join(rq_lines) + "\n")
    fb.write_text("\n".join(fb_lines) + "\n")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta), "--require", str(rq), "--forbid", str(fb), "--reannotation", str(out), "--pin-margins", str(pm)],
                         capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    ann.constrain(forbid, require)
    st, offs, rec, lost = ann.pinmargins()
    assert st.tolist() == [0, 0]
    text = open(pm, "rb").read()
    assert text == format_pin_margins(list(seqs), st, offs, rec, lost)
    rows = [ln.split("\t") for ln in text.decode().splitlines() if not ln.startswith("#")]
    assert len(rows) == int((rec["through"] == 1).sum()) and all(len(r) == 8 for r in rows)
    assert sum(int(r[6]) > 0 for r in rows) == int(((lost > 0) & (rec["through"] == 1)).sum()) > 0
    ann.close()
