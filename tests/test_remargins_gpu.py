"""Re-annotation margins on the device (phx_remargins_flat) against python integers.  The yardstick is EvRef.solve(forbid,
bias) of tests/test_evidence_gpu.py: its `dist` is d_s', and d_t' is a Bellman-Ford from the target over the policy's edges reversed, using
only edges whose source the forward solve reached, in py_dist_to_target's sweep order.  Records are compared field by field as check_full
of tests/test_margins_gpu.py does; redist() node for node in both directions.  Also the chain theorem through the solver itself, the
identities with margins(), statuses, isolation, the cache and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_cases, golden_params, golden_trnas, load_golden
from test_evidence_gpu import NEGCYCLE, EvRef, called_orfs, draw_orfs, evidence, solved_contigs
from test_margins_gpu import parse_margins_file, sweep_idx
from test_reannotate_gpu import fuzz, mask_rounds, run_batch, wide_cases
from test_scenarios_gpu import case1_seqs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def py_dt_in_R(V, edges, dist):
    """d_t' of every node: Bellman-Ford from the target over `edges` reversed, restricted to the edges whose source has a forward distance
    (a node outside R is never given a value), in py_dist_to_target's sweep order; None: no such path."""
    use = sorted((e for e in edges if dist[e[0]] is not None), key=lambda e: sweep_idx(e[0], V))
    d = [None] * V
    if dist[V - 1] is not None:
        d[V - 1] = 0
    for _ in range(V + 1):
        ch = False
        for u, v, w in use:
            dv = d[v]
            if dv is None:
                continue
            c = dv + w
            if d[u] is None or c < d[u]:
                d[u] = c
                ch = True
        if not ch:
            return d
    raise AssertionError("no fixed point: a cycle of negative length inside R")


def rec_bytes(out, i=None):
    st, offs, rec = out
    if i is None:
        return st.tobytes(), offs.tobytes(), rec.tobytes()
    return int(st[i]), rec[offs[i]:offs[i + 1]].tobytes()


def check_called(ann, i, rec, genes):
    """`called` marks exactly the CDS genes the re-annotation call returned for the contig."""
    got = sorted((int(r["left"]), int(r["right"]), int(r["strand"])) for r in rec[rec["called"] == 1])
    want = sorted((int(g["left"]), int(g["right"]), int(g["strand"])) for g in genes if abs(int(g["frame"])) <= 3)
    assert got == want, i


def check_contig(ann, ref, forbid, bias, st, rec, genes, nodes=True):
    """One contig's records against the yardstick; returns NEGCYCLE, None (no path) or D'."""
    i = ref.i
    sol = ref.solve(forbid or [], bias)
    if sol == NEGCYCLE:
        assert st == -9 and len(rec) == 0, (i, forbid, bias, st)
        return NEGCYCLE
    DB, path, want_genes, dist, edges = sol
    orfs = ref.orfs
    assert len(rec) == len(orfs), i
    if DB is None:
        assert st == 1 and not rec["through"].any() and (rec["margin"] == np.inf).all() and not rec["called"].any(), (i, forbid, bias, st)
        return None
    assert st == 0, (i, forbid, bias, st)
    V = ref.V
    dt = py_dt_in_R(V, edges, dist)
    assert dt[V - 2] == DB and dt[V - 1] == 0
    if nodes:
        assert ann.redist(i) == dist, i
        assert ann.redist(i, to_target=True) == dt, i
    wmap = {(u, v): w for u, v, w in edges}  # the policy's edges: refused ones are gone, biased ones weigh W + B
    assert len(wmap) == len(edges)
    refused = set(forbid or [])
    for k, (o, r) in enumerate(zip(orfs, rec)):
        fwd = o["frame"] > 0
        assert (int(r["left"]), int(r["right"])) == ((int(o["start"]), int(o["stop"]) + 2) if fwd else (int(o["stop"]), int(o["start"]) + 2))
        assert int(r["frame"]) == int(o["frame"]) and int(r["strand"]) == (1 if fwd else -1) and float(r["score"]) == float(o["weight"])
        e = ref.orf_edge[k]
        if k in refused or e is None or dist[e[0]] is None or dt[e[1]] is None:
            assert e is None or k not in refused or e not in wmap
            assert r["through"] == 0 and r["margin"] == np.inf, (i, k, e)
            continue
        delta = dist[e[0]] + wmap[e] + dt[e[1]] - DB
        assert delta >= 0, (i, k, delta)
        assert r["through"] == 1 and float(r["margin"]) == float(delta) / 1000.0, (i, k, delta, float(r["margin"]))
    check_called(ann, i, rec, genes)
    assert (rec["margin"][rec["called"] == 1] == 0.0).all() and (rec["through"][rec["called"] == 1] == 1).all(), i
    return DB


def check_batch(ann, refs, forbid, bias, nodes=True):
    """evidence(bias, forbid) — reannotate(forbid) where there is no bias —, remargins(), every contig of refs against the yardstick."""
    n = ann.n
    if bias is None:
        st, offs, genes, delta = ann.reannotate(forbid)
    else:
        st, offs, genes, delta = evidence(ann, bias, forbid)
    mst, moffs, mrec = ann.remargins()
    out = {}
    for i in refs:
        f = None if forbid is None else forbid[i]
        b = None if bias is None else bias[i]
        if f is None and b is None:
            continue
        out[i] = check_contig(ann, refs[i], f, b, int(mst[i]), mrec[moffs[i]:moffs[i + 1]], genes[offs[i]:offs[i + 1]], nodes)
        assert int(mst[i]) == int(st[i]), i
    return out


@pytest.fixture(scope="module")
def big(pa):
    """case1_seqs + fuzz(11, 6), run once: contigs below 256 nodes (one chunk of the reverse pass) and the three long ones (several chunks,
    overlap edges re-opening an earlier chunk).  (ann, the run's download, yardsticks, the run's D, the called ORFs.)  The tests leave the
    batch resident."""
    ann = pa.Annotator()
    dl = run_batch(ann, case1_seqs(pa) + fuzz(11, 6))
    idx = solved_contigs(ann, dl[0])
    V = {i: int(ann.globals(i).n_node) for i in idx}
    print("nodes per contig:", sorted(V.items()))
    assert any(v <= 256 for v in V.values()) and all(i in V and V[i] > 256 for i in range(3)), sorted(V.items())  # both kinds are present
    refs = {i: EvRef(ann, i) for i in idx}
    called = {i: called_orfs(ann, i, dl[2][dl[1][i]:dl[1][i + 1]]) for i in idx}
    yield ann, dl, refs, {i: ann.path(i)[1] for i in idx}, called
    ann.close()


def draw_penalties(ann, refs, called, rng):
    """Per contig 6 drawn ORFs and two called ones with B > 0, |B| from 10^1 to 10^6; and a mask of called genes without a bias."""
    n = ann.n
    bias = [{k: int(10 ** rng.uniform(1, 6)) for k in draw_orfs(refs[i], called[i], rng, 6)} if i in refs else None for i in range(n)]
    forbid = [sorted(set(called[i][1::4]) - set(bias[i])) or None if i in refs else None for i in range(n)]
    return bias, forbid


# ---- 1. masks ----
def test_masks_against_the_yardstick(big):
    ann, dl, refs, D, called = big
    n = ann.n
    rng = np.random.RandomState(2101)
    order = sorted(refs)
    plans = dict(zip(order, mask_rounds([refs[i] for i in order], [called[i] for i in order], rng)))
    have = [i for i in order if called[i]]
    assert len(have) >= len(order) - 1 and all(plans[i] for i in have)
    few = [sorted(rng.choice(called[i], min(len(called[i]), int(rng.randint(1, 4))), replace=False).tolist()) if i in have else None for i in range(n)]
    sets = [plans[i][-1] if i in have else None for i in range(n)]
    seen = 0
    for forbid, nodes in ((few, True), (sets, False)):  # 1-3 called genes; mask_rounds' draw: 1-5 % of the ORFs with a called gene among them
        got = check_batch(ann, refs, forbid, None, nodes)
        assert set(got) == set(have) and NEGCYCLE not in got.values()  # no point is left out
        seen += sum(g is not None for g in got.values())
        for i, g in got.items():
            assert g is None or g >= D[i]
    assert seen >= 2 * len(refs) - 2, seen


# ---- 2. penalties ----
def test_penalties_alone_and_with_a_mask(big):
    ann, dl, refs, D, called = big
    bias, forbid = draw_penalties(ann, refs, called, np.random.RandomState(2102))
    assert any(f for f in forbid)
    for fb, nodes in ((None, True), (forbid, False)):
        got = check_batch(ann, refs, fb, bias, nodes)
        assert set(got) == set(refs) and NEGCYCLE not in got.values()  # a penalty cannot make a cycle negative: no point is left out
        assert all(g is None or g >= D[i] for i, g in got.items())
        assert sum(g is not None for g in got.values()) >= len(refs) - 1


# ---- 3. bonuses: the draw of test_margin_titration at -Delta - 1 ----
def test_bonuses_of_the_titration_draw(big):
    ann, dl, refs, D, called = big
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
        got = check_batch(ann, refs, None, bias, nodes=r == 0)
        assert NEGCYCLE not in got.values() and None not in got.values(), (r, got)  # (none of the draw's points lies on a negative cycle)
        for i, DB in got.items():
            assert DB == D[i] - 1, (i, r)  # the bonus wins by one unit
        points += len(got)
    print("bonuses: %d points of the titration draw" % points)
    assert points == sum(len(p) for p in picks.values()) >= 60


# ---- 4. the chain theorem: on top of evidence B0 the smallest further bonus that gets an uncalled ORF called is its margin here ----
def test_chain_theorem_through_the_solver(big):
    ann, dl, refs, D, called = big
    n = ann.n
    idx = sorted(refs)
    B0, _ = draw_penalties(ann, refs, called, np.random.RandomState(2102))
    st, offs, genes, delta = evidence(ann, B0)
    assert all(st[i] == 0 for i in idx)
    D1 = {i: ann.reannotated_path(i)[1] for i in idx}
    mst, moffs, mrec = ann.remargins()
    rng = np.random.RandomState(2104)
    picks = {}
    for i in idx:
        rec = mrec[moffs[i]:moffs[i + 1]]
        ok = [k for k in range(len(rec)) if rec["through"][k] == 1 and rec["called"][k] == 0 and round(float(rec["margin"][k]) * 1000) < 1 << 50]
        picks[i] = [(k, int(round(float(rec["margin"][k]) * 1000))) for k in sorted(rng.choice(ok, min(len(ok), 3), replace=False).tolist())]
    points = left_out = clean = 0
    for r in range(3):
        ok_at = {i: 0 for i in idx if r < len(picks[i])}
        for step in (1, -1):
            bias = []
            for i in range(n):
                b = dict(B0[i]) if B0[i] is not None else None
                if i in ok_at:
                    k, Delta = picks[i][r]
                    b[k] = b.get(k, 0) - Delta + step
                bias.append(b)
            st, offs, genes, delta = evidence(ann, bias)
            for i in ok_at:
                k, Delta = picks[i][r]
                points += 1
                if st[i] == -9:
                    left_out += 1
                    continue
                assert st[i] == 0, (i, k, st[i])
                DB = ann.reannotated_path(i)[1]
                assert DB == (D1[i] if step > 0 else D1[i] - 1), (i, k, Delta, step, DB, D1[i])
                if step < 0:
                    assert k in called_orfs(ann, i, genes[offs[i]:offs[i + 1]]), (i, k, Delta)
                ok_at[i] += 1
        clean += sum(c == 2 for c in ok_at.values())
    print("chain: %d points, %d left out (negative cycle), %d ORFs clean at both" % (points, left_out, clean))
    assert 3 * left_out <= points and clean >= 15, (points, left_out, clean)


# ---- 5. identities ----
def check_equals_margins(ann, cert):
    """Nothing refused, no bias: solved again or not, the records are margins() byte for byte on the certified contigs."""
    n = ann.n
    want = ann.margins()
    seen = 0
    for solve_all in (True, False):
        ann.reannotate([None] * n, solve_all=solve_all)
        got = ann.remargins()
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
        for i in range(n):
            if cert[i] == 1 and want[0][i] >= 0:
                assert rec_bytes(got, i) == rec_bytes(want, i), (i, solve_all)
                seen += solve_all and want[1][i + 1] > want[1][i]
    return seen


def test_nothing_refused_no_bias_is_margins_byte_for_byte(pa, big):
    ann = big[0]
    n = check_equals_margins(ann, ann.certified())
    for case in golden_cases():
        g, name, seq = load_golden(case)
        if str(g["error"]):
            continue
        one = pa.Annotator(pa.make_params(**golden_params(g)))
        tr = golden_trnas(g)
        run_batch(one, [seq], None if tr is None else [tr])
        n += check_equals_margins(one, one.certified())
        one.close()
    assert n >= 15, n


def test_called_orfs_have_margin_zero_and_refused_ones_no_path(big):
    ann, dl, refs, D, called = big
    n = ann.n
    bias, forbid = draw_penalties(ann, refs, called, np.random.RandomState(2105))
    st, offs, genes, delta = evidence(ann, bias, forbid)
    mst, moffs, mrec = ann.remargins()
    seen = 0
    for i in refs:
        assert mst[i] == st[i] and st[i] in (0, 1), i
        rec = mrec[moffs[i]:moffs[i + 1]]
        if st[i] == 1:  # the mask leaves no path: nothing is called, nothing runs through any ORF
            assert not rec["through"].any() and not rec["called"].any() and offs[i + 1] == offs[i]
            continue
        for k in called_orfs(ann, i, genes[offs[i]:offs[i + 1]]):
            assert rec["margin"][k] == 0.0 and rec["through"][k] == 1 and rec["called"][k] == 1, (i, k)
            seen += 1
        for k in forbid[i] or []:
            assert rec["through"][k] == 0 and rec["margin"][k] == np.inf and rec["called"][k] == 0, (i, k)
    assert seen >= 30


# ---- 6. the wide classes ----
@pytest.mark.parametrize("case", range(4))
def test_a_mask_and_a_penalty_in_the_wide_classes(pa, case):
    seqs, nl = wide_cases(pa)[case]
    ann = pa.Annotator()
    dl = run_batch(ann, seqs)
    want = (4, 8, 8, 17)[case]  # 256, 512, 512 and 1088 bits
    i = next(i for i in range(len(seqs)) if dl[0][i] == 0 and int(ann.globals(i).n_limbs) == want)
    refs = {i: EvRef(ann, i)}
    cg = called_orfs(ann, i, dl[2][dl[1][i]:dl[1][i + 1]])
    rng = np.random.RandomState(2106 + case)
    forbid = [None] * len(seqs)
    forbid[i] = [cg[int(rng.randint(len(cg)))]]
    got = check_batch(ann, refs, forbid, None)
    assert got[i] is not NEGCYCLE
    bias = [None] * len(seqs)
    bias[i] = {k: int(10 ** rng.uniform(1, 6)) for k in draw_orfs(refs[i], cg, rng, 6)}
    got = check_batch(ann, refs, None, bias)
    assert got[i] not in (NEGCYCLE, None)
    ann.close()


# ---- 7. statuses ----
def cycle_orf(ref):
    """An ORF whose edge lies on a cycle the source reaches: a bonus far beyond every weight makes that cycle negative."""
    out = {}
    for u, v, w in ref.edges:
        out.setdefault(u, []).append(v)
    for k, e in enumerate(ref.orf_edge):
        if e is None:
            continue
        seen, todo = {e[1]}, [e[1]]
        while todo and e[0] not in seen:
            for x in out.get(todo.pop(), []):
                if x not in seen:
                    seen.add(x)
                    todo.append(x)
        if e[0] in seen and ref.solve([], {k: -10 ** 9}) == NEGCYCLE:
            return k
    return None


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
        ann.remargins()
    assert e.value.code == -13
    assert st0.tolist() == [-2, -3, 0, 0, 0, 0]
    forbid = [None, None, np.arange(len(ann.orfs(2))), None, None, None]
    bias = [None, None, None, {neg[1]: -10 ** 9}, None, None]
    for i in (4, 5):
        bias[i] = {called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])[0]: 4000, 3: -2500}
    st, offs, genes, delta = evidence(ann, bias, forbid)
    assert st.tolist() == [-2, -3, 1, -9, 0, 0]
    mst, moffs, mrec = ann.remargins()
    assert mst.tolist() == [-2, -3, 1, -9, 0, 0]
    assert np.diff(moffs).tolist() == [0, 0, len(ann.orfs(2)), 0, len(ann.orfs(4)), len(ann.orfs(5))]
    nopath = mrec[moffs[2]:moffs[3]]
    assert len(nopath) > 0 and not nopath["through"].any() and (nopath["margin"] == np.inf).all() and not nopath["called"].any()
    assert (nopath["left"] > 0).all() and [int(x) for x in nopath["frame"]] == [int(x) for x in ann.orfs(2)["frame"]]
    assert ann.redist(2, to_target=True) == [None] * int(ann.globals(2).n_node)  # no path: no d_t'
    assert ann.redist(3) == ann.redist(3, to_target=True) == [None] * int(ann.globals(3).n_node)  # the solve gave up: no vectors
    assert ann.redist(0) == ann.redist(1, to_target=True) == []
    for k, i in enumerate((4, 5)):  # the neighbours are unaffected
        check_contig(ann, EvRef(ann, i), None, bias[i], int(mst[i]), mrec[moffs[i]:moffs[i + 1]], genes[offs[i]:offs[i + 1]])
        lone = pa.Annotator()
        run_batch(lone, [good[k]])
        evidence(lone, [bias[i]])
        assert rec_bytes(lone.remargins(), 0) == rec_bytes((mst, moffs, mrec), i)
        lone.close()
    # not solved again: the run's records (the plain contigs, without solve_all)
    ann.reannotate([None] * 6)
    got, want, cert = ann.remargins(), ann.margins(), ann.certified()
    assert got[0].tolist() == want[0].tolist() == [-2, -3, 0, 0, 0, 0] and got[1].tolist() == want[1].tolist()
    assert [rec_bytes(got, i) == rec_bytes(want, i) for i in (2, 3, 4, 5) if cert[i] == 1].count(True) >= 2
    assert ann.redist(4) == ann.dist(4) and ann.redist(4, to_target=True) == ann.dist_to_target(4)
    # required ORFs on any contig: PHX_E_STATE, and the text says why
    req = [None] * 6
    req[5] = [called_orfs(ann, 5, genes0[offs0[5]:offs0[6]])[0]]
    ann.constrain(require=req)
    for call in (ann.remargins, lambda: ann.redist(4)):
        with pytest.raises(pa.PhxError) as e:
            call()
        assert e.value.code == -13 and "required" in str(e.value)
    ann.constrain(forbid=req)  # nothing required: phx_constrain_flat serves too
    assert ann.remargins()[0].tolist() == [-2, -3, 0, 0, 0, 0]
    ann.close()


# ---- 8. isolation and the cache ----
def some_evidence(ann, seed, only=None):
    """Per solved contig (of `only`) a refused called gene, a penalised called gene and three ORFs with a bonus."""
    rng = np.random.RandomState(seed)
    st0, offs0, genes0 = ann.download_flat(exact=False)
    bias, forbid = [], []
    for i in range(ann.n):
        cg = called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]]) if st0[i] == 0 and (only is None or i in only) else []
        if len(cg) < 2:
            bias.append(None)
            forbid.append(None)
            continue
        b = {int(k): -int(rng.randint(1, 3000)) for k in rng.choice(len(ann.orfs(i)), min(3, len(ann.orfs(i))), replace=False)}
        b[cg[len(cg) // 2]] = 5000
        bias.append(b)
        forbid.append([cg[0]])
    return bias, forbid


def test_remargins_disturb_nothing_are_cached_and_invalidated(pa):
    a, b = fuzz(31, 20), fuzz(32, 20)

    def everything(ann, bias, forbid):
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()],
                [x.tobytes() for x in evidence(ann, bias, forbid)], [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n)])

    ann = pa.Annotator()
    run_batch(ann, a)
    bias, forbid = some_evidence(ann, 2108)
    before = everything(ann, bias, forbid)
    assert ann.remargins_ms() == dict(apply=0.0, reverse=0.0, margins=0.0, download=0.0)
    r1 = rec_bytes(ann.remargins())
    ms = ann.remargins_ms()
    assert ms["reverse"] > 0 and ms["margins"] > 0
    assert rec_bytes(ann.remargins()) == r1 and ann.remargins_ms() == ms  # the second call launches nothing
    assert everything(ann, bias, forbid) == before  # (the same re-annotation hits its cache ...)
    assert rec_bytes(ann.remargins()) == r1 and ann.remargins_ms() == ms  # ... and keeps the margins
    other = pa.Annotator()  # the margins of the re-annotation first, everything else behind them
    run_batch(other, a)
    evidence(other, bias, forbid)
    assert rec_bytes(other.remargins()) == r1 and everything(other, bias, forbid) == before
    # a different re-annotation invalidates them
    bias2, forbid2 = some_evidence(ann, 2109)
    evidence(ann, bias2, forbid2)
    evidence(other, bias2, forbid2)
    r2 = rec_bytes(ann.remargins())
    assert r2 != r1 and r2 == rec_bytes(other.remargins())
    other.close()
    # ... and so does the next batch
    ann.upload(b)
    with pytest.raises(pa.PhxError) as e:
        ann.remargins()
    assert e.value.code == -13
    ann.run()
    with pytest.raises(pa.PhxError) as e:
        ann.remargins()
    assert e.value.code == -13
    fresh = pa.Annotator()
    run_batch(fresh, b)
    bias, forbid = some_evidence(fresh, 2110)
    evidence(ann, bias, forbid)
    evidence(fresh, bias, forbid)
    assert rec_bytes(ann.remargins()) == rec_bytes(fresh.remargins())
    for x in (ann, fresh):
        x.close()


def test_lone_contig_and_batch_of_300_give_the_same_bytes(pa):
    seqs = fuzz(23, 300)
    ann = pa.Annotator()
    run_batch(ann, seqs)
    only = set(range(2, 300, 37))
    bias, forbid = some_evidence(ann, 2111, only)
    evidence(ann, bias, forbid, solve_all=True)
    out = ann.remargins()
    got = {i: rec_bytes(out, i) for i in only if bias[i] is not None}
    assert len(got) >= 5
    for i, want in got.items():
        lone = pa.Annotator()
        run_batch(lone, [seqs[i]])
        evidence(lone, [bias[i]], [forbid[i]])
        assert rec_bytes(lone.remargins(), 0) == want, i
        lone.close()
    ann.close()


def test_create_flags_give_the_same_bytes(pa):
    batches = ([pa.synth_contig(61, 14000), pa.synth_contig(62, 9000)], fuzz(5, 20))

    def outs(flags):
        ann = pa.Annotator(flags=flags)
        res = []
        for seqs in batches:
            run_batch(ann, seqs)
            bias, forbid = some_evidence(ann, 2112)
            evidence(ann, bias, forbid)
            res.append(rec_bytes(ann.remargins()))
        ann.close()
        return res

    want = outs(())
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        assert outs((fl,)) == want, fl


# ---- 9. the CLI ----
def test_cli_remargins(pa, tmp_path):
    g, name, phix = load_golden("phiX174")
    fasta = tmp_path / "phix.fasta"
    fasta.write_text(">%s\n%s\n" % (name, phix))
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, [phix])
    orfs = ann.orfs(0)
    cds = [x for x in genes0 if abs(int(x["frame"])) <= 3]
    rows = []  # (ORF index, the line's first four columns)
    for k in [int(x) for x in np.random.RandomState(2113).choice(len(orfs), 4, replace=False)] + called_orfs(ann, 0, cds[:2]):
        o = orfs[k]
        a, z = (int(o["start"]), int(o["stop"]) + 2) if o["frame"] > 0 else (int(o["start"]) + 2, int(o["stop"]))
        rows.append((k, "%d\t%d\t%s\t%s" % (a, z, "+" if o["frame"] > 0 else "-", name)))
    vals = [-30.0, -2.5, 1.25, -8.0, 4.0]
    ev, fb, out, mg = tmp_path / "ev.txt", tmp_path / "fb.txt", tmp_path / "out.txt", tmp_path / "mg.txt"
    ev.write_text("".join("%s\t%r\n" % (ln, b) for (k, ln), b in zip(rows, vals)))
    fb.write_text(rows[5][1] + "\n")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta), "--evidence", str(ev), "--forbid", str(fb), "--reannotation", str(out), "--remargins", str(mg)],
                         capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    ann.evidence([[(k, b) for (k, ln), b in zip(rows, vals)]], [[rows[5][0]]])
    st, offs, rec = ann.remargins()
    assert st.tolist() == [0]
    r = rec[rec["through"] == 1]
    r = r[np.lexsort((r["strand"], r["right"], r["left"]))]
    want = [[str(x["right"] if x["strand"] < 0 else x["left"]), str(x["left"] if x["strand"] < 0 else x["right"]), "+" if x["strand"] > 0 else "-", name,
             "%E" % float(x["score"]), "%E" % float(x["margin"]), str(int(x["called"]))] for x in r]
    blocks = parse_margins_file(str(mg))  # (it parses as a --margins file)
    assert list(blocks) == [name] and blocks[name] == want
    assert rec["through"][rows[5][0]] == 0 and len(r) < len(rec)
    ann.close()
