"""Evidence-weighted re-annotation on the device (phx_evidence_flat) against python integers: the yardstick of
tests/test_reannotate_gpu.py — the device's own tapped edges, W = trunc(w * 1000), in Graph.iteredges order, under an in-place Bellman-Ford
with a strict '<' — with B added to the listed ORF edges.  Status, delta, the tapped path, D_B and the gene tuples must be the yardstick's;
where its Bellman-Ford does not settle the device must say PHX_S_NEGCYCLE, and nowhere else."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_cases, golden_params, golden_trnas, inorder_bellman_ford, load_golden
from test_reannotate_gpu import Ref, fuzz, gene_tuples, reann_bytes, run_batch, wide_cases

pytestmark = pytest.mark.gpu

NEGCYCLE = "negcycle"
B_MAX = 1 << 52


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def score(B):
    """A float b of SCORE units with math.trunc(b * 1000.0) == B, the conversion Annotator.evidence documents."""
    b = B / 1000.0
    for _ in range(4):
        got = math.trunc(b * 1000.0)
        if got == B:
            return b
        b = math.nextafter(b, math.inf if got < B else -math.inf)
    raise AssertionError(B)


def settle(V, edges, s):
    """conftest.inorder_bellman_ford — the same relaxations in the same order, hence the same distances and parents — that gives up as
    soon as the parent pointers close a circle: in an in-place Bellman-Ford that happens only on a cycle of negative length, on which
    it would not settle within V + 1 rounds either.  (None, None) then, as there."""
    dist, par = [None] * V, [-1] * V
    dist[s] = 0
    for _ in range(V + 1):
        ch = False
        for i, (u, v, w) in enumerate(edges):
            du = dist[u]
            if du is None:
                continue
            nd = du + w
            if dist[v] is None or nd < dist[v]:
                dist[v], par[v], ch = nd, i, True
        if not ch:
            return dist, par
        mark = [0] * V  # 0: unseen, else the walk that saw the node
        for v0 in range(V):
            v = v0
            while v != s and par[v] >= 0 and not mark[v]:
                mark[v] = v0 + 1
                v = edges[par[v]][0]
            if v != s and par[v] >= 0 and mark[v] == v0 + 1:
                return None, None
    return None, None


class EvRef(Ref):
    def solve(self, forbid, bias=None):
        """Ref.solve on G_{F,B}: `bias` maps ORF indices to integers B.  NEGCYCLE when the Bellman-Ford does not settle."""
        gone = {self.orf_edge[k] for k in forbid} - {None}
        add = {}
        for k, B in (bias or {}).items():
            if self.orf_edge[k] is not None:  # an ORF without an edge in the graph is ignored
                add[self.orf_edge[k]] = add.get(self.orf_edge[k], 0) + B
        edges = [(u, v, w + add.get((u, v), 0)) for u, v, w in self.edges if (u, v) not in gone]
        dist, par = settle(self.V, edges, self.V - 2)
        if dist is None:
            return NEGCYCLE
        if dist[self.V - 1] is None:
            return None, [], [], dist, edges
        path, v = [self.V - 1], self.V - 1
        while v != self.V - 2:
            v = edges[par[v]][0]
            path.append(v)
            assert len(path) <= self.V
        path.reverse()
        genes = []
        for k in range((len(path) - 1) // 2):
            a, b = path[2 * k + 1], path[2 * k + 2]
            left, right, fr = self.pos[a], self.pos[b] + 2, self.frame[a]
            strand = -1 if fr < 0 else 1
            genes.append((left, right, strand, fr, -20.0 if abs(fr) == 4 else self.weight.get((left, right, strand), 0.0)))
        return dist[self.V - 1], path, genes, dist, edges


def check(ann, ref, forbid, bias, st, genes, delta, D):
    """One contig's result against the yardstick; returns NEGCYCLE, None (no path) or D_B."""
    sol = ref.solve(forbid or [], bias)
    i = ref.i
    if sol == NEGCYCLE:
        assert st == -9 and delta == np.inf and len(genes) == 0, (i, forbid, bias, st)
        assert len(ann.reannotated_path(i)[0]) == 0
        return NEGCYCLE
    DB, path, want = sol[:3]
    if DB is None:
        assert st == 1 and delta == np.inf and len(genes) == 0, (i, forbid, bias, st)
        return None
    assert st == 0, (i, forbid, bias, st)
    got_path, got_D = ann.reannotated_path(i)
    assert got_D == DB, (i, forbid, bias, got_D, DB)
    assert float(delta) == float(DB - D) / 1000.0, (i, forbid, bias, float(delta), DB - D)
    assert got_path.tolist() == path, (i, forbid, bias)
    assert gene_tuples(genes) == want, (i, forbid, bias)
    return DB


def evidence(ann, bias, forbid=None, solve_all=False):
    """Annotator.evidence with integer B per ORF: bias = per contig None or {ORF index: B}."""
    return ann.evidence([None if b is None else [(k, score(B)) for k, B in b.items()] for b in bias], forbid, solve_all=solve_all)


def ev_bytes(ann, bias, forbid=None, i=None, solve_all=False):
    st, offs, genes, delta = evidence(ann, bias, forbid, solve_all)
    if i is None:
        return st.tobytes(), offs.tobytes(), genes.tobytes(), delta.tobytes()
    return int(st[i]), genes[offs[i]:offs[i + 1]].tobytes(), delta[i].tobytes(), ann.reannotated_path(i)[0].tobytes()


def called_orfs(ann, i, genes):
    return [ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in genes if abs(int(g["frame"])) <= 3]


def solved_contigs(ann, st0):
    return [i for i in range(ann.n) if st0[i] == 0 and int(ann.globals(i).n_node) > 2]


@pytest.fixture(scope="module")
def small(pa):
    """fuzz(11, 6), run once: (ann, the run's download, a yardstick and the run's D per solved contig).  The tests leave the batch resident."""
    ann = pa.Annotator()
    dl = run_batch(ann, fuzz(11, 6))
    idx = solved_contigs(ann, dl[0])
    assert len(idx) >= 5
    yield ann, dl, {i: EvRef(ann, i) for i in idx}, {i: ann.path(i)[1] for i in idx}
    ann.close()


def test_the_quick_yardstick_is_the_conftest_one(small):
    ann, dl, refs, D = small
    i = sorted(refs)[0]
    ref = refs[i]
    assert settle(ref.V, ref.edges, ref.V - 2) == inorder_bellman_ford(ref.V, ref.edges, ref.V - 2)
    k = next(k for k, e in enumerate(ref.orf_edge) if e is not None)
    for B in (-5, 900, -(10 ** 9)):  # the last one: far beyond any cycle's length, if the ORF lies on one
        edges = [(u, v, w + (B if (u, v) == ref.orf_edge[k] else 0)) for u, v, w in ref.edges]
        assert settle(ref.V, edges, ref.V - 2) == inorder_bellman_ford(ref.V, edges, ref.V - 2)


# ---- 1. zero bias ----
def check_zero_bias(ann, rng):
    n = ann.n
    st0, offs0, genes0 = ann.download_flat(exact=False)
    none = [None] * n
    want = reann_bytes(ann, none)
    paths = [ann.reannotated_path(i)[0].tobytes() for i in range(n) if st0[i] >= 0]
    assert ev_bytes(ann, none) == want
    assert ev_bytes(ann, none, solve_all=True) == want == (st0.tobytes(), offs0.tobytes(), genes0.tobytes(), want[3])  # the run's genes, ties included
    assert [ann.reannotated_path(i)[0].tobytes() for i in range(n) if st0[i] >= 0] == paths
    mask = [called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])[::3] or None if st0[i] == 0 else None for i in range(n)]
    zeros = [None if st0[i] < 0 or not len(ann.orfs(i)) else {int(k): 0 for k in rng.choice(len(ann.orfs(i)), 3)} for i in range(n)]
    st, offs, genes, delta = ann.reannotate(mask)
    want = (st.tobytes(), offs.tobytes(), genes.tobytes(), delta.tobytes())
    assert ev_bytes(ann, none, mask) == want and ev_bytes(ann, zeros, mask) == want
    # what b holds beyond three decimals is cut off: |b| < 0.001 is no evidence
    tiny = [None if z is None else [(k, 0.00099 * (-1) ** k) for k in z] for z in zeros]
    st, offs, genes, delta = ann.evidence(tiny, mask)
    assert (st.tobytes(), offs.tobytes(), genes.tobytes(), delta.tobytes()) == want
    return sum(m is not None for m in mask)


def test_zero_bias_is_reannotate_byte_for_byte(pa, small):
    rng = np.random.RandomState(1901)
    n = check_zero_bias(small[0], rng)
    for case in golden_cases():
        g, name, seq = load_golden(case)
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        tr = golden_trnas(g)
        run_batch(ann, [seq], None if tr is None else [tr])
        n += check_zero_bias(ann, rng)
        ann.close()
    assert n >= 15


def test_zero_bias_and_nothing_refused_gives_the_run_ties_included(pa):
    seqs = fuzz(7, 300)
    ann = pa.Annotator()
    ties = 0
    for b0 in range(0, 300, 100):
        st0, offs0, genes0 = run_batch(ann, seqs[b0:b0 + 100])
        paths = [ann.path(i)[0].tobytes() if st0[i] >= 0 else None for i in range(100)]
        st, offs, genes, delta = ann.evidence([None] * 100, solve_all=True)
        assert (st.tobytes(), offs.tobytes(), genes.tobytes()) == (st0.tobytes(), offs0.tobytes(), genes0.tobytes())
        assert [ann.reannotated_path(i)[0].tobytes() if st0[i] >= 0 else None for i in range(100)] == paths
        ties += sum(int(ann.globals(i).tie) != 0 for i in range(100))
    ann.close()
    assert ties >= 2, ties


# ---- 2. penalties ----
def draw_orfs(ref, called, rng, m):
    """m ORFs with an edge, called ones among them."""
    have = [k for k, e in enumerate(ref.orf_edge) if e is not None]
    pick = set(rng.choice(have, min(m, len(have)), replace=False).tolist())
    pick.update(called[k] for k in rng.choice(len(called), min(2, len(called)), replace=False))
    return sorted(pick)


def check_penalties(ann, refs, D, dl, rng):
    st0, offs0, genes0 = dl
    n = ann.n
    called = {i: called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]]) for i in refs}
    bias = [{k: int(rng.choice([1, 7, 999, 12345, 10 ** 7])) for k in draw_orfs(refs[i], called[i], rng, 8)} if i in refs else None for i in range(n)]
    forbid = [sorted(set(called[i][1::4]) - set(bias[i])) if i in refs else None for i in range(n)]
    seen = 0
    for fb in (None, forbid):
        st, offs, genes, delta = evidence(ann, bias, fb)
        for i in refs:
            got = check(ann, refs[i], fb[i] if fb else [], bias[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], D[i])
            assert got != NEGCYCLE and (got is None or delta[i] >= 0), i
            seen += got is not None
    return seen


def test_penalties_against_the_yardstick(small):
    ann, dl, refs, D = small
    assert check_penalties(ann, refs, D, dl, np.random.RandomState(1902)) >= 10


@pytest.mark.parametrize("case", range(4))
def test_penalties_in_the_wide_classes(pa, case):
    seqs, nl = wide_cases(pa)[case]
    ann = pa.Annotator()
    dl = run_batch(ann, seqs)
    want = (4, 8, 8, 17)[case]  # 256, 512, 512 and 1088 bits
    i = next(i for i in range(len(seqs)) if dl[0][i] == 0 and int(ann.globals(i).n_limbs) == want)
    assert check_penalties(ann, {i: EvRef(ann, i)}, {i: ann.path(i)[1]}, dl, np.random.RandomState(1903 + case)) >= 2
    ann.close()


def test_the_largest_penalty_is_a_refusal(small):
    ann, dl, refs, D = small
    st0, offs0, genes0 = dl
    n = ann.n
    seen = 0
    for r in range(2):
        F = [called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])[r::5] or None if i in refs else None for i in range(n)]
        st, offs, genes, delta = ann.reannotate(F)
        st, offs, genes, delta = st.copy(), offs.copy(), genes.copy(), delta.copy()
        pst, poffs, pgenes, pdelta = evidence(ann, [None if f is None else {k: B_MAX for k in f} for f in F])
        for i in refs:
            if F[i] is None or st[i] != 0:
                continue
            assert pst[i] == 0 and pgenes[poffs[i]:poffs[i + 1]].tobytes() == genes[offs[i]:offs[i + 1]].tobytes() and pdelta[i].tobytes() == delta[i].tobytes(), (i, r)
            seen += 1
    assert seen >= 8


# ---- 3. margin titration: the smallest bonus that gets an ORF called is its path margin ----
def test_margin_titration(pa):
    """For uncalled ORFs k with through == 1 and a finite margin, Delta = round(margin * 1000) < 2^50 (a called ORF has Delta = 0 and
    -Delta + 1 would be a penalty on the path itself, about which the theorem says nothing; an uncalled ORF with Delta = 0 — an equal-length
    alternative — is titrated like any other): B(k) = -Delta + 1 leaves D alone (delta == 0.0), -Delta ties (delta == 0.0, the path the
    in-order rule's), -Delta - 1 wins by one unit (delta == -0.001, k among the genes).  Each point equals the yardstick; a point where its
    Bellman-Ford does not settle — the bonus has made a cycle through k negative — must be PHX_S_NEGCYCLE on the device, and only those are."""
    from test_scenarios_gpu import case1_seqs

    ann = pa.Annotator()
    dl = run_batch(ann, case1_seqs(pa) + fuzz(11, 6))
    n = ann.n
    idx = solved_contigs(ann, dl[0])
    refs = {i: EvRef(ann, i) for i in idx}
    D = {i: ann.path(i)[1] for i in idx}
    mst, moffs, mrec = ann.margins()
    rng = np.random.RandomState(1904)
    picks = {}
    for i in idx:
        rec = mrec[moffs[i]:moffs[i + 1]]
        ok = [k for k in range(len(rec)) if rec["through"][k] == 1 and rec["called"][k] == 0 and np.isfinite(rec["margin"][k]) and round(float(rec["margin"][k]) * 1000) < 1 << 50]
        take = sorted(rng.choice(ok, min(len(ok), 10 if i >= 3 else 4), replace=False).tolist())  # (the three contigs of case1 are the long ones)
        picks[i] = [(k, int(round(float(rec["margin"][k]) * 1000))) for k in take]
    points = left_out = clean = 0
    for r in range(max(len(p) for p in picks.values())):
        ok_at = {i: 0 for i in idx if r < len(picks[i])}
        for step in (1, 0, -1):
            bias = [{picks[i][r][0]: -picks[i][r][1] + step} if i in ok_at else None for i in range(n)]
            st, offs, genes, delta = evidence(ann, bias)
            for i in ok_at:
                k, Delta = picks[i][r]
                g = genes[offs[i]:offs[i + 1]]
                got = check(ann, refs[i], [], bias[i], int(st[i]), g, delta[i], D[i])
                points += 1
                if got == NEGCYCLE:
                    left_out += 1
                    continue
                assert got is not None
                assert float(delta[i]) == (0.0 if step >= 0 else -0.001), (i, k, Delta, step)
                if step < 0:
                    assert k in called_orfs(ann, i, g), (i, k, Delta)
                ok_at[i] += 1
        clean += sum(c == 3 for c in ok_at.values())
    ann.close()
    print("titration: %d points, %d left out (negative cycle), %d ORFs clean at all three" % (points, left_out, clean))
    assert 3 * left_out <= points and clean >= 20, (points, left_out, clean)


# ---- 4. mixed bonuses and penalties ----
def test_mixed_signs_against_the_yardstick_negative_cycles_included(pa):
    ann = pa.Annotator()
    dl = run_batch(ann, fuzz(11, 12))
    st0, offs0, genes0 = dl
    n = ann.n
    idx = solved_contigs(ann, st0)
    refs = {i: EvRef(ann, i) for i in idx}
    D = {i: ann.path(i)[1] for i in idx}
    rng = np.random.RandomState(1905)
    neg = ok = lower = 0
    for lo, hi in ((1, 4), (4, 9), (3, 12)):  # |B| from 10^lo to 10^hi: a hundredth of a SCORE unit up to far beyond every weight
        bias = []
        for i in range(n):
            if i not in refs:
                bias.append(None)
                continue
            ks = draw_orfs(refs[i], called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]]), rng, 10)
            bias.append({k: int(rng.choice([-1, 1]) * 10 ** rng.uniform(lo, hi)) for k in ks})
        st, offs, genes, delta = evidence(ann, bias)
        for i in refs:
            got = check(ann, refs[i], [], bias[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], D[i])
            neg += got == NEGCYCLE
            ok += got not in (NEGCYCLE, None)
            lower += got not in (NEGCYCLE, None) and delta[i] < 0
    ann.close()
    print("mixed signs: %d settled (%d with a negative delta), %d negative cycles" % (ok, lower, neg))
    assert ok >= 12 and lower >= 1 and neg >= 1, (ok, lower, neg)


# ---- 5. invariance and isolation ----
def some_bias(ann, seed):
    """Per solved contig three uncalled ORFs with a bonus and one called gene with a penalty."""
    rng = np.random.RandomState(seed)
    st0, offs0, genes0 = ann.download_flat(exact=False)
    out = []
    for i in range(ann.n):
        cg = called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]]) if st0[i] == 0 else []
        if not cg:
            out.append(None)
            continue
        b = {int(k): -int(rng.randint(1, 30000)) for k in rng.choice(len(ann.orfs(i)), min(3, len(ann.orfs(i))), replace=False)}
        b[cg[len(cg) // 2]] = 5000
        out.append(b)
    return out


def test_lone_contig_and_batch_give_the_same_bytes(pa):
    seqs = fuzz(23, 36)
    ann = pa.Annotator()
    run_batch(ann, seqs)
    bias = some_bias(ann, 1906)
    evidence(ann, bias)
    got = {i: ev_bytes(ann, bias, i=i) for i in range(2, 36, 7) if bias[i] is not None}
    assert len(got) >= 3
    for i, want in got.items():
        lone = pa.Annotator()
        run_batch(lone, [seqs[i]])
        assert ev_bytes(lone, [bias[i]], i=0) == want, i
        lone.close()
    ann.close()


def test_create_flags_give_the_same_bytes(pa):
    batches = ([pa.synth_contig(61, 14000), pa.synth_contig(62, 9000)], fuzz(5, 20))

    def outs(flags):
        ann = pa.Annotator(flags=flags)
        res = []
        for seqs in batches:
            st0 = run_batch(ann, seqs)[0]
            res.append(ev_bytes(ann, some_bias(ann, 1907)))
            res.append([ann.reannotated_path(i)[0].tobytes() for i in range(len(seqs)) if st0[i] == 0])
        ann.close()
        return res

    want = outs(())
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        assert outs((fl,)) == want, fl


def test_evidence_disturbs_nothing_is_cached_and_is_invalidated_by_the_next_batch(pa):
    a, b = fuzz(31, 20), fuzz(32, 20)

    def everything(ann):
        st0, offs0, genes0 = ann.download_flat(exact=False)
        mask = [called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])[:2] or None for i in range(ann.n)]
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()],
                [x.tobytes() for x in ann.replacements()], reann_bytes(ann, mask), [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n)])

    ann = pa.Annotator()
    run_batch(ann, a)
    before = everything(ann)
    bias = some_bias(ann, 1908)
    r1 = ev_bytes(ann, bias)
    ms = ann.reannotate_ms()
    assert ms["solve"] > 0
    assert ev_bytes(ann, bias) == r1 and ann.reannotate_ms() == ms  # the second identical call reuses the solve: no kernel ran
    assert everything(ann) == before
    assert ev_bytes(ann, bias) == r1
    other = pa.Annotator()  # the evidence first, then everything else
    run_batch(other, a)
    assert ev_bytes(other, bias) == r1 and everything(other) == before
    other.close()
    ann.upload(b)
    for call in (lambda: ann.reannotated_path(0), lambda: ann.evidence([None] * 20)):
        with pytest.raises(pa.PhxError) as e:
            call()
        assert e.value.code == -13
    ann.run()
    with pytest.raises(pa.PhxError) as e:
        ann.reannotated_path(0)
    assert e.value.code == -13
    fresh = pa.Annotator()
    run_batch(fresh, b)
    bias = some_bias(fresh, 1909)
    assert ev_bytes(ann, bias) == ev_bytes(fresh, bias)
    for x in (ann, fresh):
        x.close()


# ---- 6. statuses ----
def test_statuses_in_one_mixed_batch(pa):
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops
    good = [pa.synth_contig(322, 9000).decode(), pa.synth_contig(323, 7000).decode()]
    bad = pa.synth_contig(324, 3000).decode()[:1500] + "x" + pa.synth_contig(324, 3000).decode()[1500:]
    seqs = [bad, "acg", unreachable, "t" * 80, good[0], good[1]]  # a run error twice, no path, an empty graph (two nodes), two healthy contigs
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    assert st0.tolist()[:4] == [-2, -3, 1, 0] and int(ann.globals(3).n_node) == 2
    bias = [None] * 6
    bias[2] = {0: -700} if len(ann.orfs(2)) else None
    for i in (4, 5):
        bias[i] = {called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])[0]: 4000, 3: -2500}
    for solve_all in (False, True):
        st, offs, genes, delta = evidence(ann, bias, solve_all=solve_all)
        assert st.tolist() == [-2, -3, 1, 0, 0, 0]
        assert np.diff(offs).tolist()[:4] == [0] * 4 and (delta[:3] == np.inf).all() and delta[3] == 0.0 and np.isfinite(delta[4:]).all()
        for k, i in enumerate((4, 5)):
            lone = pa.Annotator()
            run_batch(lone, [good[k]])
            assert ev_bytes(lone, [bias[i]], i=0) == ev_bytes(ann, bias, i=i, solve_all=solve_all)
            lone.close()
    # |B| beyond 2^52 and offsets that are not the batch's: PHX_E_ARG before any kernel runs; the float path raises ValueError
    oo = ann.orf_offsets().copy()
    B = np.zeros(int(oo[-1]) + 8, np.int64)
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    offs, st, delta, total = np.zeros(7, np.int64), np.zeros(6, np.int32), np.zeros(6), C.c_int64()
    call = lambda bias, o: ann.L.phx_evidence_flat(ann.h, vp(bias), None, vp(o), 0, None, 0, vp(offs), vp(st), vp(delta), C.byref(total))
    assert call(B, oo) == 0 and call(None, oo) == 0  # (bias and forbid may be NULL)
    for x in (B_MAX + 1, -B_MAX - 1, np.iinfo(np.int64).min):
        B[int(oo[4]) + 1] = x
        assert call(B, oo) == -1
    B[int(oo[4]) + 1] = -B_MAX
    assert call(B, oo) == 0
    for wrong in (oo + 1, np.concatenate([oo[:-1], [oo[-1] + 1]])):
        assert call(B, np.ascontiguousarray(wrong, np.int64)) == -1
    for b in (float("nan"), float("inf"), 2.0 ** 52 / 1000.0 * 1.01):
        with pytest.raises(ValueError):
            ann.evidence([None] * 4 + [[(0, b)], None])
    with pytest.raises(IndexError):
        ann.evidence([None] * 4 + [[(10 ** 6, 1.0)], None])
    ann.close()
    early = pa.Annotator()
    early.upload([pa.synth_contig(5, 5000)])
    with pytest.raises(pa.PhxError) as e:
        early.evidence([None])
    assert e.value.code == -13
    early.close()


# ---- 8. the CLI ----
def test_cli_evidence_alone_and_with_forbid(pa, tmp_path):
    from phanotate_amd.cli import format_reannotation

    g, name, phix = load_golden("phiX174")
    fasta = tmp_path / "phix.fasta"
    fasta.write_text(">%s\n%s\n" % (name, phix))
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, [phix])
    orfs = ann.orfs(0)
    cds = [x for x in genes0 if abs(int(x["frame"])) <= 3]
    rows = []  # (ORF index, the line's first four columns)
    for k in [int(x) for x in np.random.RandomState(1910).choice(len(orfs), 4, replace=False)] + called_orfs(ann, 0, cds[:2]):
        o = orfs[k]
        a, z = (int(o["start"]), int(o["stop"]) + 2) if o["frame"] > 0 else (int(o["start"]) + 2, int(o["stop"]))
        assert ann.orf_index(0, min(a, z), max(a, z), 1 if o["frame"] > 0 else -1) == k
        rows.append((k, "%d\t%d\t%s\t%s" % (a, z, "+" if o["frame"] > 0 else "-", name)))
    vals = [-30.0, -2.5, 1.25, -8.0, 4.0, 0.75]
    ev = tmp_path / "ev.txt"
    ev.write_text("# hits\n" + "".join("%s\t%r\n" % (ln, b) for (k, ln), b in zip(rows, vals)) + "%s\t-1.5\tagain\n" % rows[0][1])  # the first ORF twice: the sum
    fb = tmp_path / "fb.txt"
    fb.write_text(rows[5][1] + "\n")
    want_bias = [[(k, b) for (k, ln), b in zip(rows, vals)] + [(rows[0][0], -1.5)]]
    for extra, forbid in (([], None), (["--forbid", str(fb)], [[rows[5][0]]])):
        out = tmp_path / ("out%d.txt" % len(extra))
        run = subprocess.run(exe + ["--evidence", str(ev), "--reannotation", str(out)] + extra, capture_output=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        st, offs, genes, delta = ann.evidence(want_bias, forbid)
        assert out.read_text() == format_reannotation([name], st, offs, genes, delta)
        assert ("#delta:\t" + repr(float(delta[0]))) in out.read_text()
    bogus = "17\t23\t+\t%s\t1.0" % name
    ev.write_text(bogus + "\n")
    err = subprocess.run(exe + ["--evidence", str(ev), "--reannotation", str(out)], capture_output=True, timeout=600)
    assert err.returncode != 0 and repr(bogus) in err.stderr.decode()
    ann.close()
