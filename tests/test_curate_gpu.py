"""Combined re-annotation on the device (phx_curate_flat, Annotator.curate) against python integers: the yardstick of
tests/test_constrain_gpu.py — the device's own tapped edges, W = trunc(w * 1000), in Graph.iteredges order — with the refused ORF edges
taken out, W + B on the biased ones and - M on the required ones, M a power of two above four times sum |W| + sum |B|, solved by
test_evidence_gpu.settle: an in-place Bellman-Ford with a strict '<' that gives up when the parents close a circle (PHX_S_NEGCYCLE).
Expected: count = round(-dist / M), S = dist + count * M, the path along that solve's parents, its genes, delta = float(S - D) / 1000,
unmet = |R| - count."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from test_constrain_gpu import Ref, bytes_of, fuzz, gene_tuples, run_batch, solved, wide_cases, wide_contig
from test_evidence_gpu import score, settle

import curate_draws as cd

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, S_NEGCYCLE, S_NOPATH = -1, -13, -9, 1
B_MAX = 1 << 52


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


class CuRef(Ref):
    """test_constrain_gpu.Ref with a bias: solve() on G_{F,B} under W + B - M·[R']."""

    def solve(self, forbid=(), require=(), bias=None):
        """dict(cycle, S (None: no path), count, path, genes)."""
        gone = {self.orf_edge[k] for k in forbid} - {None}
        pinned = {self.orf_edge[k] for k in require} - {None} - gone
        add = {}
        for k, B in (bias or {}).items():
            if self.orf_edge[k] is not None:  # an ORF without an edge in the graph is ignored
                add[self.orf_edge[k]] = add.get(self.orf_edge[k], 0) + B
        M = 1 << ((sum(abs(w) for _, _, w in self.edges) + sum(abs(B) for B in add.values())).bit_length() + 2)
        edges = [(u, v, w + add.get((u, v), 0) - (M if (u, v) in pinned else 0)) for u, v, w in self.edges if (u, v) not in gone]
        dist, par = settle(self.V, edges, self.V - 2)
        if dist is None:
            return dict(cycle=True, S=None, count=0, path=[], genes=[])
        d = dist[self.V - 1]
        if d is None:
            return dict(cycle=False, S=None, count=0, path=[], genes=[])
        count = (-d + M // 2) // M  # round(-dist / M)
        path, v = [self.V - 1], self.V - 1
        while v != self.V - 2:
            v = edges[par[v]][0]
            path.append(v)
            assert len(path) <= self.V
        path.reverse()
        assert count == sum((a, b) in pinned for a, b in zip(path, path[1:]))
        genes = []
        for k in range((len(path) - 1) // 2):
            a, b = path[2 * k + 1], path[2 * k + 2]
            left, right, fr = self.pos[a], self.pos[b] + 2, self.frame[a]
            strand = -1 if fr < 0 else 1
            genes.append((left, right, strand, fr, -20.0 if abs(fr) == 4 else self.weight.get((left, right, strand), 0.0)))
        return dict(cycle=False, S=d + count * M, count=count, path=path, genes=genes)


def check(ann, ref, forbid, require, bias, st, genes, delta, unmet, D):
    """One contig's result against the yardstick; returns the yardstick's solve."""
    sol = ref.solve(forbid or (), require or (), bias)
    i, nreq = ref.i, len(require or ())
    what = (i, list(forbid or ()), list(require or ()), bias)
    if sol["cycle"] or sol["S"] is None:
        assert st == (S_NEGCYCLE if sol["cycle"] else S_NOPATH) and delta == np.inf and len(genes) == 0 and unmet == nreq, (what, st, unmet)
        assert len(ann.reannotated_path(i)[0]) == 0
        return sol
    assert st == 0, (what, st)
    got_path, got_S = ann.reannotated_path(i)
    assert got_S == sol["S"], (what, got_S, sol["S"])
    assert got_path.tolist() == sol["path"], what
    assert gene_tuples(genes) == sol["genes"], what
    assert float(delta) == float(sol["S"] - D) / 1000.0, (what, float(delta), sol["S"] - D)
    assert unmet == nreq - sol["count"], (what, int(unmet), nreq, sol["count"])
    return sol


def curate(ann, bias=None, forbid=None, require=None, solve_all=False):
    """Annotator.curate with integer B per ORF: bias = None or per contig None or {ORF index: B}."""
    fb = None if bias is None else [None if b is None else [(k, score(B)) for k, B in b.items()] for b in bias]
    return ann.curate(fb, forbid, require, solve_all=solve_all)


def evidence(ann, bias, forbid=None, solve_all=False):
    return ann.evidence([None if b is None else [(k, score(B)) for k, B in b.items()] for b in bias], forbid, solve_all=solve_all)


def paths(ann, st0):
    return [ann.reannotated_path(i)[0].tobytes() if st0[i] >= 0 else None for i in range(ann.n)]


def contig_bytes(ann, res, i):
    """What one contig got: status, its genes, delta, unmet (0 where the call has none) and the tapped path with its length."""
    st, offs, genes, delta = res[:4]
    p, S = ann.reannotated_path(i)
    return int(st[i]), genes[offs[i]:offs[i + 1]].tobytes(), delta[i].tobytes(), int(res[4][i]) if len(res) > 4 else 0, p.tobytes(), S


def unsettle(ann):
    """A solve under another key, so that the next call computes instead of answering from the cache."""
    ann.reannotate([None] * ann.n, solve_all=True)


class Batch:
    """A batch after its run: the download, a yardstick per solved contig, the margins, and per contig the called / uncalled-but-reachable ORFs."""

    def __init__(self, ann, seqs):
        self.ann, self.seqs, self.n = ann, seqs, len(seqs)
        self.dl = self.st0, self.offs0, self.genes0 = run_batch(ann, seqs)
        self.mst, self.moffs, self.mrec = ann.margins()
        self.idx = [i for i in range(self.n) if solved(ann, self.st0, i) and self.mst[i] == 0]
        self.refs = {i: CuRef(ann, i) for i in self.idx}
        self.D = {i: ann.path(i)[1] for i in self.idx}
        self.called = {i: self.refs[i].called(self.genes0[self.offs0[i]:self.offs0[i + 1]]) for i in self.idx}

    def rec(self, i):
        return self.mrec[self.moffs[i]:self.moffs[i + 1]]

    def reachable(self, i):
        """Uncalled ORFs some path runs through, in an order that does not depend on the batch."""
        rec = self.rec(i)
        return sorted(np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0].tolist(), key=lambda k: (int(rec["left"][k]), int(rec["right"][k]), int(rec["strand"][k])))

    def per_contig(self, fn):
        return [fn(i) if i in self.refs else None for i in range(self.n)]

    def check_all(self, res, forbid, require, bias):
        st, offs, genes, delta, unmet = res
        out = {}
        for i in self.idx:
            if (forbid and forbid[i]) or (require and require[i]) or (bias and bias[i]):
                out[i] = check(self.ann, self.refs[i], forbid and forbid[i], require and require[i], bias and bias[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), self.D[i])
        return out


@pytest.fixture(scope="module")
def small(pa):
    """case1_seqs + fuzz(11, 6), run once; the tests leave the batch resident."""
    ann = pa.Annotator()
    b = Batch(ann, cd.mix_seqs(pa))
    assert len(b.idx) >= 8
    yield b
    ann.close()


def sets_of(b, seed):
    """Per solved contig: two reachable uncalled ORFs to require, a called gene to refuse, a bonus on an uncalled ORF and a penalty on a called gene."""
    rng = np.random.RandomState(seed)
    forbid, require, bias = [None] * b.n, [None] * b.n, [None] * b.n
    for i in b.idx:
        pool, cg = b.reachable(i), b.called[i]
        if len(pool) < 3 or len(cg) < 2:
            continue
        a = int(rng.randint(len(pool) - 2))
        require[i] = [pool[a], pool[a + 1]]
        forbid[i] = [cg[int(rng.randint(len(cg) - 1))]]
        bias[i] = {pool[a + 2]: -int(rng.randint(1, 30000)), cg[-1]: 5000}
        if cg[-1] in forbid[i]:
            del bias[i][cg[-1]]
    return forbid, require, bias


# ---- 1. the reductions ----
def test_the_three_reductions_byte_for_byte(small):
    b, ann = small, small.ann
    n = b.n
    forbid, require, bias = sets_of(b, 2210)
    assert sum(r is not None for r in require) >= 6
    zeros = [None if x is None else {k: 0 for k in x} for x in bias]
    for solve_all in (False, True):
        # B == 0: phx_constrain_flat
        want = bytes_of(ann.constrain(forbid, require, solve_all=solve_all))
        wp = paths(ann, b.st0)
        for bz in (None, [None] * n, zeros):
            unsettle(ann)
            assert bytes_of(curate(ann, bz, forbid, require, solve_all)) == want and paths(ann, b.st0) == wp
        # R empty: phx_evidence_flat, unmet 0
        unsettle(ann)
        want = bytes_of(evidence(ann, bias, forbid, solve_all))
        wp = paths(ann, b.st0)
        for rq in (None, [None] * n, [[] for _ in range(n)]):
            unsettle(ann)
            got = curate(ann, bias, forbid, rq, solve_all)
            assert bytes_of(got[:4]) == want and got[4].tolist() == [0] * n and paths(ann, b.st0) == wp
        # both: phx_reannotate_flat
        want = bytes_of(ann.reannotate(forbid, solve_all=solve_all))
        wp = paths(ann, b.st0)
        ann.constrain(None, require)
        got = curate(ann, None, forbid, None, solve_all)
        assert bytes_of(got[:4]) == want and got[4].tolist() == [0] * n and paths(ann, b.st0) == wp
    # (the three differ from one another and from the full mix: the test means something)
    assert bytes_of(curate(ann, bias, forbid, require)) != bytes_of(ann.constrain(forbid, require))


# ---- 2. random mixes ----
class DeviceGraph:
    """What curate_draws.mixes needs of a contig, from the device's yardstick."""

    def __init__(self, ref, called):
        self.ok = True
        self.orf_edge = {key: ref.orf_edge[k] for key, k in ref.by_ends.items() if ref.orf_edge[k] is not None}
        back = {k: key for key, k in ref.by_ends.items()}
        self.called = {back[k] for k in called}


class NoGraph:
    ok = False


def test_random_mixes_against_the_yardstick(small, oracle):
    b, ann = small, small.ann
    graphs = [DeviceGraph(b.refs[i], b.called[i]) if i in b.refs else NoGraph() for i in range(b.n)]
    for g, seq in zip(graphs, b.seqs):  # the draws are the ones tests/test_curate_host.py counts on the oracle's graphs
        og = cd.OracleGraph(oracle, seq)
        assert g.ok == og.ok and (not g.ok or (sorted(g.orf_edge) == sorted(og.orf_edge) and g.called == og.called))
    draws = ok = neg = kept = 0
    for row in cd.mixes(graphs):
        forbid, require, bias = [None] * b.n, [None] * b.n, [None] * b.n
        for i, d in enumerate(row):
            if d is not None:
                by = b.refs[i].by_ends
                forbid[i], require[i], bias[i] = [by[k] for k in d["forbid"]], [by[k] for k in d["require"]], {by[k]: B for k, B in d["bias"].items()}
                draws += 1
        sols = b.check_all(curate(ann, bias, forbid, require), forbid, require, bias)
        ok += sum(not s["cycle"] and s["S"] is not None for s in sols.values())
        neg += sum(s["cycle"] for s in sols.values())
        kept += sum(s["count"] for s in sols.values())
    print("random mixes: %d draws, %d settle with status 0 (%d required ORFs kept), %d negative cycles" % (draws, ok, kept, neg))
    assert draws >= 40 and ok >= 30 and kept >= 30, (draws, ok, neg, kept)


# ---- 3. a bias on a required ORF that is kept ----
def test_a_bias_on_a_kept_required_orf_moves_the_sum_by_exactly_b(small):
    b, ann = small, small.ann
    require = b.per_contig(lambda i: b.reachable(i)[len(b.reachable(i)) // 3:][:1] or None)
    st, offs, genes, delta, unmet = [x.copy() for x in ann.constrain(None, require)]
    base = {i: (ann.reannotated_path(i)[0].tolist(), ann.reannotated_path(i)[1]) for i in b.idx if require[i] and st[i] == 0 and unmet[i] == 0}
    assert len(base) >= 6
    for B in (777, -555, 12345678):
        bias = [{require[i][0]: B} if i in base else None for i in range(b.n)]
        req = [require[i] if i in base else None for i in range(b.n)]
        res = curate(ann, bias, None, req)
        b.check_all(res, None, req, bias)
        for i, (p0, S0) in base.items():
            p, S = ann.reannotated_path(i)
            assert res[0][i] == 0 and res[4][i] == 0 and p.tolist() == p0 and S == S0 + B, (i, B, S, S0)
            g, g0 = res[2][res[1][i]:res[1][i + 1]], genes[offs[i]:offs[i + 1]]
            assert g.tobytes() == g0.tobytes()  # each gene carries its ORF's own score, not the biased one
            assert float(res[3][i]) == float(S0 + B - b.D[i]) / 1000.0


# ---- 4. two starts of one stop group ----
def test_a_bias_flips_which_of_two_required_starts_is_kept(pa):
    ann = pa.Annotator()
    b = Batch(ann, fuzz(11, 60)[:24])
    rng = np.random.RandomState(1604)
    require, pairs = [None] * b.n, {}
    for i in b.idx:
        orfs, rec = ann.orfs(i), b.rec(i)
        ok = np.nonzero((rec["through"] == 1) & np.isfinite(rec["margin"]))[0]
        grp = {}
        for k in ok:
            grp.setdefault(int(orfs["group"][k]), []).append(int(k))
        cand = [(a, c) for ks in grp.values() for a in ks for c in ks if a < c and 0 < abs(float(rec["margin"][a]) - float(rec["margin"][c])) < 2.0 ** 30]  # (a bias is at most 2^52 / 1000)
        if cand and len(pairs) < 12:
            pairs[i] = cand[rng.randint(len(cand))]
            require[i] = list(pairs[i])
    assert len(pairs) >= 8
    st, offs, genes, delta, unmet = ann.constrain(None, require)
    cheap, dear, bias = {}, {}, [None] * b.n
    for i, (a, c) in pairs.items():
        if st[i] != 0:
            continue
        rec = b.rec(i)
        cheap[i], dear[i] = (a, c) if rec["margin"][a] < rec["margin"][c] else (c, a)
        called = b.refs[i].called(genes[offs[i]:offs[i + 1]])
        assert unmet[i] == 1 and cheap[i] in called and dear[i] not in called
        bias[i] = {dear[i]: -int(round((float(rec["margin"][dear[i]]) - float(rec["margin"][cheap[i]])) * 1000.0)) - 1000}  # one SCORE unit past the tie
    res = curate(ann, bias, None, [require[i] if i in cheap else None for i in range(b.n)])
    sols = b.check_all(res, None, [require[i] if i in cheap else None for i in range(b.n)], bias)
    flipped = 0
    for i, sol in sols.items():
        if sol["cycle"]:
            continue
        called = b.refs[i].called(res[2][res[1][i]:res[1][i + 1]])
        assert res[4][i] == 1 and dear[i] in called and cheap[i] not in called, (i, pairs[i])
        flipped += 1
    ann.close()
    assert flipped >= 6, (flipped, len(sols))


# ---- 5. refused and biased; the argument checks ----
def test_a_refused_orfs_bias_is_ignored_and_bad_arguments_are_refused(pa, small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 2211)
    loud = [None if x is None else {**x, forbid[i][0]: -40000} for i, x in enumerate(bias)]  # a bonus on the refused gene as well
    only = [None if f is None else {f[0]: -40000} for f in forbid]  # ... and nothing else
    want = bytes_of(curate(ann, bias, forbid, require))
    wp = paths(ann, b.st0)
    unsettle(ann)
    assert bytes_of(curate(ann, loud, forbid, require)) == want and paths(ann, b.st0) == wp
    want = bytes_of(ann.constrain(forbid, require))
    unsettle(ann)
    assert bytes_of(curate(ann, only, forbid, require)) == want
    # an ORF both refused and required, |B| beyond 2^52: PHX_E_ARG before any kernel, the last result stands
    i = next(i for i in b.idx if require[i])
    both = [None] * b.n
    both[i] = require[i]
    with pytest.raises(pa.PhxError) as e:
        curate(ann, bias, both, both)
    assert e.value.code == E_ARG
    oo = ann.orf_offsets().copy()
    N = int(oo[-1])
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    offs, st, delta, um, total = np.zeros(b.n + 1, np.int64), np.zeros(b.n, np.int32), np.zeros(b.n), np.zeros(b.n, np.int32), C.c_int64()
    call = lambda B, F, R: ann.L.phx_curate_flat(ann.h, vp(B), vp(F), vp(R), vp(oo), 0, None, 0, vp(offs), vp(st), vp(delta), vp(um), C.byref(total))
    Bv, R = np.zeros(N + 8, np.int64), np.zeros(N + 8, np.uint8)
    R[int(oo[i]) + require[i][0]] = 1
    assert call(None, None, None) == 0 and call(Bv, None, R) == 0 and um[i] in (0, 1)
    for x in (B_MAX + 1, -B_MAX - 1, np.iinfo(np.int64).min):
        Bv[int(oo[i]) + require[i][1]] = x
        assert call(Bv, None, R) == E_ARG and call(Bv, None, None) == E_ARG
    Bv[int(oo[i]) + require[i][1]] = -B_MAX
    assert call(Bv, None, R) == 0  # (the largest bonus there is: a status per contig, not an argument error)
    assert call(Bv, R, R) == E_ARG
    assert ann.L.phx_curate_flat(ann.h, vp(Bv), None, vp(R), vp(oo), 0, None, 0, vp(offs), vp(st), vp(delta), None, C.byref(total)) == E_ARG  # no unmet array
    for bad in (float("nan"), float("inf"), 2.0 ** 52 / 1000.0 * 1.01):
        with pytest.raises(ValueError):
            ann.curate([[(0, bad)]] + [None] * (b.n - 1), None, require)
    assert bytes_of(curate(ann, only, forbid, require)) == want


# ---- 6. the wide classes ----
@pytest.mark.parametrize("case", range(4))
def test_one_required_and_one_biased_orf_in_the_wide_classes(pa, case):
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
    rng = np.random.RandomState(2216 + case)
    other = int(pool[rng.randint(len(pool))])
    cg = ref.called(genes0[offs0[c]:offs0[c + 1]])
    D = ann.path(c)[1]
    seen = 0
    for req, bias in (([long_one], {other: -2500, cg[0]: 4000}), ([other], {long_one: -(10 ** 6)}), ([long_one], {long_one: 999})):
        require, bb = [None] * len(seqs), [None] * len(seqs)
        require[c], bb[c] = req, bias
        st, offs, genes, delta, unmet = curate(ann, bb, None, require)
        sol = check(ann, ref, None, req, bias, int(st[c]), genes[offs[c]:offs[c + 1]], delta[c], int(unmet[c]), D)
        seen += not sol["cycle"] and sol["S"] is not None
        for j in range(len(seqs)):  # neighbours keep the run's result
            if j != c:
                assert st[j] == st0[j] and genes[offs[j]:offs[j + 1]].tobytes() == genes0[offs0[j]:offs0[j + 1]].tobytes()
    ann.close()
    assert seen >= 2


# ---- 7. the untiled window, and rows of one tile ----
def test_required_and_biased_rows_in_an_untiled_window_and_in_one_tile(pa, small):
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
    ok = 0
    for req, bias, fb in (([a], {m: -3000}, None), ([m], {m: 500, z: -300}, None), ([a, z], {into[1]: -5000, m: 250}, None), ([into[1]], {a: -700}, own)):
        st, offs, genes, delta, unmet = curate(ann, [bias], [fb], [req])
        sol = check(ann, ref, fb, req, bias, int(st[0]), genes, delta[0], int(unmet[0]), D)
        ok += not sol["cycle"] and sol["S"] is not None
    ann.close()
    assert ok >= 3
    # a tiled window: a required and a biased ORF of one stop group (rows of one node), and of adjacent nodes
    b, ann = small, small.ann
    forbid, require, bias = [None] * b.n, [None] * b.n, [None] * b.n
    for i in b.idx:
        orfs, pool = ann.orfs(i), b.reachable(i)
        grp = {}
        for k in pool:
            grp.setdefault(int(orfs["group"][k]), []).append(k)
        same = [ks for ks in grp.values() if len(ks) >= 2]
        if same:
            ks = same[len(same) // 2]
            near = [k for k in (ks[0] - 1, ks[-1] + 1) if 0 <= k < len(orfs) and b.refs[i].orf_edge[k] is not None]
            require[i], bias[i] = [ks[0]], {ks[1]: -2000, **{k: -1500 for k in near[:1]}}
    assert sum(r is not None for r in require) >= 5
    sols = b.check_all(curate(ann, bias, forbid, require), forbid, require, bias)
    assert sum(not s["cycle"] and s["S"] is not None for s in sols.values()) >= 4


# ---- 8. the tie rule ----
def test_tie_made_by_a_bias_on_a_contig_with_a_required_orf(small):
    """R = {r}.  S1: the best sum with r kept; S2: the best with r and another reachable ORF k kept.  B(k) = -(S2 - S1) makes the best path
    through k as long as the best without it: the device's path must be the one the in-place Bellman-Ford leaves, not merely as long."""
    b, ann = small, small.ann
    picks = {}
    for i in b.idx:
        pool = b.reachable(i)
        if len(pool) < 4:
            continue
        r = pool[len(pool) // 2]
        s1 = b.refs[i].solve((), [r])
        if s1["cycle"] or s1["count"] != 1:
            continue
        for k in (pool[len(pool) // 2 + 1], pool[0], pool[-1]):
            s2 = b.refs[i].solve((), [r, k])
            if not s2["cycle"] and s2["count"] == 2 and s2["S"] > s1["S"]:
                picks[i] = (r, k, s1["S"], s2["S"] - s1["S"])
                break
    assert len(picks) >= 5
    tied = 0
    for step in (1, 0, -1):
        require = [[picks[i][0]] if i in picks else None for i in range(b.n)]
        bias = [{picks[i][1]: -picks[i][3] + step} if i in picks else None for i in range(b.n)]
        res = curate(ann, bias, None, require)
        sols = b.check_all(res, None, require, bias)
        for i, sol in sols.items():
            if sol["cycle"]:
                continue
            r, k, S1, gap = picks[i]
            assert sol["S"] == (S1 if step >= 0 else S1 - 1) and res[4][i] == 0
            if step < 0:
                assert k in b.refs[i].called(res[2][res[1][i]:res[1][i + 1]])
            tied += step == 0
    assert tied >= 4


# ---- 9. negative cycles ----
def test_negative_cycles_by_a_required_edge_by_a_bias_and_out_of_reach(pa):
    from phanotate_amd.fasta import read_fasta

    seqs = [seq for name, seq in read_fasta(os.path.join(ROOT, "tests", "golden", "constrain_cycle.fasta"))]
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops  # no path: what lies behind the first stops is out of the source's reach
    seqs = seqs + [pa.synth_contig(61, 9000), unreachable]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    assert st0.tolist() == [0, 0, 0, 1]
    seen = made = 0
    for i in (0, 1):
        ref = CuRef(ann, i)
        D = ann.path(i)[1]
        cyc = [k for k, e in enumerate(ref.orf_edge) if e is not None and ref.on_cycle({e})]
        free = [k for k, e in enumerate(ref.orf_edge) if e is not None and k not in cyc]
        assert cyc and len(free) >= 2
        for k in cyc[:2] + cyc[-1:]:
            # a required ORF on a reachable cycle, an unrelated bias
            for req, bias in (([k], {free[0]: 500}), ([k, free[1]], {free[0]: -500})):
                require, bb = [None] * 4, [None] * 4
                require[i], bb[i] = req, bias
                st, offs, genes, delta, unmet = curate(ann, bb, None, require)
                assert st[i] == S_NEGCYCLE and offs[i + 1] == offs[i] and delta[i] == np.inf and unmet[i] == len(req), (i, k, int(st[i]))
                assert len(ann.reannotated_path(i)[0]) == 0
                for j in (0, 1, 2):  # neighbours keep the run's result
                    if j != i:
                        assert st[j] == 0 and genes[offs[j]:offs[j + 1]].tobytes() == genes0[offs0[j]:offs0[j + 1]].tobytes() and delta[j] == 0.0
                seen += 1
            # a cycle the bias makes negative, the required ORF elsewhere
            require, bb = [None] * 4, [None] * 4
            require[i], bb[i] = [free[1]], {k: -(10 ** 9)}
            st, offs, genes, delta, unmet = curate(ann, bb, None, require)
            sol = check(ann, ref, None, require[i], bb[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), D)
            assert sol["cycle"] and st[i] == S_NEGCYCLE and unmet[i] == 1 and delta[i] == np.inf
            made += 1
            # refusing the ORF takes either cycle away
            fb = [None] * 4
            fb[i] = [k]
            st, offs, genes, delta, unmet = curate(ann, bb, fb, require)
            sol = check(ann, ref, fb[i], require[i], bb[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), D)
            assert not sol["cycle"]
    # cycles the source cannot reach are no cycles of the solve: the contig without a path stays without one
    ref = CuRef(ann, 3)
    quiet = [k for k, e in enumerate(ref.orf_edge) if e is None or not ref.on_cycle({e})]
    apart = [k for k in quiet if ref.orf_edge[k] is not None and ref.on_cycle({ref.orf_edge[k]}, anywhere=True)]
    print("negative cycles: the contig without a path has %d ORFs, %d on a cycle the source does not reach" % (len(ref.orfs), len(apart)))
    assert len(apart) >= 2  # one ORF on an unreached cycle to require, another one to give a bonus beyond any cycle's length
    require, bb = [None] * 4, [None] * 4
    require[3] = sorted({apart[0], quiet[0]})
    bb[3] = {apart[1]: -(10 ** 9), apart[0]: -700}
    st, offs, genes, delta, unmet = curate(ann, bb, None, require)
    sol = check(ann, ref, None, require[3], bb[3], int(st[3]), genes[offs[3]:offs[4]], delta[3], int(unmet[3]), 0)
    assert not sol["cycle"] and st[3] == S_NOPATH and unmet[3] == len(require[3])
    ann.close()
    assert seen >= 12 and made >= 6


# ---- 10. one batch, five policies ----
def test_a_batch_with_every_policy_equals_the_lone_single_policy_calls(small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 2213)
    full = [i for i in b.idx if require[i]]
    assert len(full) >= 5
    role = {full[0]: 0, full[1]: 1, full[2]: 2, full[3]: 3}  # the run's result, refused only, required only, biased only; the others all three
    F = [forbid[i] if role.get(i, 4) in (1, 4) and i in full else None for i in range(b.n)]
    R = [require[i] if role.get(i, 4) in (2, 4) and i in full else None for i in range(b.n)]
    Bs = [bias[i] if role.get(i, 4) in (3, 4) and i in full else None for i in range(b.n)]
    res = [x.copy() for x in curate(ann, Bs, F, R)]
    got = {i: contig_bytes(ann, res, i) for i in full}
    b.check_all(res, F, R, Bs)
    lone = lambda x, i: [x[j] if j == i else None for j in range(b.n)]
    for i in full:
        unsettle(ann)
        r = role.get(i, 4)
        if r == 0:
            assert got[i][:4] == (0, b.genes0[b.offs0[i]:b.offs0[i + 1]].tobytes(), np.float64(0.0).tobytes(), 0) and got[i][4] == ann.path(i)[0].tobytes()
            continue
        one = ann.reannotate(lone(F, i)) if r == 1 else ann.constrain(None, lone(R, i)) if r == 2 else evidence(ann, lone(Bs, i)) if r == 3 else curate(ann, lone(Bs, i), lone(F, i), lone(R, i))
        assert contig_bytes(ann, one, i) == got[i], (i, r)
    # solve_all: the contig without a set is solved again and gives the run
    assert contig_bytes(ann, curate(ann, Bs, F, R, solve_all=True), full[0]) == got[full[0]]


# ---- 11. determinism ----
def keyed(ann, i, ks):
    o = ann.orfs(i)
    return [(int(o["start"][k]), int(o["stop"][k]), int(o["frame"][k])) for k in ks]


def test_lone_contig_and_batch_and_create_flags_give_the_same_bytes(pa, small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 2214)
    res = [x.copy() for x in curate(ann, bias, forbid, require)]
    full = [i for i in b.idx if require[i]]
    for i in full[1::3]:
        want = contig_bytes(ann, res, i)
        lone = pa.Annotator()
        run_batch(lone, [b.seqs[i]])
        where = {key: k for k, key in enumerate(keyed(lone, 0, range(len(lone.orfs(0)))))}
        at = lambda ks: [where[key] for key in keyed(ann, i, ks)]
        one = curate(lone, [dict(zip(at(list(bias[i])), bias[i].values()))], [at(forbid[i])], [at(require[i])])
        assert contig_bytes(lone, one, 0) == want, i
        lone.close()
    want = bytes_of(res), paths(ann, b.st0)
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        other = pa.Annotator(flags=(fl,))
        run_batch(other, b.seqs)
        assert (bytes_of(curate(other, bias, forbid, require)), paths(other, b.st0)) == want, fl
        other.close()


# ---- 12. side effects and the cache ----
def test_curate_disturbs_nothing_caches_rightly_and_is_invalidated(pa):
    a, nxt = fuzz(31, 12), fuzz(32, 12)
    ann = pa.Annotator()
    b = Batch(ann, a)

    def everything():
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()], [ann.path(i)[0].tobytes() for i in range(ann.n)])

    forbid, require, bias = sets_of(b, 2215)
    assert sum(r is not None for r in require) >= 5
    before = everything()
    c_want = bytes_of(ann.constrain(forbid, require))
    r1 = bytes_of(curate(ann, bias, forbid, require))
    p1 = paths(ann, b.st0)
    ms = ann.reannotate_ms()
    assert ms["solve"] > 0 and r1[2:4] != c_want[2:4]
    assert bytes_of(curate(ann, bias, forbid, require)) == r1 and ann.reannotate_ms() == ms  # the second identical call reuses the solve: no kernel ran
    assert everything() == before
    assert bytes_of(curate(ann, bias, forbid, require)) == r1 and paths(ann, b.st0) == p1
    # the same F and R without the bias must be solved again, and the reverse
    assert bytes_of(ann.constrain(forbid, require)) == c_want
    assert bytes_of(curate(ann, bias, forbid, require)) == r1 and paths(ann, b.st0) == p1
    # margins on the re-annotation's graph: refused after a solve that pinned a contig, served after one that reduces to evidence()
    with pytest.raises(pa.PhxError) as e:
        ann.remargins()
    assert e.value.code == E_STATE
    ev = bytes_of(curate(ann, bias, forbid, None))
    rm = [x.tobytes() for x in ann.remargins()]
    evidence(ann, bias, forbid)
    assert [x.tobytes() for x in ann.remargins()] == rm and bytes_of(evidence(ann, bias, forbid)) == ev[:4]
    assert everything() == before
    fresh = pa.Annotator()  # a context that never ran anything else
    run_batch(fresh, a)
    assert bytes_of(curate(fresh, bias, forbid, require)) == r1 and paths(fresh, b.st0) == p1
    fresh.close()
    # the next batch invalidates
    ann.upload(nxt)
    for call in (lambda: ann.reannotated_path(0), lambda: ann.curate(None, None, None)):
        with pytest.raises(pa.PhxError) as e:
            call()
        assert e.value.code == E_STATE
    ann.run()
    with pytest.raises(pa.PhxError) as e:
        ann.reannotated_path(0)
    assert e.value.code == E_STATE
    st, offs, genes, delta, unmet = ann.curate(None, None, None)
    assert bytes_of((st, offs, genes)) == bytes_of(ann.download_flat(exact=False)) and unmet.tolist() == [0] * 12
    ann.close()
