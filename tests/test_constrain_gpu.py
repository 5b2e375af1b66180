"""Pinned re-annotation on the device (phx_constrain_flat, Annotator.constrain) against python integers over the device's own
tapped edges in Graph.iteredges order: an in-place Bellman-Ford with a strict '<' (conftest.inorder_bellman_ford) on the edge list without
the refused ORF edges, the required ORF edges carrying W - M with M = 1 << 4000.  Expected: count = round(-dist / M), W-sum = dist +
count * M, the path along that solve's parents, its genes, delta = float(W-sum - D) / 1000, unmet = |R| - count."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_cases, golden_params, golden_trnas, inorder_bellman_ford, load_golden

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

BIG_M = 1 << 4000
E_ARG, E_STATE, S_NEGCYCLE, S_NOPATH, S_OVERFLOW = -1, -13, -9, 1, -7


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def fuzz(seed, n):
    import fuzz_gpu

    rng = np.random.RandomState(seed)
    return [fuzz_gpu.make(rng) for _ in range(n)]


class Ref:
    """The yardstick for one contig (the helper of tests/test_reannotate_gpu.py with a required set): its tapped graph in the reference's
    edge order and the ORF edges by index in orfs(i)."""

    def __init__(self, ann, i):
        from phanotate_amd.functions import edge_order

        self.i = i
        g = ann.globals(i)
        self.V = int(g.n_node)
        self.nd = nd = ann.nodes(i)
        ed = ann.edges(i)
        src, dst = ed["src"].tolist(), ed["dst"].tolist()
        w = [int(math.trunc(float(x) * 1000.0)) for x in ed["w"]]
        self.edges = [(src[k], dst[k], w[k]) for k in edge_order(nd, ed)]
        self.orfs = orfs = ann.orfs(i)
        ids = {(int(p), int(t), 1 if f > 0 else -1): v for v, (p, t, f) in enumerate(zip(nd["pos"], nd["type"], nd["frame"])) if t in (0, 1) and abs(int(f)) <= 3}
        have = {(u, v) for u, v, _ in self.edges}
        self.orf_edge, self.by_ends, self.weight = [], {}, {}
        for k, o in enumerate(orfs):
            fwd = o["frame"] > 0
            s = ids.get((int(o["start"]), 0, 1 if fwd else -1))
            t = ids.get((int(o["stop"]), 1, 1 if fwd else -1))
            e = (s, t) if fwd else (t, s)
            self.orf_edge.append(e if e in have else None)  # an ORF without an edge in the graph is ignored
            left, right = (int(o["start"]), int(o["stop"]) + 2) if fwd else (int(o["stop"]), int(o["start"]) + 2)
            self.by_ends.setdefault((left, right, 1 if fwd else -1), k)
            self.weight.setdefault((left, right, 1 if fwd else -1), float(o["weight"]))
        self.pos, self.frame = nd["pos"].tolist(), nd["frame"].tolist()

    def on_cycle(self, pinned, gone=frozenset(), anywhere=False):
        """Some edge of `pinned` lies on a cycle of the graph without the edges `gone` — both ends in one strongly connected component —
        that a path from the source reaches: the Bellman-Ford from the source never settles then.  (anywhere: reached or not.)"""
        out = [[] for _ in range(self.V)]
        for u, v, _ in self.edges:
            if (u, v) not in gone:
                out[u].append(v)
        reach, todo = {self.V - 2}, [self.V - 2]
        while todo:
            for w in out[todo.pop()]:
                if w not in reach:
                    reach.add(w)
                    todo.append(w)
        index, low, comp, stack, on, n = [-1] * self.V, [0] * self.V, [-1] * self.V, [], [False] * self.V, 0
        for root in range(self.V):  # Tarjan, without recursion
            if index[root] >= 0:
                continue
            work = [(root, 0)]
            while work:
                v, k = work.pop()
                if k == 0:
                    index[v] = low[v] = n
                    n += 1
                    stack.append(v)
                    on[v] = True
                if k < len(out[v]):
                    work.append((v, k + 1))
                    w = out[v][k]
                    if index[w] < 0:
                        work.append((w, 0))
                    elif on[w]:
                        low[v] = min(low[v], index[w])
                    continue
                if low[v] == index[v]:
                    while True:
                        w = stack.pop()
                        on[w] = False
                        comp[w] = v
                        if w == v:
                            break
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
        return any(comp[u] == comp[v] and (anywhere or u in reach) for u, v in pinned)

    def solve(self, forbid, require=()):
        """dict(cycle, W (None: no path), count, path, genes) without the ORFs `forbid`, keeping those of `require`."""
        gone = {self.orf_edge[k] for k in forbid} - {None}
        pinned = {self.orf_edge[k] for k in require} - {None} - gone
        edges = [e for e in self.edges if (e[0], e[1]) not in gone] if gone else self.edges
        if pinned:
            edges = [(u, v, w - BIG_M) if (u, v) in pinned else (u, v, w) for u, v, w in edges]
        if pinned and self.on_cycle(pinned, gone):  # W' has a cycle of negative length (the Bellman-Ford below would only run out of rounds on it)
            return dict(cycle=True, W=None, count=0, path=[], genes=[])
        dist, par = inorder_bellman_ford(self.V, edges, self.V - 2)
        assert dist is not None
        d = dist[self.V - 1]
        if d is None:
            return dict(cycle=False, W=None, count=0, path=[], genes=[])
        count = (-d + BIG_M // 2) // BIG_M  # round(-dist / M)
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
        return dict(cycle=False, W=d + count * BIG_M, count=count, path=path, genes=genes)

    def called(self, genes):
        """ORF indices of the CDS genes of a gene array."""
        return [self.by_ends[(int(g["left"]), int(g["right"]), int(g["strand"]))] for g in genes if abs(int(g["frame"])) <= 3]


def gene_tuples(genes):
    return [(int(g["left"]), int(g["right"]), int(g["strand"]), int(g["frame"]), float(g["score"])) for g in genes]


def check_against_ref(ann, ref, forbid, require, st, genes, delta, unmet, D):
    """One contig's result against the yardstick; returns the yardstick's solve."""
    sol = ref.solve(forbid or (), require or ())
    i, nreq = ref.i, len(require or ())
    what = (i, list(forbid or ()), list(require or ()))
    if sol["cycle"] or sol["W"] is None:
        assert st == (S_NEGCYCLE if sol["cycle"] else S_NOPATH) and delta == np.inf and len(genes) == 0 and unmet == nreq, (what, st, unmet)
        if not sol["cycle"]:
            assert len(ann.reannotated_path(i)[0]) == 0
        return sol
    assert st == 0, (what, st)
    got_path, got_W = ann.reannotated_path(i)
    assert got_W == sol["W"], (what, got_W, sol["W"])
    assert got_path.tolist() == sol["path"], what
    assert gene_tuples(genes) == sol["genes"], what
    assert float(delta) == float(sol["W"] - D) / 1000.0 and (delta >= 0 or nreq == 0), (what, float(delta), sol["W"] - D)
    assert unmet == nreq - sol["count"], (what, int(unmet), nreq, sol["count"])
    return sol


def run_batch(ann, seqs, trnas=None):
    ann.upload(seqs)
    ann.set_trnas(trnas)
    ann.run()
    return ann.download_flat(exact=False)


def golden_runs(pa, skip=("edge_huge",)):
    """(case, annotator after a run of the fixture) for the fixtures that annotate."""
    for case in golden_cases():
        g, name, seq = load_golden(case)
        if str(g["error"]) or case in skip:
            continue
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        tr = golden_trnas(g)
        run_batch(ann, [seq], None if tr is None else [tr])
        yield case, ann
        ann.close()


def solved(ann, st0, i):
    return st0[i] == 0 and int(ann.globals(i).n_node) > 2


def bytes_of(res):
    return [np.asarray(x).tobytes() for x in res]


def wide_contig(pa, ncodons, seed, density=None):
    rng = np.random.RandomState(seed)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    if density is None:
        w = np.array([12.0 if c in ("atg", "gtg", "ttg") else 1.0 for c in sense])
        body = "".join(rng.choice(sense, ncodons, p=w / w.sum()))
    else:
        quiet = [c for c in sense if c not in ("atg", "gtg", "ttg")]
        body = "".join("atg" if rng.rand() < density else quiet[rng.randint(len(quiet))] for _ in range(ncodons))
    return pa.synth_contig(900, 4000).decode() + "atg" + body + "taa" + pa.synth_contig(901, 4000).decode()


def wide_cases(pa):
    """The 256 / 512 / 1088-bit inputs of tests/test_drop_gpu.py."""
    rng = np.random.RandomState(3000)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    c256 = [pa.synth_contig(900 + k, 20000).decode() + "atg" + "".join(rng.choice(sense, 3000)) + "taa" + pa.synth_contig(1900 + k, 20000).decode() for k in range(6)]
    return [(c256, 2), ([wide_contig(pa, 8000, 8000, density=0.01)], 8), ([wide_contig(pa, 5500, 42)], 8), ([wide_contig(pa, 12000, 42)], 17)]


# ---- 1. nothing required ----
def called_masks(ann, st0, offs0, genes0, every=3):
    out = []
    for i in range(ann.n):
        cds = [g for g in genes0[offs0[i]:offs0[i + 1]] if abs(int(g["frame"])) <= 3]
        out.append([ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds[::every]] if st0[i] == 0 and cds else None)
    return out


def check_nothing_required(ann, n, st0, offs0, genes0):
    checked = 0
    for forbid in ([None] * n, called_masks(ann, st0, offs0, genes0)):
        for solve_all in (False, True):
            want = ann.reannotate(forbid, solve_all=solve_all)
            wpaths = [ann.reannotated_path(i)[0].tobytes() if st0[i] >= 0 else None for i in range(n)]
            for req in (None, [None] * n, [[] for _ in range(n)]):
                got = ann.constrain(forbid, req, solve_all=solve_all)
                assert bytes_of(got[:4]) == bytes_of(want)
                assert got[4].tolist() == [0] * n
                assert [ann.reannotated_path(i)[0].tobytes() if st0[i] >= 0 else None for i in range(n)] == wpaths
                checked += 1
    return checked


def test_nothing_required_is_reannotate_byte_for_byte(pa):
    seqs = fuzz(11, 60)
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    assert check_nothing_required(ann, 60, st0, offs0, genes0) == 12
    ann.close()
    n = 0
    for case, ann in golden_runs(pa, skip=()):
        st0, offs0, genes0 = ann.download_flat(exact=False)
        n += check_nothing_required(ann, 1, st0, offs0, genes0)
    assert n >= 15 * 12


# ---- 2. a called gene required ----
def test_a_called_gene_required_gives_the_run(pa):
    """... unless a required gene's edge lies on a cycle (short overlapping genes of opposite strands do): then the definition
    asks for PHX_S_NEGCYCLE, and the yardstick says which contigs those are."""
    seqs = fuzz(11, 60)
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    paths = [ann.path(i) if st0[i] >= 0 else None for i in range(60)]
    refs = [Ref(ann, i) if solved(ann, st0, i) else None for i in range(60)]
    n = cyclic = 0
    for every, first in ((1, 0), (4, 1)):  # all called genes; a few of them
        require = called_masks(ann, st0, offs0, genes0, every)
        require = [r[first:] if r else None for r in require]
        st, offs, genes, delta, unmet = ann.constrain(None, require)
        for i in range(60):
            if not require[i] or refs[i] is None:
                assert st[i] == st0[i] and genes[offs[i]:offs[i + 1]].tobytes() == genes0[offs0[i]:offs0[i + 1]].tobytes() and unmet[i] == len(require[i] or [])
                continue
            if refs[i].on_cycle({refs[i].orf_edge[k] for k in require[i]} - {None}):
                assert st[i] == S_NEGCYCLE and offs[i + 1] == offs[i] and delta[i] == np.inf and unmet[i] == len(require[i]), (i, int(st[i]))
                cyclic += 1
                continue
            assert st[i] == 0 and genes[offs[i]:offs[i + 1]].tobytes() == genes0[offs0[i]:offs0[i + 1]].tobytes(), (i, int(st[i]))
            p, W = ann.reannotated_path(i)
            assert p.tolist() == paths[i][0].tolist() and W == paths[i][1] and delta[i] == 0.0 and unmet[i] == 0, (i, float(delta[i]), int(unmet[i]))
            n += 1
    ann.close()
    print("a called gene required: %d contigs give the run, %d have a required gene on a cycle" % (n, cyclic))
    assert n >= 50 and n > cyclic, (n, cyclic)


# ---- 3. one uncalled ORF required ----
def check_one_uncalled(ann, n, rng, rounds):
    st0, offs0, genes0 = ann.download_flat(exact=False)
    mst, moffs, mrec = ann.margins()
    refs = [Ref(ann, i) if solved(ann, st0, i) else None for i in range(n)]
    D = [ann.path(i) if refs[i] else None for i in range(n)]
    finite = dead = 0
    for r in range(rounds):
        require = [None] * n
        for i in range(n):
            if refs[i] is None or mst[i] != 0:
                continue
            rec = mrec[moffs[i]:moffs[i + 1]]
            assert len(rec) == len(refs[i].orfs)
            # alternately an ORF some path runs through and, where the contig has one, an ORF none does
            pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0]
            none = np.nonzero(rec["through"] == 0)[0]
            if r % 2 and len(none):
                pool = none
            if len(pool):
                require[i] = [int(pool[rng.randint(len(pool))])]
        st, offs, genes, delta, unmet = ann.constrain(None, require)
        for i in range(n):
            if require[i] is None:
                assert st[i] == st0[i] and genes[offs[i]:offs[i + 1]].tobytes() == genes0[offs0[i]:offs0[i + 1]].tobytes() and unmet[i] == 0, i
                continue
            k = require[i][0]
            sol = check_against_ref(ann, refs[i], None, require[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), D[i][1])
            if sol["cycle"]:
                continue
            rec = mrec[moffs[i] + k]
            if rec["through"]:
                assert unmet[i] == 0 and delta[i].tobytes() == rec["margin"].tobytes(), (i, k, float(delta[i]), float(rec["margin"]))
                assert k in refs[i].called(genes[offs[i]:offs[i + 1]]), (i, k)
                finite += 1
            else:
                assert unmet[i] == 1 and delta[i] == 0.0 and genes[offs[i]:offs[i + 1]].tobytes() == genes0[offs0[i]:offs0[i + 1]].tobytes(), (i, k)
                assert ann.reannotated_path(i)[0].tolist() == D[i][0].tolist()
                dead += 1
    return finite, dead


def test_one_uncalled_orf_required_on_fuzz_contigs(pa):
    seqs = fuzz(11, 60)
    ann = pa.Annotator()
    run_batch(ann, seqs)
    finite, dead = check_one_uncalled(ann, 60, np.random.RandomState(1601), 6)
    ann.close()
    print("one uncalled ORF required, fuzz contigs: %d with a finite margin, %d that no path runs through" % (finite, dead))
    assert finite >= 150 and dead >= 20, (finite, dead)


def test_one_uncalled_orf_required_on_the_golden_fixtures(pa):
    rng = np.random.RandomState(1602)
    finite = dead = 0
    for case, ann in golden_runs(pa):
        f, d = check_one_uncalled(ann, 1, rng, 4)
        finite, dead = finite + f, dead + d
    print("one uncalled ORF required, golden fixtures: %d with a finite margin, %d that no path runs through" % (finite, dead))
    assert finite >= 25 and dead >= 1, (finite, dead)


# ---- 4. several required ----
def test_several_required_compatible_and_not(pa):
    seqs = fuzz(11, 60)
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    rng = np.random.RandomState(1603)
    refs = [Ref(ann, i) if solved(ann, st0, i) else None for i in range(60)]
    D = [ann.path(i)[1] if refs[i] else None for i in range(60)]
    checked = partial = full = 0
    for r in range(5):
        require = [None] * 60
        for i in range(60):
            if refs[i] is None or len(refs[i].orfs) < 6:
                continue
            n_orf = len(refs[i].orfs)
            m = int(rng.randint(2, 6))
            if r % 2:  # neighbours in the ORF list: the starts of one stop group, overlapping frames — incompatible mixes
                a = int(rng.randint(0, n_orf - m + 1))
                require[i] = list(range(a, a + m))
            else:
                require[i] = sorted(rng.choice(n_orf, m, replace=False).tolist())
        st, offs, genes, delta, unmet = ann.constrain(None, require)
        for i in range(60):
            if require[i] is None:
                continue
            sol = check_against_ref(ann, refs[i], None, require[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), D[i])
            checked += 1
            if not sol["cycle"] and sol["W"] is not None:
                partial += 0 < sol["count"] < len(require[i])
                full += sol["count"] == len(require[i]) and sol["count"] >= 2
    ann.close()
    print("several required: %d solves, %d keep a part of R, %d keep all of two or more" % (checked, partial, full))
    assert checked >= 200 and partial >= 40 and full >= 10, (checked, partial, full)


# ---- 5. two starts of one stop group ----
def test_two_starts_of_one_stop_group_keep_the_cheaper(pa):
    seqs = fuzz(11, 60)
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    mst, moffs, mrec = ann.margins()
    rng = np.random.RandomState(1604)
    seen = 0
    for r in range(3):
        require, pairs = [None] * 60, {}
        for i in range(60):
            if not solved(ann, st0, i) or mst[i] != 0:
                continue
            orfs, rec = ann.orfs(i), mrec[moffs[i]:moffs[i + 1]]
            ok = np.nonzero((rec["through"] == 1) & np.isfinite(rec["margin"]))[0]
            grp = {}
            for k in ok:
                grp.setdefault(int(orfs["group"][k]), []).append(int(k))
            cand = [(a, b) for ks in grp.values() for a in ks for b in ks if a < b and rec["margin"][a] != rec["margin"][b]]
            if cand:
                pairs[i] = cand[rng.randint(len(cand))]
                require[i] = list(pairs[i])
        st, offs, genes, delta, unmet = ann.constrain(None, require)
        for i, (a, b) in pairs.items():
            ref = Ref(ann, i)
            sol = check_against_ref(ann, ref, None, [a, b], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), ann.path(i)[1])
            if sol["cycle"]:
                continue
            rec = mrec[moffs[i]:moffs[i + 1]]
            cheap = a if rec["margin"][a] < rec["margin"][b] else b
            called = ref.called(genes[offs[i]:offs[i + 1]])
            assert unmet[i] == 1 and cheap in called and (a + b - cheap) not in called, (i, a, b)
            assert delta[i].tobytes() == rec["margin"][cheap].tobytes()
            seen += 1
    ann.close()
    assert seen >= 40, seen


# ---- 6. require and forbid together ----
def test_require_and_forbid_together(pa):
    seqs = fuzz(11, 60)
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    mst, moffs, mrec = ann.margins()
    rng = np.random.RandomState(1605)
    refs = [Ref(ann, i) if solved(ann, st0, i) and mst[i] == 0 else None for i in range(60)]
    D = [ann.path(i)[1] if refs[i] else None for i in range(60)]
    a_seen = b_seen = 0
    # (a) a required uncalled ORF, every other ORF of its stop group refused
    require, forbid = [None] * 60, [None] * 60
    for i in range(60):
        if refs[i] is None:
            continue
        orfs, rec = refs[i].orfs, mrec[moffs[i]:moffs[i + 1]]
        pool = [int(k) for k in np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0] if (orfs["group"] == orfs["group"][k]).sum() >= 2]
        if pool:
            k = pool[rng.randint(len(pool))]
            require[i] = [k]
            forbid[i] = [int(x) for x in np.nonzero(orfs["group"] == orfs["group"][k])[0] if x != k]
    st, offs, genes, delta, unmet = ann.constrain(forbid, require)
    for i in range(60):
        if require[i] is None:
            continue
        sol = check_against_ref(ann, refs[i], forbid[i], require[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), D[i])
        if not sol["cycle"]:
            assert unmet[i] == 0 and require[i][0] in refs[i].called(genes[offs[i]:offs[i + 1]])
            a_seen += 1
    # (b) a called gene refused while the called gene next to it is required
    require, forbid = [None] * 60, [None] * 60
    for i in range(60):
        if refs[i] is None:
            continue
        cg = refs[i].called(genes0[offs0[i]:offs0[i + 1]])
        if len(cg) >= 2:
            j = int(rng.randint(len(cg) - 1))
            forbid[i], require[i] = [cg[j]], [cg[j + 1]]
    st, offs, genes, delta, unmet = ann.constrain(forbid, require)
    for i in range(60):
        if require[i] is None:
            continue
        sol = check_against_ref(ann, refs[i], forbid[i], require[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), D[i])
        if sol["W"] is not None:
            called = refs[i].called(genes[offs[i]:offs[i + 1]])
            assert forbid[i][0] not in called and (unmet[i] == 1 or require[i][0] in called)
            b_seen += 1
    assert a_seen >= 25 and b_seen >= 30, (a_seen, b_seen)
    # the same ORF in both sets: refused before any kernel, the last result stands
    before = bytes_of(ann.constrain(forbid, require))
    i = next(i for i in range(60) if require[i] is not None)
    both = [None] * 60
    both[i] = require[i]
    with pytest.raises(pa.PhxError) as e:
        ann.constrain(both, both)
    assert e.value.code == E_ARG
    assert bytes_of(ann.constrain(forbid, require)) == before
    ann.close()


# ---- 7. the wide classes ----
def test_one_required_orf_in_the_wide_classes(pa):
    rng = np.random.RandomState(1606)
    seen = set()
    for seqs, nl in wide_cases(pa):
        ann = pa.Annotator()
        st0, offs0, genes0 = run_batch(ann, seqs)
        mst, moffs, mrec = ann.margins()
        c = int(np.argmax([int(ann.globals(i).n_limbs) if st0[i] == 0 else 0 for i in range(len(seqs))]))  # the widest contig of the batch
        assert st0[c] == 0 and mst[c] == 0
        seen.add(int(ann.globals(c).n_limbs))
        ref = Ref(ann, c)
        rec = mrec[moffs[c]:moffs[c + 1]]
        pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0]
        # the widest ORF weights sit in the long ORF's group: one of its starts, and one ORF drawn from all
        picks = [int(pool[np.argmax(ref.orfs["length"][pool])]), int(pool[rng.randint(len(pool))])]
        for k in picks:
            require = [None] * len(seqs)
            require[c] = [k]
            st, offs, genes, delta, unmet = ann.constrain(None, require)
            sol = check_against_ref(ann, ref, None, [k], int(st[c]), genes[offs[c]:offs[c + 1]], delta[c], int(unmet[c]), ann.path(c)[1])
            if not sol["cycle"]:
                assert unmet[c] == 0 and delta[c].tobytes() == rec["margin"][k].tobytes() and k in ref.called(genes[offs[c]:offs[c + 1]])
            for j in range(len(seqs)):  # neighbours keep the run's result
                if j != c:
                    assert st[j] == st0[j] and genes[offs[j]:offs[j + 1]].tobytes() == genes0[offs0[j]:offs0[j + 1]].tobytes()
        ann.close()
    assert {4, 8, 17} <= seen  # (no class reports PHX_S_OVERFLOW: every class is solved on one limb more)


# ---- 8. the tie rule ----
def test_tie_rule_with_a_required_orf(pa):
    """Contigs with equal-length alternatives: the paths must be the yardstick's, not merely as long."""
    seqs = fuzz(101, 300) + fuzz(7, 300)
    ann = pa.Annotator()
    rng = np.random.RandomState(1607)
    pairs = ambiguous = 0
    for b0 in range(0, 600, 100):
        st0, offs0, genes0 = run_batch(ann, seqs[b0:b0 + 100])
        mst, moffs, mrec = ann.margins()
        tied = [i for i in range(100) if solved(ann, st0, i) and mst[i] == 0 and int(ann.globals(i).tie) != 0]
        refs = {i: Ref(ann, i) for i in tied}
        for r in range(3):
            require = [None] * 100
            for i in tied:
                rec = mrec[moffs[i]:moffs[i + 1]]
                pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0]
                if len(pool):
                    require[i] = [int(pool[rng.randint(len(pool))])]
            st, offs, genes, delta, unmet = ann.constrain(None, require)
            for i in tied:
                if require[i] is None:
                    continue
                sol = check_against_ref(ann, refs[i], None, require[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), ann.path(i)[1])
                pairs += 1
                ambiguous += int(ann.globals(i).tie) != 0 and not sol["cycle"]
    ann.close()
    print("tie rule with a required ORF: %d (contig, ORF) pairs on contigs with equal-length alternatives" % pairs)
    assert pairs >= 30 and ambiguous >= 30, (pairs, ambiguous)


# ---- 9. the untiled window ----
def test_a_required_orf_in_an_untiled_window(pa):
    """The input of test_an_untiled_window_in_the_run_and_under_a_mask: a stop node with more in-edges than the solver's tile holds, so
    that window is relaxed from global memory row by row — one of those rows required."""
    ann = pa.Annotator(flags=("solver_no_wave",))
    st0, offs0, genes0 = run_batch(ann, [wide_contig(pa, 6000, 6000, density=0.2)])
    assert st0[0] == 0
    ed = ann.edges(0)
    indeg = np.bincount(ed["dst"])
    big = int(indeg.argmax())
    assert indeg[big] > 1024, int(indeg[big])
    ref = Ref(ann, 0)
    mst, moffs, mrec = ann.margins()
    into = [k for k, e in enumerate(ref.orf_edge) if e is not None and e[1] == big and not mrec[k]["called"] and mrec[k]["through"]]
    assert len(into) > 1000
    D = ann.path(0)[1]
    for k in (into[0], into[len(into) // 2], into[-1]):
        st, offs, genes, delta, unmet = ann.constrain(None, [[k]])
        sol = check_against_ref(ann, ref, None, [k], int(st[0]), genes, delta[0], int(unmet[0]), D)
        assert not sol["cycle"] and unmet[0] == 0 and k in ref.called(genes) and delta[0].tobytes() == mrec[k]["margin"].tobytes()
    # ... and with the called gene of that node refused as well
    own = [g for g in genes0 if abs(int(g["frame"])) <= 3 and int(g["strand"]) == 1 and int(g["right"]) == int(ref.pos[big]) + 2]
    assert len(own) == 1
    forbid = ref.called(own)
    st, offs, genes, delta, unmet = ann.constrain([forbid], [[into[1]]])
    check_against_ref(ann, ref, forbid, [into[1]], int(st[0]), genes, delta[0], int(unmet[0]), D)
    ann.close()


# ---- 10. determinism ----
def constrain_bytes(ann, forbid, require, i=None):
    st, offs, genes, delta, unmet = ann.constrain(forbid, require)
    if i is None:
        return st.tobytes(), offs.tobytes(), genes.tobytes(), delta.tobytes(), unmet.tobytes()
    return int(st[i]), genes[offs[i]:offs[i + 1]].tobytes(), delta[i].tobytes(), int(unmet[i]), ann.reannotated_path(i)[0].tobytes()


def uncalled_picks(ann, n, seed):
    """Per contig two uncalled ORFs some path runs through (required) and a called gene (refused); None where there are none."""
    st0, offs0, genes0 = ann.download_flat(exact=False)
    mst, moffs, mrec = ann.margins()
    rng = np.random.RandomState(seed)
    forbid, require = [None] * n, [None] * n
    for i in range(n):
        if not solved(ann, st0, i) or mst[i] != 0:
            continue
        rec = mrec[moffs[i]:moffs[i + 1]]
        key = lambda k: (int(rec["left"][k]), int(rec["right"][k]), int(rec["strand"][k]))
        pool = sorted(np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0].tolist(), key=key)  # (an order that does not depend on the batch)
        cg = sorted(np.nonzero(rec["called"] == 1)[0].tolist(), key=key)
        if len(pool) >= 2 and cg:
            a = rng.randint(len(pool) - 1)
            require[i] = [pool[a], pool[a + 1]]
            forbid[i] = [cg[rng.randint(len(cg))]]
    return forbid, require


def test_lone_contig_and_batch_of_300_give_the_same_bytes(pa):
    seqs = fuzz(23, 300)
    ann = pa.Annotator()
    run_batch(ann, seqs)
    forbid, require = uncalled_picks(ann, 300, 1608)
    st, offs, genes, delta, unmet = ann.constrain(forbid, require)
    n = 0
    for i in range(5, 300, 37):
        if require[i] is None:
            continue
        got = (int(st[i]), genes[offs[i]:offs[i + 1]].tobytes(), delta[i].tobytes(), int(unmet[i]), ann.reannotated_path(i)[0].tobytes())
        ends = lambda ks: [(int(o["start"]), int(o["stop"]), int(o["frame"])) for o in ann.orfs(i)[ks]]
        lone = pa.Annotator()
        run_batch(lone, [seqs[i]])
        lo = lone.orfs(0)
        where = {(int(o["start"]), int(o["stop"]), int(o["frame"])): k for k, o in enumerate(lo)}
        f1, r1 = [where[e] for e in ends(forbid[i])], [where[e] for e in ends(require[i])]
        assert constrain_bytes(lone, [f1], [r1], 0) == got, i
        lone.close()
        n += 1
    ann.close()
    assert n >= 5


def test_create_flags_give_the_same_bytes(pa):
    small = [pa.synth_contig(61, 14000), pa.synth_contig(62, 9000)]
    medium = fuzz(5, 40)

    def outs(flags):
        ann = pa.Annotator(flags=flags)
        res = []
        for seqs in (small, medium):
            st0, offs0, genes0 = run_batch(ann, seqs)
            forbid, require = uncalled_picks(ann, len(seqs), 1609)
            res.append(constrain_bytes(ann, forbid, require))
            res.append([ann.reannotated_path(i)[0].tobytes() for i in range(len(seqs)) if st0[i] == 0])
        ann.close()
        return res

    want = outs(())
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        assert outs((fl,)) == want, fl


# ---- 11. side effects ----
def test_constrain_disturbs_nothing_shares_the_cache_rightly_and_is_invalidated(pa):
    a, b = fuzz(31, 30), fuzz(32, 30)
    ann = pa.Annotator()
    ann.upload(a)
    with pytest.raises(pa.PhxError) as e:  # before a run
        ann.constrain(None, None)
    assert e.value.code == E_STATE
    ann.run()

    def everything():
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [ann.path(i)[0].tobytes() for i in range(ann.n)])

    forbid, require = uncalled_picks(ann, 30, 1610)
    before = everything()
    r_forbid = bytes_of(ann.reannotate(forbid))
    p_forbid = [ann.reannotated_path(i)[0].tobytes() for i in range(30)]
    c1 = constrain_bytes(ann, forbid, require)
    assert everything() == before
    # the cache: the same forbid set right after a constrain() with a non-empty require set must be solved again, and the reverse
    assert bytes_of(ann.reannotate(forbid)) == r_forbid
    assert [ann.reannotated_path(i)[0].tobytes() for i in range(30)] == p_forbid
    assert constrain_bytes(ann, forbid, require) == c1
    assert constrain_bytes(ann, forbid, require) == c1  # (and the cached one)
    assert bytes_of(ann.reannotate(forbid)) == r_forbid
    assert c1[2] != r_forbid[2]  # (the two differ: the test means something)
    assert everything() == before
    fresh = pa.Annotator()
    fresh.upload(a)
    fresh.run()
    assert constrain_bytes(fresh, forbid, require) == c1  # a context that never ran reannotate()
    fresh.close()
    # the next upload invalidates
    ann.upload(b)
    with pytest.raises(pa.PhxError) as e:
        ann.reannotated_path(0)
    assert e.value.code == E_STATE
    with pytest.raises(pa.PhxError) as e:
        ann.constrain(None, None)
    assert e.value.code == E_STATE
    ann.close()


# ---- 12. statuses ----
def test_statuses_in_one_mixed_batch(pa):
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops
    rng = np.random.RandomState(12)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    huge = pa.synth_contig(320, 2000).decode() + "atg" + "".join(sense[i] for i in rng.randint(0, len(sense), 24000)) + "taa" + pa.synth_contig(321, 2000).decode()
    good = [pa.synth_contig(322, 9000).decode(), pa.synth_contig(323, 7000).decode()]
    bad = pa.synth_contig(324, 3000).decode()[:1500] + "x" + pa.synth_contig(324, 3000).decode()[1500:]
    seqs = [bad, "acg", unreachable, huge, good[0], good[1]]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    assert st0.tolist()[:3] == [-2, -3, 1]
    oo = ann.orf_offsets()
    forbid, require = uncalled_picks(ann, 6, 1611)
    assert require[4] is not None and require[5] is not None
    assert oo[3] - oo[2] >= 2 and oo[4] == oo[3]  # (a contig without device distances counts no ORFs: none of its can be named)
    # the contig without a path: required ORFs on no cycle that the source reaches — and, if it has one, an ORF on a cycle the source does
    # not reach, which is no cycle of the solve.  No result there: every required ORF is unmet.
    ref2 = Ref(ann, 2)
    quiet = [k for k, e in enumerate(ref2.orf_edge) if e is None or not ref2.on_cycle({e})]
    apart = [k for k in quiet if ref2.orf_edge[k] is not None and ref2.on_cycle({ref2.orf_edge[k]}, anywhere=True)]
    assert len(quiet) >= 2
    require[2] = sorted(set([quiet[0], quiet[-1]] + apart[:1]))
    print("statuses: the contig without a path has %d ORFs, %d on a cycle the source reaches, %d on one it does not" % (len(ref2.orfs), len(ref2.orfs) - len(quiet), len(apart)))
    for solve_all in (False, True):
        st, offs, genes, delta, unmet = ann.constrain(forbid, require, solve_all=solve_all)
        assert st.tolist() == [-2, -3, 1, S_OVERFLOW, 0, 0]
        assert np.diff(offs).tolist()[:4] == [0] * 4 and (delta[:4] == np.inf).all() and (delta[4:] >= 0).all() and np.isfinite(delta[4:]).all()
        assert unmet.tolist()[:4] == [0, 0, len(require[2]), 0]
        check_against_ref(ann, ref2, None, require[2], int(st[2]), genes[offs[2]:offs[3]], delta[2], int(unmet[2]), 0)
        for k, i in enumerate((4, 5)):
            lone = pa.Annotator()
            run_batch(lone, [good[k]])
            assert constrain_bytes(lone, [forbid[i]], [require[i]], 0) == constrain_bytes(ann, forbid, require, i)
            lone.close()
            ref = Ref(ann, i)
            check_against_ref(ann, ref, forbid[i], require[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), ann.path(i)[1])
    # offsets that are not the batch's: refused before any kernel runs; NULL sets are empty sets
    import ctypes as C

    oo = oo.copy()
    mask = np.zeros(int(oo[-1]) + 8, np.uint8)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    offs, st, delta, um, total = np.zeros(7, np.int64), np.zeros(6, np.int32), np.zeros(6), np.zeros(6, np.int32), C.c_int64()
    assert ann.L.phx_constrain_flat(ann.h, None, None, vp(oo), 0, None, 0, vp(offs), vp(st), vp(delta), vp(um), C.byref(total)) == 0
    assert st.tolist() == [-2, -3, 1, S_OVERFLOW, 0, 0] and um.tolist() == [0] * 6
    assert ann.L.phx_constrain_flat(ann.h, vp(mask), vp(mask), vp(oo), 0, None, 0, vp(offs), vp(st), vp(delta), vp(um), C.byref(total)) == 0
    for wrong in (oo + 1, np.concatenate([oo[:-1], [oo[-1] + 1]]), np.concatenate([oo[:4], [oo[4] + 1], oo[5:]])):
        wrong = np.ascontiguousarray(wrong, np.int64)
        assert ann.L.phx_constrain_flat(ann.h, vp(mask), vp(mask), vp(wrong), 0, None, 0, vp(offs), vp(st), vp(delta), vp(um), C.byref(total)) == E_ARG
    ann.close()


# ---- 13. the cycle guard ----
def test_a_cycle_through_a_required_edge_is_reported_at_once(pa):
    """tests/golden/constrain_cycle.fasta: two contigs of tools/fuzz_gpu.py's generator (seed 11, the contigs 74 and 0; found by a search
    of its contigs on the CPU oracle's graph, where one ORF edge in 25 lies on a cycle: short ORFs of opposite strands that overlap, joined by
    connectors that reach back).  Requiring such an ORF gives W' a cycle of negative length: PHX_S_NEGCYCLE, no genes, delta +inf — and the
    call returns, the solver having met a distance that counts more required edges than exist."""
    from phanotate_amd.fasta import read_fasta

    names, seqs = [], []
    for name, seq in read_fasta(os.path.join(ROOT, "tests", "golden", "constrain_cycle.fasta")):
        names.append(name)
        seqs.append(seq)
    assert names == ["fuzz11_74", "fuzz11_0"]
    seqs = seqs + [pa.synth_contig(61, 9000)]  # a neighbour
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    assert st0.tolist() == [0, 0, 0]
    seen = 0
    for i in (0, 1):
        ref = Ref(ann, i)
        cyc = [k for k, e in enumerate(ref.orf_edge) if e is not None and ref.on_cycle({e})]
        free = [k for k, e in enumerate(ref.orf_edge) if e is not None and k not in cyc]
        assert cyc and free, (i, len(cyc), len(free))
        for k in cyc[:4] + cyc[-2:]:
            for extra in ([], free[:1]):
                require = [None] * 3
                require[i] = [k] + extra
                st, offs, genes, delta, unmet = ann.constrain(None, require)
                assert st[i] == S_NEGCYCLE and offs[i + 1] == offs[i] and delta[i] == np.inf and unmet[i] == len(require[i]), (i, k, int(st[i]))
                assert len(ann.reannotated_path(i)[0]) == 0
                for j in range(3):  # neighbours keep the run's result
                    if j != i:
                        assert st[j] == 0 and genes[offs[j]:offs[j + 1]].tobytes() == genes0[offs0[j]:offs0[j + 1]].tobytes() and delta[j] == 0.0
                seen += 1
            # refusing an edge of the cycle takes the cycle away: then there is a result again, the yardstick's
        k = cyc[0]
        u, v = ref.orf_edge[k]
        others = [x for x, e in enumerate(ref.orf_edge) if e is not None and x != k]
        lone = [x for x in others if not ref.on_cycle({ref.orf_edge[k]}, {ref.orf_edge[x]})]
        if lone:
            forbid, require = [None] * 3, [None] * 3
            forbid[i], require[i] = [lone[0]], [k]
            st, offs, genes, delta, unmet = ann.constrain(forbid, require)
            sol = check_against_ref(ann, ref, forbid[i], require[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], int(unmet[i]), ann.path(i)[1])
            assert not sol["cycle"]
    ann.close()
    assert seen >= 12


# ---- 14. the CLI ----
def test_cli_require_alone_and_with_forbid(pa, tmp_path):
    from phanotate_amd.cli import format_reannotation

    seqs = {"c1": pa.synth_contig(71, 20000).decode(), "c2": pa.synth_contig(72, 9000).decode()}
    names = list(seqs)
    fasta = tmp_path / "two.fasta"
    fasta.write_text("".join(">%s\n%s\n" % (k, v) for k, v in seqs.items()))
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    plain = subprocess.run(exe, capture_output=True, timeout=600)
    assert plain.returncode == 0
    rows = [ln for ln in plain.stdout.decode().splitlines() if ln and not ln.startswith("#")]
    ann = pa.Annotator()
    ann.upload(list(seqs.values()))
    ann.set_trnas(None)
    ann.run()
    mst, moffs, mrec = ann.margins()

    def line_of(i, rec):  # START STOP FRAME CONTIG as the tabular output prints a gene
        a, z = (int(rec["left"]), int(rec["right"])) if rec["strand"] > 0 else (int(rec["right"]), int(rec["left"]))
        return "%d\t%d\t%s\t%s" % (a, z, "+" if rec["strand"] > 0 else "-", names[i])

    require, req_lines = [None, None], []
    for i in range(2):
        rec = mrec[moffs[i]:moffs[i + 1]]
        pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0]
        k = int(pool[len(pool) // 2])
        require[i] = [k]
        req_lines.append(line_of(i, rec[k]))
        assert ann.orf_index(i, int(rec[k]["left"]), int(rec[k]["right"]), int(rec[k]["strand"])) == k
    rq = tmp_path / "keep.txt"
    rq.write_text("# kept calls\n" + "\n".join(req_lines) + "\n")
    refused = [ln for ln in (rows[1], rows[-2]) if "\t".join(ln.split("\t")[:4]) not in req_lines]
    fb = tmp_path / "refuse.txt"
    fb.write_text("\n".join(refused) + "\n")
    forbid = [None, None]
    for ln in refused:
        a, z, fr, ctg = ln.split("\t")[:4]
        i = names.index(ctg)
        forbid[i] = (forbid[i] or []) + [ann.orf_index(i, min(int(a), int(z)), max(int(a), int(z)), 1 if fr == "+" else -1)]
    out = tmp_path / "out.txt"
    # --require alone
    run = subprocess.run(exe + ["--require", str(rq), "--reannotation", str(out)], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == plain.stdout
    st, offs, genes, delta, unmet = ann.constrain(None, require)
    text = out.read_text()
    assert text == format_reannotation(names, st, offs, genes, delta, unmet)
    assert text.count("#delta:\t") == 2 and text.count("#unmet:\t0\n") == 2 and all((ln + "\t") in text for ln in req_lines)
    lines = text.splitlines()
    assert all(lines[k + 1].startswith("#unmet:\t") for k, ln in enumerate(lines) if ln.startswith("#delta:\t"))
    # --require with --forbid
    run = subprocess.run(exe + ["--forbid", str(fb), "--require", str(rq), "--reannotation", str(out)], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    st, offs, genes, delta, unmet = ann.constrain(forbid, require)
    text = out.read_text()
    assert text == format_reannotation(names, st, offs, genes, delta, unmet)
    assert all((ln + "\t") in text for ln in req_lines) and all(("\t".join(ln.split("\t")[:4]) + "\t") not in text for ln in refused)
    # --forbid alone: byte for byte what it was (no #unmet: line)
    run = subprocess.run(exe + ["--forbid", str(fb), "--reannotation", str(out)], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    st, offs, genes, delta = ann.reannotate(forbid)
    assert out.read_text() == format_reannotation(names, st, offs, genes, delta) and "#unmet:" not in out.read_text()
    ann.close()
    # a line that names no ORF of its contig ends the program with an error that names the flag and quotes the line
    bogus = "17\t23\t+\t%s" % names[0]
    rq.write_text(bogus + "\n")
    err = subprocess.run(exe + ["--require", str(rq), "--reannotation", str(out)], capture_output=True, timeout=600)
    assert err.returncode != 0 and ("--require: no such ORF in its contig: %r" % bogus) in err.stderr.decode()
    rq.write_text("17\t23\t+\tnobody\n")
    err = subprocess.run(exe + ["--require", str(rq), "--reannotation", str(out)], capture_output=True, timeout=600)
    assert err.returncode != 0 and "--require: no such ORF" in err.stderr.decode()
    # the same ORF in both files: the library refuses it
    rq.write_text(req_lines[0] + "\n")
    fb.write_text(req_lines[0] + "\n")
    err = subprocess.run(exe + ["--forbid", str(fb), "--require", str(rq), "--reannotation", str(out)], capture_output=True, timeout=600)
    assert err.returncode != 0
