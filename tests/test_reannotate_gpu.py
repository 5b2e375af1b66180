"""Masked re-annotation on the device (phx_reannotate_flat) against python integers over the device's own tapped edges
(W = trunc(w * 1000)) in Graph.iteredges order (phanotate_amd.functions.edge_order): D_F, delta, the path and the genes are what an
in-place Bellman-Ford with a strict '<' leaves on the edge list without the refused ORF edges (conftest.inorder_bellman_ford).  Also the
empty mask (the device path byte for byte), the tie rule under a mask, the drop margins of §12 as a cross-check, determinism,
non-interference, statuses and the CLI."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_cases, golden_params, golden_trnas, inorder_bellman_ford, load_golden

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def fuzz(seed, n):
    import fuzz_gpu

    rng = np.random.RandomState(seed)
    return [fuzz_gpu.make(rng) for _ in range(n)]


class Ref:
    """The yardstick for one contig: its tapped graph in the reference's edge order and the ORF edges by index in orfs(i)."""

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

    def solve(self, forbid):
        """(D_F, path, genes [(left, right, strand, frame, score)], dist) without the ORFs `forbid`; D_F None: no path."""
        gone = {self.orf_edge[k] for k in forbid} - {None}
        edges = [e for e in self.edges if (e[0], e[1]) not in gone] if gone else self.edges
        dist, par = inorder_bellman_ford(self.V, edges, self.V - 2)
        assert dist is not None
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

    def called(self, genes):
        """ORF indices of the CDS genes of a gene array."""
        return [self.by_ends[(int(g["left"]), int(g["right"]), int(g["strand"]))] for g in genes if abs(int(g["frame"])) <= 3]


def gene_tuples(genes):
    return [(int(g["left"]), int(g["right"]), int(g["strand"]), int(g["frame"]), float(g["score"])) for g in genes]


def check_against_ref(ann, ref, forbid, st, genes, delta, D):
    """One contig's re-annotation without `forbid` against the in-place Bellman-Ford on the list without those edges."""
    sol = ref.solve(forbid)
    DF, path, want = sol[:3]
    i = ref.i
    if DF is None:
        assert st == 1 and delta == np.inf and len(genes) == 0, (i, forbid)
        assert len(ann.reannotated_path(i)[0]) == 0
        return sol
    assert st == 0, (i, forbid, st)
    got_path, got_D = ann.reannotated_path(i)
    assert got_D == DF and DF >= D, (i, forbid, got_D, DF, D)
    assert float(delta) == float(DF - D) / 1000.0, (i, forbid, float(delta), DF - D)
    assert got_path.tolist() == path, (i, forbid)
    assert gene_tuples(genes) == want, (i, forbid)
    return sol


def run_batch(ann, seqs, trnas=None):
    ann.upload(seqs)
    ann.set_trnas(trnas)
    ann.run()
    return ann.download_flat(exact=False)


def check_empty_mask(ann, n):
    """Bit 0 set, nothing refused: every contig is solved again and comes out as the run left it."""
    st0, offs0, genes0 = ann.download_flat(exact=False)
    paths = [ann.path(i) if st0[i] >= 0 else None for i in range(n)]
    st, offs, genes, delta = ann.reannotate([None] * n, solve_all=True)
    assert st.tolist() == st0.tolist() and offs.tolist() == offs0.tolist()
    assert genes.tobytes() == genes0.tobytes()
    solved = 0
    for i in range(n):
        if st0[i] < 0:
            assert delta[i] == np.inf
            continue
        p, D = ann.reannotated_path(i)
        assert p.tolist() == paths[i][0].tolist(), i
        if st0[i] == 0:
            assert delta[i] == 0.0 and D == paths[i][1], i
            solved += int(ann.globals(i).n_node) > 2
        else:
            assert delta[i] == np.inf
    return solved


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


# ---- 1. the empty mask ----
def test_empty_mask_on_every_golden_fixture(pa):
    n = 0
    for case in golden_cases():
        g, name, seq = load_golden(case)
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        tr = golden_trnas(g)
        run_batch(ann, [seq], None if tr is None else [tr])
        n += check_empty_mask(ann, 1)
        ann.close()
    assert n >= 15


def test_empty_mask_on_the_fuzz_contigs_ties_included(pa):
    seqs = fuzz(101, 300) + fuzz(7, 300)
    ann = pa.Annotator()
    solved = ties = 0
    for b0 in range(0, 600, 100):
        run_batch(ann, seqs[b0:b0 + 100])
        ties += sum(int(ann.globals(i).tie) != 0 for i in range(100))
        solved += check_empty_mask(ann, 100)
    ann.close()
    assert solved > 400 and ties >= 5


def test_empty_mask_in_the_wide_classes(pa):
    seen = set()
    for seqs, nl in wide_cases(pa):
        ann = pa.Annotator()
        run_batch(ann, seqs)
        seen.update(int(ann.globals(i).n_limbs) for i in range(len(seqs)))
        assert check_empty_mask(ann, len(seqs)) >= 1
        ann.close()
    assert {4, 8, 17} <= seen


# ---- 2. non-empty masks ----
def mask_rounds(refs, called, rng):
    """Per contig a list of masks: every called gene singly (at most 6, drawn), then three sets of 1-5 % of the ORFs with a called gene each."""
    plans = []
    for ref, cg in zip(refs, called):
        if ref is None or not cg:
            plans.append([])
            continue
        single = cg if len(cg) <= 6 else [cg[k] for k in sorted(rng.choice(len(cg), 6, replace=False).tolist())]
        plan = [[k] for k in single]
        n_orf = len(ref.orfs)
        for _ in range(3):
            m = max(1, int(n_orf * rng.uniform(0.01, 0.05)))
            s = set(rng.choice(n_orf, min(m, n_orf), replace=False).tolist())
            s.add(cg[rng.randint(len(cg))])
            plan.append(sorted(s))
        plans.append(plan)
    return plans


def check_masks(ann, n, rng, contigs=None):
    st0, offs0, genes0 = ann.download_flat(exact=False)
    pick = range(n) if contigs is None else contigs
    refs = [Ref(ann, i) if i in pick and st0[i] == 0 and int(ann.globals(i).n_node) > 2 else None for i in range(n)]
    called = [refs[i].called(genes0[offs0[i]:offs0[i + 1]]) if refs[i] else [] for i in range(n)]
    D = [ann.path(i)[1] if refs[i] else None for i in range(n)]
    plans = mask_rounds(refs, called, rng)
    checked = 0
    for r in range(max([len(p) for p in plans] + [0])):
        forbid = [plans[i][r] if r < len(plans[i]) else None for i in range(n)]
        st, offs, genes, delta = ann.reannotate(forbid)
        for i in range(n):
            if forbid[i] is None:  # the run's result stands
                assert st[i] == st0[i] and genes[offs[i]:offs[i + 1]].tobytes() == genes0[offs0[i]:offs0[i + 1]].tobytes(), i
                continue
            check_against_ref(ann, refs[i], forbid[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], D[i])
            checked += 1
    return checked


def test_masks_on_the_golden_fixtures(pa):
    rng = np.random.RandomState(1401)
    n = 0
    for case in golden_cases():
        g, name, seq = load_golden(case)
        if str(g["error"]) or case == "edge_huge":
            continue
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        tr = golden_trnas(g)
        run_batch(ann, [seq], None if tr is None else [tr])
        n += check_masks(ann, 1, rng)
        ann.close()
    assert n >= 60


def test_masks_on_fuzz_contigs_in_a_batch(pa):
    seqs = fuzz(11, 60)
    ann = pa.Annotator()
    run_batch(ann, seqs)
    assert check_masks(ann, 60, np.random.RandomState(1402)) >= 200
    ann.close()


def test_masks_in_the_wide_classes(pa):
    rng = np.random.RandomState(1403)
    for seqs, nl in wide_cases(pa):
        ann = pa.Annotator()
        run_batch(ann, seqs)
        assert check_masks(ann, len(seqs), rng, contigs=[0]) >= 4
        ann.close()


def test_an_untiled_window_in_the_run_and_under_a_mask(pa):
    """One long ORF with some 1200 in-frame starts: its stop node has more in-edges than the in-edge tile of the windowed solver holds
    (1024 rows; 512 in the 1088-bit class of the re-annotation), so the window's advance nodes alone exceed the tile and both k_sssp_lds
    and k_rs_lds relax that window from global memory, row by row.  The run's distances are exact, the empty mask returns the run's bytes,
    and without the long ORF's own called gene, whose edge is one of those rows, the result is the in-place Bellman-Ford's."""
    from test_gpu_parity import check_exact_distances

    ann = pa.Annotator(flags=("solver_no_wave",))  # k_sssp_lds is the only solver
    st0, offs0, genes0 = run_batch(ann, [wide_contig(pa, 6000, 6000, density=0.2)])
    assert st0[0] == 0
    indeg = np.bincount(ann.edges(0)["dst"])
    big = int(indeg.argmax())
    assert indeg[big] > 1024, int(indeg[big])
    check_exact_distances(ann, 0)
    assert check_empty_mask(ann, 1) == 1
    ref = Ref(ann, 0)
    own = [g for g in genes0 if abs(int(g["frame"])) <= 3 and int(g["strand"]) == 1 and int(g["right"]) == int(ref.pos[big]) + 2]
    assert len(own) == 1  # the called gene that ends at the node of many in-edges
    forbid = ref.called(own)
    st, offs, genes, delta = ann.reannotate([forbid])
    check_against_ref(ann, ref, forbid, int(st[0]), genes, delta[0], ann.path(0)[1])
    ann.close()


# ---- 3. the tie rule under a mask ----
def test_tie_rule_under_a_mask(pa):
    """Contigs with equal-length alternatives (globals.tie != 0), every called gene masked singly: the path is the in-place
    Bellman-Ford's, and often enough the masked path has a node with two allowed tight in-edges for that to mean something."""
    seqs = fuzz(101, 300) + fuzz(7, 300)
    ann = pa.Annotator()
    pairs = ambiguous = 0
    for b0 in range(0, 600, 100):
        st0, offs0, genes0 = run_batch(ann, seqs[b0:b0 + 100])
        tied = [i for i in range(100) if st0[i] == 0 and int(ann.globals(i).tie) != 0]
        refs = {i: Ref(ann, i) for i in tied}
        called = {i: refs[i].called(genes0[offs0[i]:offs0[i + 1]]) for i in tied}
        D = {i: ann.path(i)[1] for i in tied}
        for r in range(max([len(called[i]) for i in tied] + [0])):
            forbid = [[called[i][r]] if i in refs and r < len(called[i]) else None for i in range(100)]
            st, offs, genes, delta = ann.reannotate(forbid)
            for i in tied:
                if forbid[i] is None:
                    continue
                DF, path, _, dist, edges = check_against_ref(ann, refs[i], forbid[i], int(st[i]), genes[offs[i]:offs[i + 1]], delta[i], D[i])
                pairs += 1
                if DF is None:
                    continue
                on_path = set(path)
                tight = {}
                for u, v, w in edges:
                    if v in on_path and dist[u] is not None and dist[u] + w == dist[v]:
                        tight[v] = tight.get(v, 0) + 1
                ambiguous += any(c >= 2 for c in tight.values())
    ann.close()
    print("tie rule under a mask: %d (contig, gene) pairs, %d with a second allowed tight in-edge on the masked path" % (pairs, ambiguous))
    assert ambiguous >= 50, (pairs, ambiguous)


# ---- 4. against the drop margins of §12 ----
def check_against_drops(ann, n):
    dst, doffs, drec = ann.drop_margins()
    orfs = [ann.orfs(i) if dst[i] == 0 else None for i in range(n)]
    idx = []
    for i in range(n):
        if dst[i] != 0:
            idx.append([])
            continue
        idx.append([ann.orf_index(i, int(r["left"]), int(r["right"]), int(r["strand"])) for r in drec[doffs[i]:doffs[i + 1]]])
    checked = 0
    for r in range(max([len(x) for x in idx] + [0])):
        one = [[idx[i][r]] if r < len(idx[i]) else None for i in range(n)]
        grp = [np.nonzero(orfs[i]["group"] == orfs[i]["group"][idx[i][r]])[0] if r < len(idx[i]) else None for i in range(n)]
        s1, _, _, d1 = ann.reannotate(one)
        s2, o2, g2, d2 = ann.reannotate(grp)
        for i in range(n):
            if grp[i] is None:
                continue
            rec = drec[doffs[i] + r]
            if rec["bypass"]:
                assert s2[i] == 0 and d2[i].tobytes() == rec["drop"].tobytes(), (i, r, float(d2[i]), float(rec["drop"]))
            else:
                assert s2[i] == 1 and d2[i] == np.inf and rec["drop"] == np.inf and o2[i + 1] == o2[i], (i, r)
            assert s1[i] in (0, 1) and 0.0 <= d1[i] <= rec["drop"], (i, r, float(d1[i]), float(rec["drop"]))
            checked += 1
    return checked


def test_stop_group_masks_equal_the_drop_margins(pa):
    n = 0
    for case in golden_cases():
        g, name, seq = load_golden(case)
        if str(g["error"]) or case == "edge_huge":
            continue
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        tr = golden_trnas(g)
        run_batch(ann, [seq], None if tr is None else [tr])
        n += check_against_drops(ann, 1)
        ann.close()
    assert n >= 300
    seqs = fuzz(11, 40)
    ann = pa.Annotator()
    run_batch(ann, seqs)
    assert check_against_drops(ann, 40) >= 200
    ann.close()


# ---- 5. determinism and non-interference ----
def reann_bytes(ann, forbid, i=None):
    st, offs, genes, delta = ann.reannotate(forbid)
    if i is None:
        return st.tobytes(), offs.tobytes(), genes.tobytes(), delta.tobytes()
    return int(st[i]), genes[offs[i]:offs[i + 1]].tobytes(), delta[i].tobytes(), ann.reannotated_path(i)[0].tobytes()


def test_lone_contig_and_batch_of_300_give_the_same_bytes(pa):
    seqs = fuzz(23, 300)
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    for i in range(5, 300, 37):
        if st0[i] != 0 or offs0[i + 1] == offs0[i]:
            continue
        g = genes0[offs0[i] + (offs0[i + 1] - offs0[i]) // 2]
        if abs(int(g["frame"])) > 3:
            continue
        k = ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"]))
        forbid = [None] * 300
        forbid[i] = [k]
        got = reann_bytes(ann, forbid, i)
        lone = pa.Annotator()
        run_batch(lone, [seqs[i]])
        assert reann_bytes(lone, [[lone.orf_index(0, int(g["left"]), int(g["right"]), int(g["strand"]))]], 0) == got, i
        lone.close()
    ann.close()


def test_create_flags_give_the_same_bytes(pa):
    small = [pa.synth_contig(61, 14000), pa.synth_contig(62, 9000)]
    medium = fuzz(5, 40)

    def outs(flags):
        ann = pa.Annotator(flags=flags)
        res = []
        for seqs in (small, medium):
            st0, offs0, genes0 = run_batch(ann, seqs)
            forbid = []
            for i in range(len(seqs)):
                cds = [g for g in genes0[offs0[i]:offs0[i + 1]] if abs(int(g["frame"])) <= 3]
                forbid.append([ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds[::3]] if st0[i] == 0 and cds else None)
            res.append(reann_bytes(ann, forbid))
            res.append([ann.reannotated_path(i)[0].tobytes() for i in range(len(seqs)) if st0[i] == 0])
        ann.close()
        return res

    want = outs(())
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        assert outs((fl,)) == want, fl


def test_reannotation_disturbs_nothing_and_is_invalidated_by_the_next_batch(pa):
    a, b = fuzz(31, 30), fuzz(32, 30)

    def everything(ann):
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()],
                [x.tobytes() for x in ann.replacements()], [ann.path(i)[0].tobytes() for i in range(ann.n)], ann.certified().tobytes())

    def some_mask(ann):
        st0, offs0, genes0 = ann.download_flat(exact=False)
        out = []
        for i in range(ann.n):
            cds = [g for g in genes0[offs0[i]:offs0[i + 1]] if abs(int(g["frame"])) <= 3]
            out.append([ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds[:2]] if cds else None)
        return out

    first = pa.Annotator()  # everything else first, then the re-annotation, then everything else again
    first.upload(a)
    first.run()
    before = everything(first)
    r1 = reann_bytes(first, some_mask(first))
    assert everything(first) == before
    other = pa.Annotator()  # the re-annotation first
    other.upload(a)
    other.run()
    assert reann_bytes(other, some_mask(other)) == r1
    assert everything(other) == before
    assert reann_bytes(other, some_mask(other)) == r1
    other.close()
    # the next upload or run invalidates it
    first.reannotated_path(0)
    first.upload(b)
    with pytest.raises(pa.PhxError) as e:
        first.reannotated_path(0)
    assert e.value.code == -13
    with pytest.raises(pa.PhxError) as e:
        first.reannotate([None] * 30)
    assert e.value.code == -13
    first.run()
    with pytest.raises(pa.PhxError) as e:
        first.reannotated_path(0)
    assert e.value.code == -13
    fresh = pa.Annotator()
    fresh.upload(b)
    fresh.run()
    assert reann_bytes(first, some_mask(first)) == reann_bytes(fresh, some_mask(fresh))
    assert everything(first) == everything(fresh)
    for x in (first, fresh):
        x.close()


# ---- 6. statuses ----
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
    for solve_all in (False, True):
        forbid = [None] * 6
        for i in (4, 5):
            g = genes0[offs0[i]]
            forbid[i] = [ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"]))]
        st, offs, genes, delta = ann.reannotate(forbid, solve_all=solve_all)
        assert st.tolist() == [-2, -3, 1, -7, 0, 0]
        assert np.diff(offs).tolist()[:4] == [0] * 4 and (delta[:4] == np.inf).all() and (delta[4:] >= 0).all() and np.isfinite(delta[4:]).all()
        for k, i in enumerate((4, 5)):
            lone = pa.Annotator()
            l0 = run_batch(lone, [good[k]])
            assert reann_bytes(lone, [forbid[i]], 0) == reann_bytes(ann, forbid, i)
            lone.close()
    # offsets that are not the batch's: refused before any kernel runs
    import ctypes as C

    oo = ann.orf_offsets().copy()
    mask = np.zeros(int(oo[-1]) + 8, np.uint8)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    offs, st, delta, total = np.zeros(7, np.int64), np.zeros(6, np.int32), np.zeros(6), C.c_int64()
    assert ann.L.phx_reannotate_flat(ann.h, vp(mask), vp(oo), 0, None, 0, vp(offs), vp(st), vp(delta), C.byref(total)) == 0
    for wrong in (oo + 1, np.concatenate([oo[:-1], [oo[-1] + 1]]), np.concatenate([oo[:4], [oo[4] + 1], oo[5:]])):
        wrong = np.ascontiguousarray(wrong, np.int64)
        assert ann.L.phx_reannotate_flat(ann.h, vp(mask), vp(wrong), 0, None, 0, vp(offs), vp(st), vp(delta), C.byref(total)) == -1
    ann.close()


def test_a_mask_that_leaves_no_path(pa):
    """Every ORF refused: connectors alone reach the target only where bridges do; else PHX_S_NOPATH with +inf and no genes."""
    seqs = [pa.synth_contig(410, 6000), pa.synth_contig(411, 8000)]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    n0 = len(ann.orfs(0))
    st, offs, genes, delta = ann.reannotate([np.arange(n0), None])
    ref = Ref(ann, 0)
    check_against_ref(ann, ref, list(range(n0)), int(st[0]), genes[offs[0]:offs[1]], delta[0], ann.path(0)[1])
    assert st[1] == 0 and delta[1] == 0.0 and genes[offs[1]:offs[2]].tobytes() == genes0[offs0[1]:offs0[2]].tobytes()
    # a contig the run itself finds no path on keeps PHX_S_NOPATH
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    lone = pa.Annotator()
    run_batch(lone, [dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops])
    st, offs, genes, delta = lone.reannotate([None], solve_all=True)
    assert st.tolist() == [1] and delta[0] == np.inf and len(genes) == 0
    lone.close()
    ann.close()


def test_a_stop_group_without_bypass_leaves_no_path(pa):
    """Drop records with bypass = 0 name genes no path can avoid: refusing the gene's whole stop group must give PHX_S_NOPATH, +inf, no
    genes and an empty path, and leave the neighbours as the run left them."""
    seqs = fuzz(11, 60)
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    dst, doffs, drec = ann.drop_margins()
    seen = 0
    for i in range(60):
        if dst[i] != 0:
            continue
        for r in drec[doffs[i]:doffs[i + 1]]:
            if r["bypass"]:
                continue
            orfs = ann.orfs(i)
            k = ann.orf_index(i, int(r["left"]), int(r["right"]), int(r["strand"]))
            forbid = [None] * 60
            forbid[i] = np.nonzero(orfs["group"] == orfs["group"][k])[0]
            st, offs, genes, delta = ann.reannotate(forbid)
            assert st[i] == 1 and delta[i] == np.inf and offs[i + 1] == offs[i], (i, k)
            assert len(ann.reannotated_path(i)[0]) == 0
            assert np.delete(st, i).tolist() == np.delete(st0, i).tolist() and len(genes) == len(genes0) - (offs0[i + 1] - offs0[i])
            seen += 1
            break
    ann.close()
    assert seen >= 1, "no gene without a bypass among these contigs: the test no longer exercises the no-path result"


def test_before_a_run_is_a_state_error(pa):
    ann = pa.Annotator()
    ann.upload([pa.synth_contig(5, 5000)])
    with pytest.raises(pa.PhxError) as e:
        ann.reannotate([None])
    assert e.value.code == -13
    ann.close()


# ---- 7. the CLI ----
def test_cli_forbid_and_reannotation(pa, tmp_path):
    from phanotate_amd.cli import format_reannotation

    g, name, phix = load_golden("phiX174") if "phiX174" in golden_cases() else (None, None, None)
    inputs = {"two": {"c1": pa.synth_contig(71, 20000).decode(), "c2": pa.synth_contig(72, 9000).decode()}}
    if phix is not None:
        inputs["phix"] = {name: phix}
    for tag, seqs in inputs.items():
        fasta = tmp_path / (tag + ".fasta")
        fasta.write_text("".join(">%s\n%s\n" % (k, v) for k, v in seqs.items()))
        plain = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)], capture_output=True, timeout=600)
        assert plain.returncode == 0
        rows = [ln for ln in plain.stdout.decode().splitlines() if ln and not ln.startswith("#")]
        picked = [rows[1], rows[-2]]
        fb = tmp_path / (tag + ".forbid")
        fb.write_text("# refused calls\n" + picked[0] + "\n" + "\t".join(picked[1].split("\t")[:4]) + "\n")
        out = tmp_path / (tag + ".reann")
        run = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta), "--forbid", str(fb), "--reannotation", str(out)], capture_output=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        assert run.stdout == plain.stdout
        ann = pa.Annotator()
        ann.upload(list(seqs.values()))
        ann.set_trnas(None)
        ann.run()
        names = list(seqs)
        forbid = [None] * len(names)
        for ln in picked:
            a, z, fr, ctg = ln.split("\t")[:4]
            i = names.index(ctg)
            forbid[i] = (forbid[i] or []) + [ann.orf_index(i, min(int(a), int(z)), max(int(a), int(z)), 1 if fr == "+" else -1)]
        st, offs, genes, delta = ann.reannotate(forbid)
        text = out.read_text()
        assert text == format_reannotation(names, st, offs, genes, delta)
        assert text.count("#delta:\t") == len(names) and all(("\t".join(ln.split("\t")[:4]) + "\t") not in text for ln in picked)
        ann.close()
        # a line that names no ORF of its contig ends the program with an error that quotes it
        bogus = "17\t23\t+\t%s" % names[0]
        fb.write_text(bogus + "\n")
        err = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta), "--forbid", str(fb), "--reannotation", str(out)], capture_output=True, timeout=600)
        assert err.returncode != 0 and repr(bogus) in err.stderr.decode()
    for bad in (["--forbid", str(fb)], ["--reannotation", str(out)], ["--forbid", str(fb), "--reannotation", str(out), "-d"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)] + bad, capture_output=True, timeout=600)
        assert r.returncode == 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta), "--forbid", str(fb), "--reannotation", str(out)], capture_output=True, timeout=600,
                       env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and b"multi-rank" in r.stderr


def test_cli_forbid_together_with_the_sibling_outputs(pa, tmp_path):
    """--forbid / --reannotation with --margins, --drop-margins and --drop-replacements, in one batch and in several: every file is
    written and equals what the flag gives on its own."""
    seqs = {"c1": pa.synth_contig(71, 20000).decode(), "c2": pa.synth_contig(72, 9000).decode(), "c3": pa.synth_contig(73, 12000).decode()}
    fasta = tmp_path / "three.fasta"
    fasta.write_text("".join(">%s\n%s\n" % (k, v) for k, v in seqs.items()))
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    sib = lambda tag: ["--margins", str(tmp_path / (tag + ".m")), "--drop-margins", str(tmp_path / (tag + ".d")), "--drop-replacements", str(tmp_path / (tag + ".r"))]
    plain = subprocess.run(exe + sib("plain"), capture_output=True, timeout=600)
    assert plain.returncode == 0, plain.stderr[-2000:]
    rows = [ln for ln in plain.stdout.decode().splitlines() if ln and not ln.startswith("#")]
    fb = tmp_path / "f.txt"
    fb.write_text(rows[2] + "\n" + rows[-3] + "\n")
    alone = subprocess.run(exe + ["--forbid", str(fb), "--reannotation", str(tmp_path / "alone.q")], capture_output=True, timeout=600)
    assert alone.returncode == 0, alone.stderr[-2000:]
    for tag, extra in (("one", []), ("many", ["--batch-bases", "21000"])):
        r = subprocess.run(exe + sib(tag) + ["--forbid", str(fb), "--reannotation", str(tmp_path / (tag + ".q"))] + extra, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == plain.stdout
        for ext in ("m", "d", "r"):
            assert (tmp_path / (tag + "." + ext)).read_bytes() == (tmp_path / ("plain." + ext)).read_bytes(), (tag, ext)
        assert (tmp_path / (tag + ".q")).read_bytes() == (tmp_path / "alone.q").read_bytes(), tag
    r = subprocess.run(exe + ["--forbid", str(fb), "--reannotation", str(tmp_path / "g.q"), "--gpus", "2"], capture_output=True, timeout=600)
    assert r.returncode == 2 and b"--gpus above 1" in r.stderr
