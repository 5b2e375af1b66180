"""Evidence scenario batches on the device (phx_evidence_scenarios_flat).  Every scenario is compared with its definition —
Annotator.evidence(..., solve_all=True) of its contig with exactly that bias and that refused set, byte for byte — or with the yardstick of
tests/test_evidence_gpu.py (python integers under conftest.inorder_bellman_ford), never with the code under test."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, inorder_bellman_ford, load_golden
from test_evidence_gpu import B_MAX, EvRef, called_orfs, score, solved_contigs
from test_reannotate_gpu import fuzz, run_batch, wide_cases
from test_scenarios_gpu import case1_seqs, result_digest, scenario_triples

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def small_seqs(pa):
    return case1_seqs(pa) + fuzz(11, 6)


def as_scen(i, bias, F=None):
    """(contig, bias, forbid) as Annotator.evidence_scenarios takes it; bias: None or (ORF index, integer B) pairs, duplicates kept."""
    return (i, None if bias is None else [(k, score(B)) for k, B in bias], F)


def sibling(ann, scen_item):
    """(status, delta bytes, gene bytes) of the scenario's contig from evidence() with that bias and that refused set on that contig alone."""
    i, bias, F = scen_item
    b, f = [None] * ann.n, [None] * ann.n
    b[i] = bias
    f[i] = None if F is None or len(F) == 0 else np.asarray(F)
    st, offs, genes, delta = ann.evidence(b, f, solve_all=True)
    return int(st[i]), delta[i].tobytes(), genes[offs[i]:offs[i + 1]].tobytes()


def merged(bias, F):
    """{ORF: summed B} without zero sums and without the ORFs of F: what the scenario's bias is by definition."""
    out = {}
    for k, B in bias or []:
        out[k] = out.get(k, 0) + B
    return {k: B for k, B in out.items() if B != 0 and k not in set(F or [])}


def rich(ann, dl, refs, m):
    """The first m solved contigs with at least four called CDS genes (a fuzz contig may call one)."""
    st0, offs0, genes0 = dl
    out = [i for i in sorted(refs) if len(called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])) >= 4][:m]
    assert len(out) == m
    return out


def small_scenarios(ann, dl, refs):
    """About 40 scenarios over the small batch, as (contig, (ORF, integer B) pairs or None, refused list or None): empty, refused only, biased
    only, both, duplicate pairs, an ORF both refused and biased, an ORF without an edge, mixed signs, and one contig named ten times."""
    st0, offs0, genes0 = dl
    rng = np.random.RandomState(2011)
    scen = []
    for i in rich(ann, dl, refs, 5):
        cg = called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])
        n_orf = len(ann.orfs(i))
        uncalled = sorted(set(range(n_orf)) - set(cg))
        u = [uncalled[int(x)] for x in rng.choice(len(uncalled), 4, replace=False)]
        scen.append((i, None, None))                                                   # empty
        scen.append((i, None, [cg[1]]))                                                # refused only
        scen.append((i, [(u[0], -int(rng.randint(20000, 200000)))], None))                # biased only: a bonus on an uncalled ORF
        scen.append((i, [(cg[0], 4000), (u[1], -2500)], [cg[2]]))                      # both
        scen.append((i, [(u[2], -1000), (cg[-1], 700), (u[2], -500), (u[2], 200), (cg[-1], -700)], None))  # duplicates: sums -1300 and 0
        scen.append((i, [(cg[1], -5000), (u[3], -800)], [cg[1], cg[1]]))               # refused and biased: the refusal wins
        scen.append((i, [(int(k), int(rng.choice([-1, 1]) * 10 ** rng.uniform(1, 4.5))) for k in rng.choice(n_orf, 6, replace=False)], None))  # mixed signs
    # an ORF without an edge: ignored.  The graph stage gives every ORF a row of its own (k_edges_orf), so the inputs may hold none:
    # case 1 then asserts exactly that, per contig, instead of passing over the kind in silence
    noedge = [(i, k) for i in sorted(refs) for k, e in enumerate(refs[i].orf_edge) if e is None]
    for i, k in noedge[:2]:
        scen.append((i, [(k, -9000)], None))
    i = sorted(refs)[1]
    cg = called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])
    for r in range(10):                                                                # one contig ten times in a row
        scen.append((i, [(cg[r % len(cg)], 1500 + 100 * r)] if r != 4 else None, [cg[(r + 1) % len(cg)]] if r % 3 == 0 else None))
    return scen, len(noedge)


def run_small(pa):
    ann = pa.Annotator()
    dl = run_batch(ann, small_seqs(pa))
    refs = {i: EvRef(ann, i) for i in solved_contigs(ann, dl[0])}
    scen, n_noedge = small_scenarios(ann, dl, refs)
    res = ann.evidence_scenarios([as_scen(*s) for s in scen])
    return ann, dl, refs, scen, res, n_noedge


@pytest.fixture(scope="module")
def small(pa):
    ann, dl, refs, scen, res, n_noedge = run_small(pa)
    chunks = ann.scenario_chunks()
    ms = ann.scenarios_ms()
    yield ann, dl, refs, scen, res, chunks, ms, n_noedge
    ann.close()


def child_main():
    """Case 7's child process: the scenarios of case 1 under the PHX_SCEN_BYTES of the environment; prints the chunk count and a digest."""
    import phanotate_amd as pa

    ann, dl, refs, scen, res, n_noedge = run_small(pa)
    print("SCEN %d %d %s" % (len(scen), ann.scenario_chunks(), result_digest(res)))
    ann.close()


# ---- 1. the definition, byte for byte ----
def test_every_scenario_equals_evidence_with_its_bias_and_mask_alone(small):
    ann, dl, refs, scen, res, chunks, ms, n_noedge = small
    st0, offs0, genes0 = dl
    assert 35 <= len(scen) <= 50 and chunks == 1
    assert set(ms) == {"mask", "solve", "finish"} and ms["solve"] > 0
    st, offs, genes, delta = res
    assert offs[0] == 0 and offs[-1] == len(genes) and (np.diff(offs) >= 0).all()
    got = scenario_triples(res)
    paths = {j: ann.scenario_path(j, scen[j][0]) for j in range(len(scen))}  # (before the sibling calls: nothing of theirs may change them, case 8 checks that)
    kinds, want_st = set(), []
    for j, s in enumerate(scen):
        sib = sibling(ann, as_scen(*s))
        assert got[j] == sib, (j, s)
        want_st.append(sib[0])
        i, bias, F = s
        m = merged(bias, F)
        kinds.add((bool(m), bool(F)))
        if not m and not F:  # the device path of a plain slot: the run's result
            assert got[j] == (int(st0[i]), np.float64(0.0).tobytes(), genes0[offs0[i]:offs0[i + 1]].tobytes()), j
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    assert any(delta[j] < 0 for j in range(len(scen))) and any(0 < delta[j] < np.inf for j in range(len(scen)))
    print("scenarios: %d, ORFs without an edge in the small batch: %d" % (len(scen), n_noedge))
    if n_noedge:  # its scenario has a biased slot (a merged bias) whose list stays empty: the run's result, byte for byte
        j = next(j for j, (i, bias, F) in enumerate(scen) if bias and len(bias) == 1 and refs[i].orf_edge[bias[0][0]] is None)
        i = scen[j][0]
        assert merged(scen[j][1], scen[j][2]) and got[j] == (int(st0[i]), np.float64(0.0).tobytes(), genes0[offs0[i]:offs0[i + 1]].tobytes()), j
    else:  # no such ORF exists on these inputs: every ORF of every contig has its own edge in the tapped graph
        for i, ref in refs.items():
            edges = {(u, v) for u, v, _ in ref.edges}
            assert len({e for e in ref.orf_edge}) == len(ref.orfs) and all(e in edges for e in ref.orf_edge), i
    # D_B and the path against the in-place Bellman-Ford on the biased python integers
    seen = 0
    for j, (i, bias, F) in enumerate(scen):
        m = merged(bias, F)
        if not m or seen >= 14 or want_st[j] == -9:  # (evidence() says a cycle is negative there: the python loop would take its V + 1 rounds)
            continue
        ref = refs[i]
        gone = {ref.orf_edge[k] for k in F or []} - {None}
        add = {ref.orf_edge[k]: B for k, B in m.items() if ref.orf_edge[k] is not None}
        edges = [(u, v, w + add.get((u, v), 0)) for u, v, w in ref.edges if (u, v) not in gone]
        dist, par = inorder_bellman_ford(ref.V, edges, ref.V - 2)
        got_path, got_D = paths[j]
        assert dist is not None, j
        if dist[ref.V - 1] is None:
            assert st[j] == 1 and delta[j] == np.inf and len(got_path) == 0, j
        else:
            D = ann.path(i)[1]
            assert st[j] == 0 and got_D == dist[ref.V - 1], (j, got_D, dist[ref.V - 1])
            assert float(delta[j]) == float(got_D - D) / 1000.0, j
            want, v = [ref.V - 1], ref.V - 1
            while v != ref.V - 2:
                v = edges[par[v]][0]
                want.append(v)
            assert got_path.tolist() == want[::-1], j
            seen += 1
    assert seen >= 10, seen


# ---- 2. list sizes where the sparse path can go wrong ----
def test_list_sizes_and_the_ends_of_the_in_edge_slots(small):
    ann, dl, refs, scen0, res0, chunks, ms, n_noedge = small
    st0, offs0, genes0 = dl
    i = max(refs, key=lambda i: len(refs[i].orfs))  # the 20 kb contig
    ref = refs[i]
    have = [k for k, e in enumerate(ref.orf_edge) if e is not None]
    assert len(have) >= 70, len(have)
    rng = np.random.RandomState(2012)
    scen = []
    for k in (1, 2, 3, 33, 64, 65):
        ks = rng.choice(have, k, replace=False)
        scen.append((i, [(int(x), int(rng.choice([-1, 1]) * rng.randint(1, 3000))) for x in ks], None))
    scen.append((i, [(k, 3) for k in range(len(ref.orfs))], None))  # a small penalty on every ORF of the contig
    scen.append((i, [(k, 3) for k in reversed(range(len(ref.orfs)))], [have[5]]))  # ... listed backwards, one of them refused
    # the tapped edges come in the order of the in-edge slots: the first and the last of them that is an ORF's edge
    ed = ann.edges(i)
    of_edge = {e: k for k, e in enumerate(ref.orf_edge) if e is not None}
    slots = [of_edge[(int(u), int(v))] for u, v in zip(ed["src"], ed["dst"]) if (int(u), int(v)) in of_edge]
    assert len(slots) == len(of_edge)
    scen.append((i, [(slots[0], -2000)], None))
    scen.append((i, [(slots[-1], -2000)], None))
    scen.append((i, [(slots[0], 900), (slots[-1], -900), (slots[len(slots) // 2], -1200)], None))
    res = ann.evidence_scenarios([as_scen(*s) for s in scen])
    got = scenario_triples(res)
    for j, s in enumerate(scen):
        assert got[j] == sibling(ann, as_scen(*s)), (j, len(s[1]))
    assert len({g[1] for g in got}) >= 3  # the biases move D


# ---- 3. no bias: the plain slot of scenarios() ----
def test_zero_sums_are_scenarios_byte_for_byte(small):
    ann, dl, refs, scen0, res0, chunks, ms, n_noedge = small
    st0, offs0, genes0 = dl
    plain, zero = [], []
    for i in rich(ann, dl, refs, 4):
        cg = called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])
        for F in (None, [cg[0]], [cg[1], cg[2]]):
            plain.append((i, F))
            zero.append((i, [(cg[0], 1.0), (cg[-1], -2.5), (cg[0], -1.0), (cg[-1], 2.5)], F))
            plain.append((i, F))
            zero.append((i, [(cg[1], 0.0009), (cg[2], -0.0004)] if F else None, F))  # less than a unit is no bias
    want = [np.ascontiguousarray(x).tobytes() for x in ann.scenarios(plain)]
    ann.evidence_scenarios([as_scen(sorted(refs)[0], [(1, -700)])])  # (another solve in between: the next one is no cached result)
    got = [np.ascontiguousarray(x).tobytes() for x in ann.evidence_scenarios(zero)]
    assert got == want
    assert [np.ascontiguousarray(x).tobytes() for x in ann.scenarios(plain)] == want


# ---- 4. the wide classes ----
@pytest.mark.parametrize("case", range(4))
def test_a_biased_scenario_in_the_wide_classes(pa, case):
    seqs, nl = wide_cases(pa)[case]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    want = (4, 8, 8, 17)[case]  # 256, 512, 512 and 1088 bits
    i = next(i for i in range(len(seqs)) if st0[i] == 0 and int(ann.globals(i).n_limbs) == want)
    cg = called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])
    rng = np.random.RandomState(2014 + case)
    uncalled = sorted(set(range(len(ann.orfs(i)))) - set(cg))
    bias = [(cg[0], 6000), (cg[len(cg) // 2], 12345)] + [(uncalled[int(x)], -int(rng.randint(1000, 20000))) for x in rng.choice(len(uncalled), 3, replace=False)]
    scen = [as_scen(i, bias), as_scen(i, bias[:1], [cg[-1]]), as_scen(i, None)]
    got = scenario_triples(ann.evidence_scenarios(scen))
    for j, s in enumerate(scen):
        assert got[j] == sibling(ann, s), (case, j)
    assert got[0][0] == 0 and got[0][1] != np.float64(0.0).tobytes() and got[2][1] == np.float64(0.0).tobytes()  # the penalties move D
    ann.close()


# ---- 5. a negative cycle beside a clean scenario of the same contig ----
def test_a_negative_cycle_sits_beside_a_clean_scenario(small):
    ann, dl, refs, scen0, res0, chunks, ms, n_noedge = small
    rng = np.random.RandomState(2015)
    draw = []
    for i in sorted(refs):
        have = [k for k, e in enumerate(refs[i].orf_edge) if e is not None]
        draw += [(i, int(k), -int(10 ** rng.uniform(4, 9))) for k in rng.choice(have, min(12, len(have)), replace=False)]
    # (the drawing alone goes through the batch; what it finds is then held against evidence())
    st = ann.evidence_scenarios([as_scen(i, [(k, B)]) for i, k, B in draw])[0]
    hit = [d for d, s in zip(draw, st) if s == -9]
    if not hit:
        pytest.skip("no drawn bonus makes a cycle negative on the small inputs")
    i, k, B = hit[0]
    clean = as_scen(i, [(k, 2000)])
    scen = [clean, as_scen(i, [(k, B)]), clean, as_scen(i, None)]
    res = ann.evidence_scenarios(scen)
    got = scenario_triples(res)
    assert got[1] == (-9, np.float64(np.inf).tobytes(), b"") and len(ann.scenario_path(1, i)[0]) == 0
    for j, s in enumerate(scen):
        assert got[j] == sibling(ann, s), j
    assert got[0] == got[2] and got[0][0] == 0 and got[3][0] == 0
    print("negative cycles among %d drawn bonuses: %d" % (len(draw), len(hit)))


# ---- 6. margin titration through the batch ----
def test_margin_titration_in_one_call(small):
    """§19's titration, every point a scenario of one call: for uncalled ORFs with a finite path margin Delta, B = -Delta + 1 leaves D
    alone, -Delta ties (the in-order rule picks the path: nothing is said about `called`), -Delta - 1 wins by one unit."""
    ann, dl, refs, scen0, res0, chunks, ms, n_noedge = small
    mst, moffs, mrec = ann.margins()
    rng = np.random.RandomState(2016)
    picks = []
    for i in sorted(refs):
        rec = mrec[moffs[i]:moffs[i + 1]]
        ok = [k for k in range(len(rec)) if rec["through"][k] == 1 and rec["called"][k] == 0 and np.isfinite(rec["margin"][k]) and round(float(rec["margin"][k]) * 1000) < 1 << 50]
        picks += [(i, int(k), int(round(float(rec["margin"][k]) * 1000))) for k in sorted(rng.choice(ok, min(len(ok), 10), replace=False).tolist())]
    assert len(picks) >= 40
    scen = [as_scen(i, [(k, -Delta + step)]) for i, k, Delta in picks for step in (1, 0, -1)]
    st, offs, genes, delta = ann.evidence_scenarios(scen)
    clean = left_out = 0
    for x, (i, k, Delta) in enumerate(picks):
        if (st[3 * x:3 * x + 3] == -9).any():  # the bonus makes a cycle through k negative: no point of this ORF counts
            left_out += 1
            continue
        assert (st[3 * x:3 * x + 3] == 0).all(), (i, k, Delta)
        assert [float(d) for d in delta[3 * x:3 * x + 3]] == [0.0, 0.0, -0.001], (i, k, Delta, delta[3 * x:3 * x + 3])
        called = [k in called_orfs(ann, i, genes[offs[3 * x + s]:offs[3 * x + s + 1]]) for s in range(3)]
        assert not called[0] and called[2], (i, k, Delta, called)
        clean += 1
    print("titration: %d ORFs, %d left out (negative cycle), %d clean at all three points" % (len(picks), left_out, clean))
    assert clean >= 20, (len(picks), left_out, clean)


# ---- 7. chunking does not matter ----
def test_three_or_more_chunks_give_the_same_bytes(small):
    ann, dl, refs, scen, res, chunks, ms, n_noedge = small
    code = "import sys; sys.path.insert(0, %r); import test_evidence_scenarios_gpu as t; t.child_main()" % HERE
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=600, env=dict(os.environ, PHX_SCEN_BYTES="300000"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("SCEN ")][-1].split()
    assert int(line[1]) == len(scen)
    assert int(line[2]) >= 3, line
    assert line[3] == result_digest(res)


# ---- 8. isolation, cache, state; 9. argument errors ----
def raw_call(ann, contig, foff, forf, boff, borf, bval, oo=None):
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    contig, foff, forf = np.ascontiguousarray(contig, np.int32), np.ascontiguousarray(foff, np.int64), np.ascontiguousarray(forf, np.int32)
    boff, borf, bval = np.ascontiguousarray(boff, np.int64), np.ascontiguousarray(borf, np.int32), np.ascontiguousarray(bval, np.int64)
    oo = np.ascontiguousarray(ann.orf_offsets() if oo is None else oo, np.int64)
    S = len(contig)
    offs, st, delta, total = np.zeros(S + 1, np.int64), np.zeros(S + 1, np.int32), np.zeros(S + 1), C.c_int64()
    return ann.L.phx_evidence_scenarios_flat(ann.h, S, vp(contig), vp(foff), vp(forf), vp(boff), vp(borf), vp(bval), vp(oo), 0, None, 0, vp(offs), vp(st), vp(delta), C.byref(total))


def test_evidence_scenarios_disturb_nothing_are_cached_and_state_and_argument_errors(pa):
    ann = pa.Annotator()
    ann.upload([pa.synth_contig(5, 5000)])
    with pytest.raises(pa.PhxError) as e:  # before a run
        ann.evidence_scenarios([(0, None, None)])
    assert e.value.code == -13
    assert raw_call(ann, [0], [0, 0], [0], [0, 0], [0], [0], oo=[0, 0]) == -13
    seqs = fuzz(31, 12)
    st0, offs0, genes0 = run_batch(ann, seqs)
    cgs = [called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]]) if st0[i] == 0 else [] for i in range(ann.n)]
    ev_bias = [[(cg[0], 2.5), (cg[-1], -1.0)] if cg else None for cg in cgs]

    def everything():
        ev = ann.evidence(ev_bias)
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ev], ann.reannotate_ms(),
                [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n)])

    before = everything()
    spec = [(i, [(cg[0], 3000), (cg[1], -800)], [cg[2]]) for i, cg in enumerate(cgs) if len(cg) >= 3] + [(i, None, None) for i in range(ann.n)]
    scen = [as_scen(*s) for s in spec]
    res = ann.evidence_scenarios(scen)
    assert [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n)] == before[4]  # evidence()'s cached result stands: no solve of its own ran since
    assert everything() == before
    ms = ann.scenarios_ms()
    assert ms["solve"] > 0
    assert result_digest(ann.evidence_scenarios(scen)) == result_digest(res) and ann.scenarios_ms() == ms  # the second identical call reuses the solve
    # the cache is keyed on the merged bias lists: a different bias is a different solve, the same sums in other pairs are not
    other = [as_scen(i, [(k, B + 500) for k, B in bias] if bias else bias, F) for i, bias, F in spec]
    assert result_digest(ann.evidence_scenarios(other)) != result_digest(res)
    split = [as_scen(i, [(k, B // 2) for k, B in bias] + [(k, B - B // 2) for k, B in reversed(bias)] if bias else bias, F) for i, bias, F in spec]
    assert result_digest(ann.evidence_scenarios(split)) == result_digest(res)
    # ---- argument errors, all before any kernel ----
    oo = ann.orf_offsets()
    n0 = int(oo[1] - oo[0])
    assert raw_call(ann, [0], [0, 0], [0], [0, 2], [1, 1], [B_MAX + 7, -7]) == 0                # the sum counts, not the parts
    assert raw_call(ann, [0, 1], [0, 1, 1], [0], [0, 1, 3], [1, 0, 0], [-500, 40, -40]) == 0
    ms_ok = ann.scenarios_ms()
    assert raw_call(ann, [0], [0, 0], [0], [0, 2], [1, 1], [(1 << 51) + 1, 1 << 51]) == -1      # |B| > 2^52 after merging
    assert raw_call(ann, [0], [0, 0], [0], [0, 2], [1, 1], [-(1 << 52), -1]) == -1
    assert raw_call(ann, [0], [0, 0], [0], [0, 1], [1], [B_MAX + 1]) == -1
    assert raw_call(ann, [ann.n], [0, 0], [0], [0, 0], [0], [0]) == -1 and raw_call(ann, [-1], [0, 0], [0], [0, 0], [0], [0]) == -1  # a contig outside the batch
    assert raw_call(ann, [0], [0, 0], [0], [0, 1], [n0], [5]) == -1 and raw_call(ann, [0], [0, 0], [0], [0, 1], [-1], [5]) == -1    # a biased ORF outside its contig
    assert raw_call(ann, [0], [0, 1], [n0], [0, 1], [0], [5]) == -1                                                              # a refused one
    assert raw_call(ann, [0, 1], [0, 1, 1], [0], [0, 2, 1], [1, 0, 0], [-500, 40, -40]) == -1  # bias offsets that decrease, everything else valid
    assert raw_call(ann, [0, 1], [0, 1, 1], [0], [1, 1, 3], [1, 0, 0], [-500, 40, -40]) == -1  # ... or do not start at 0
    assert raw_call(ann, [0, 1], [0, 1, 0], [0], [0, 1, 3], [1, 0, 0], [-500, 40, -40]) == -1  # refused offsets that decrease
    assert raw_call(ann, [0], [0, 0], [0], [0, 0], [0], [0], oo=oo + 1) == -1
    assert ann.scenarios_ms() == ms_ok and ann.scenario_chunks() == 1  # no kernel ran for a refused call: the times are the last good solve's
    with pytest.raises(ValueError):
        ann.evidence_scenarios([(0, [(1, 2.0 ** 52 / 1000.0 * 0.75), (1, 2.0 ** 52 / 1000.0 * 0.75)], None)])
    for b in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ann.evidence_scenarios([(0, [(1, b)], None)])
    for bad in ([(0, [(n0, 1.0)], None)], [(0, None, [n0])], [(ann.n, None, None)], [(0, {-1: 1.0}, None)]):
        with pytest.raises(IndexError):
            ann.evidence_scenarios(bad)
    with pytest.raises(ValueError):
        ann.evidence_scenarios([(0, None)])
    assert result_digest(ann.evidence_scenarios(scen)) == result_digest(res) and everything() == before  # the refused calls left nothing behind
    # ---- the next upload invalidates the result ----
    ann.scenario_path(0, scen[0][0])
    ann.upload(seqs[:3])
    with pytest.raises(pa.PhxError) as e:
        ann.scenario_path(0, 0)
    assert e.value.code == -13
    assert raw_call(ann, [0], [0, 0], [0], [0, 0], [0], [0], oo=oo[:4]) == -13
    ann.run()
    fresh = pa.Annotator()
    run_batch(fresh, seqs[:3])
    few = [s for s in scen if s[0] < 3]
    assert result_digest(ann.evidence_scenarios(few)) == result_digest(fresh.evidence_scenarios(few))
    fresh.close()
    ann.close()


# ---- 10. evidence_scan() and the CLI ----
def scan_expectation(ann, i, k, b, run_genes):
    """One record of evidence_scan() from a single evidence() call and the run's device genes."""
    bias = [None] * ann.n
    bias[i] = [(k, b)]
    st, offs, genes, delta = ann.evidence(bias, solve_all=True)
    key = lambda g: (int(g["left"]), int(g["right"]), int(g["strand"]), int(g["frame"]))
    have, new = {key(g) for g in run_genes}, {key(g) for g in genes[offs[i]:offs[i + 1]]}
    o = ann.orfs(i)[k]
    fwd = o["frame"] > 0
    left, right = (int(o["start"]), int(o["stop"]) + 2) if fwd else (int(o["stop"]), int(o["start"]) + 2)
    return dict(left=left, right=right, strand=1 if fwd else -1, orf=k, bias=b, status=int(st[i]), delta=float(delta[i]),
                was_called=int(k in called_orfs(ann, i, run_genes)), called=int(k in called_orfs(ann, i, genes[offs[i]:offs[i + 1]])),
                n_removed=len(have - new), n_added=len(new - have)), genes[offs[i]:offs[i + 1]].tobytes()


def test_evidence_scan_records_equal_single_evidence_calls(small):
    ann, dl, refs, scen0, res0, chunks, ms, n_noedge = small
    st0, offs0, genes0 = dl
    rng = np.random.RandomState(2017)
    hits = [None] * ann.n
    for i in rich(ann, dl, refs, 4):
        cg = called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])
        uncalled = sorted(set(range(len(ann.orfs(i)))) - set(cg))
        hits[i] = [(cg[0], 3.5), (uncalled[int(rng.randint(len(uncalled)))], -25.0), (cg[1], -0.0004), (uncalled[int(rng.randint(len(uncalled)))], -400.0)]
    st, offs, rec, soffs, genes = ann.evidence_scan(hits)
    assert st.tolist() == st0.tolist() and offs.tolist() == np.concatenate([[0], np.cumsum([len(h or []) for h in hits])]).tolist()
    assert len(rec) == offs[-1] and len(soffs) == len(rec) + 1
    x = 0
    for i, h in enumerate(hits):
        for k, b in h or []:
            want, gbytes = scan_expectation(ann, i, k, b, genes0[offs0[i]:offs0[i + 1]])
            got = {name: (float(rec[x][name]) if name in ("bias", "delta") else int(rec[x][name])) for name in rec.dtype.names}
            assert got == want, (i, k, b)
            assert genes[soffs[x]:soffs[x + 1]].tobytes() == gbytes
            x += 1
    assert rec["was_called"].sum() >= 4 and (rec["called"] != rec["was_called"]).any() and (rec["n_added"] > 0).any()


def test_cli_evidence_scan(pa, tmp_path):
    from phanotate_amd.cli import format_evidence_scan

    g, name, phix = load_golden("phiX174")
    fasta = tmp_path / "phix.fasta"
    fasta.write_text(">%s\n%s\n" % (name, phix))
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, [phix])
    orfs = ann.orfs(0)
    cds = [x for x in genes0 if abs(int(x["frame"])) <= 3]
    rows = []
    for k in [int(x) for x in np.random.RandomState(2018).choice(len(orfs), 5, replace=False)] + called_orfs(ann, 0, cds[:2]):
        o = orfs[k]
        a, z = (int(o["start"]), int(o["stop"]) + 2) if o["frame"] > 0 else (int(o["start"]) + 2, int(o["stop"]))
        rows.append((k, "%d\t%d\t%s\t%s" % (a, z, "+" if o["frame"] > 0 else "-", name)))
    vals = [-30.0, -2.5, 1.25, -8.0, -600.0, 4.0, 0.75]
    ev = tmp_path / "ev.txt"
    ev.write_text("# hits\n" + "".join("%s\t%r\n" % (ln, b) for (k, ln), b in zip(rows, vals)) + "%s\t-1.5\tagain\n" % rows[0][1])  # an ORF named twice: two rows, each alone
    out = tmp_path / "scan.txt"
    run = subprocess.run(exe + ["--evidence-scan", str(ev), str(out)], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    st, offs, rec, soffs, genes = ann.evidence_scan([[(k, b) for (k, ln), b in zip(rows, vals)] + [(rows[0][0], -1.5)]])
    text = out.read_text()
    assert text == format_evidence_scan([name], st, offs, rec)
    body = [ln.split("\t") for ln in text.splitlines() if not ln.startswith("#")]
    assert len(body) == 8 and [r[:3] for r in body[:7]] == [ln.split("\t")[:3] for k, ln in rows] and body[7][:4] == body[0][:3] + ["-1.5"]
    bogus = "17\t23\t+\t%s\t1.0" % name
    ev.write_text(bogus + "\n")
    err = subprocess.run(exe + ["--evidence-scan", str(ev), str(out)], capture_output=True, timeout=600)
    assert err.returncode != 0 and repr(bogus) in err.stderr.decode() and "--evidence-scan" in err.stderr.decode()
    ann.close()
