"""Pinned scenario batches on the device (phx_pinned_scenarios_flat, Annotator.pinned_scenarios / alt_starts): S pinned
re-annotations of the batch last run in one call, one workgroup per scenario.  Every scenario is, by definition, constrain() of its
contig with its two sets alone, so the sibling is the yardstick byte for byte; on one contig the in-place Bellman-Ford of
tests/test_constrain_gpu.py (Ref) is the independent one."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE, S_NEGCYCLE, S_NOPATH, S_OVERFLOW = -1, -13, -9, 1, -7


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def helpers():
    import test_constrain_gpu as t  # its generators and its yardstick, unchanged

    return t


def scen_helpers():
    import test_scenarios_gpu as s

    return s


def as_list(x):
    return [] if x is None else [int(k) for k in x]


def sibling(ann, i, F, R):
    """(status, delta bits, unmet, gene bytes) of contig i from constrain() with the sets F and R on that contig alone, every contig solved."""
    forbid, require = [None] * ann.n, [None] * ann.n
    forbid[i] = None if F is None or len(F) == 0 else np.asarray(F)
    require[i] = None if R is None or len(R) == 0 else np.asarray(R)
    st, offs, genes, delta, unmet = ann.constrain(forbid, require, solve_all=True)
    return int(st[i]), delta[i].tobytes(), int(unmet[i]), genes[offs[i]:offs[i + 1]].tobytes()


def quads(res):
    st, offs, genes, delta, unmet = res
    return [(int(st[j]), delta[j].tobytes(), int(unmet[j]), genes[offs[j]:offs[j + 1]].tobytes()) for j in range(len(st))]


def result_digest(res):
    h = hashlib.sha256()
    for x in res:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def uncalled_through(ann, i, mres, called):
    """Uncalled ORFs of contig i some source -> target path runs through, in orfs(i) order."""
    mst, moffs, mrec = mres
    rec = mrec[moffs[i]:moffs[i + 1]]
    return [int(k) for k in np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0] if int(k) not in called]


# ---- the batch and the scenarios of cases 1-3 ----
def case1_seqs(pa):
    from phanotate_amd.fasta import read_fasta

    seqs = list(scen_helpers().case1_seqs(pa))  # synth 20 kb, synth 9 kb, phiX174
    cyc = list(read_fasta(os.path.join(ROOT, "tests", "golden", "constrain_cycle.fasta")))
    assert [nm for nm, _ in cyc] == ["fuzz11_74", "fuzz11_0"]
    return seqs + [s for _, s in cyc]


def case1_scenarios(ann, dl):
    """Eight kinds of scenario for each of the five contigs, a required ORF on a cycle (alone, and with an edge of the cycle refused)
    between healthy scenarios of the same contig for the two cycle contigs, and the 9 kb contig ten times in a row, plain and pinned
    slots alternating.  (The cycle contigs are small: a kind that needs more genes than they call wraps around.)"""
    t, s = helpers(), scen_helpers()
    st0, offs0, genes0 = dl
    mres = ann.margins()
    rng = np.random.RandomState(1801)
    scen = []
    for i in range(ann.n):
        cg = s.called_orfs(ann, i, st0, offs0, genes0)
        group = ann.orfs(i)["group"]
        norf = len(group)
        unc = uncalled_through(ann, i, mres, set(cg)) or [k for k in range(norf) if k not in cg]
        assert cg and len(unc) >= 2, (i, len(cg), len(unc))
        u = unc[rng.randint(len(unc))]
        scen.append((i, [], []))
        scen.append((i, [], [u]))  # one uncalled ORF required
        scen.append((i, None, [cg[len(cg) // 2]]))  # a called gene required
        twin = next(((a, b) for a in unc + cg for b in np.nonzero(group == group[a])[0].tolist() if b != a), None)
        assert twin is not None, i
        scen.append((i, None, list(twin)))  # two starts of one stop group
        scen.append((i, [cg[1 % len(cg)]], [unc[0]]))  # one required, a called gene refused
        gone = cg[2 % len(cg)]
        other = next(k for k in unc + cg if group[k] != group[gone])
        scen.append((i, np.nonzero(group == group[gone])[0], [other]))  # a whole stop group refused, an ORF of another group required
        scen.append((i, [cg[-1], cg[-1], cg[0]], [u, unc[-1], u, u, unc[-1]]))  # duplicates in both lists
        scen.append((i, None, None))
    for i in (3, 4):  # the contigs of tests/golden/constrain_cycle.fasta
        ref = t.Ref(ann, i)
        cyc = [k for k, e in enumerate(ref.orf_edge) if e is not None and ref.on_cycle({e})]
        free = [k for k, e in enumerate(ref.orf_edge) if e is not None and k not in cyc]
        assert cyc and free, i
        k = cyc[0]
        cut = [x for x, e in enumerate(ref.orf_edge) if e is not None and x != k and not ref.on_cycle({ref.orf_edge[k]}, {e})]
        scen.append((i, [], None))
        scen.append((i, None, [k]))  # PHX_S_NEGCYCLE between two healthy scenarios of the same contig
        scen.append((i, None, [free[0]]))
        if cut:
            scen.append((i, [cut[0]], [k]))  # an edge of the cycle refused: a result again
    cg = s.called_orfs(ann, 1, st0, offs0, genes0)
    unc = uncalled_through(ann, 1, mres, set(cg))
    assert len(cg) >= 4 and len(unc) >= 4
    for r in range(10):  # the same contig ten times in a row: plain and pinned slots at two widths in one distance buffer
        scen.append((1, [cg[r % len(cg)]], None) if r % 2 == 0 else (1, [cg[r % len(cg)]] if r % 4 == 1 else None, [unc[(3 * r) % len(unc)]]))
    return scen


@pytest.fixture(scope="module")
def case1(pa):
    ann = pa.Annotator()
    ann.upload(case1_seqs(pa))
    ann.run()
    dl = ann.download_flat(exact=False)
    assert dl[0].tolist() == [0] * 5
    scen = case1_scenarios(ann, dl)
    res = ann.pinned_scenarios(scen)
    chunks = ann.scenario_chunks()
    yield ann, dl, scen, res, chunks
    ann.close()


def child_main():
    """Case 3's child process: the scenarios of case 1 under the PHX_SCEN_BYTES of the environment; prints the chunk count and a digest."""
    import phanotate_amd as pa

    ann = pa.Annotator()
    ann.upload(case1_seqs(pa))
    ann.run()
    scen = case1_scenarios(ann, ann.download_flat(exact=False))
    res = ann.pinned_scenarios(scen)
    print("PSCEN %d %d %s" % (len(scen), ann.scenario_chunks(), result_digest(res)))
    ann.close()


# ---- 1. equals the sibling, byte for byte ----
def test_every_scenario_equals_constrain_with_its_sets_alone(case1):
    ann, dl, scen, res, chunks = case1
    st0, offs0, genes0 = dl
    assert 40 <= len(scen) <= 70 and chunks == 1
    got = quads(res)
    st, offs, genes, delta, unmet = res
    assert offs[0] == 0 and offs[-1] == len(genes) and (np.diff(offs) >= 0).all()
    print("nodes per contig (a pinned slot of an odd count has an odd number of 3-limb words):", [int(ann.globals(i).n_node) for i in range(ann.n)],
          "edge_off of contig 1 modulo 32:", int(np.cumsum([0] + [int(ann.globals(i).n_edge) for i in range(ann.n)])[1]) % 32)
    plain = [(i, F) for i, F, R in scen if len(as_list(R)) == 0]
    plain_got = scen_helpers().scenario_triples(ann.scenarios(plain))  # (another key: solves again)
    p = 0
    for j, (i, F, R) in enumerate(scen):
        assert got[j] == sibling(ann, i, F, R), (j, i, as_list(F), as_list(R), got[j][:3])
        if len(as_list(R)) == 0:  # scenarios()' scenario byte for byte, unmet 0
            assert (got[j][0], got[j][1], got[j][3]) == plain_got[p] and got[j][2] == 0, j
            p += 1
        if len(as_list(R)) == 0 and len(as_list(F)) == 0:  # the device path
            assert got[j] == (0, np.float64(0.0).tobytes(), 0, genes0[offs0[i]:offs0[i + 1]].tobytes()), j
    assert any(got[j][0] == 0 and got[j][2] == 0 and len(as_list(R)) and got[j][3] != genes0[offs0[i]:offs0[i + 1]].tobytes() for j, (i, F, R) in enumerate(scen))
    cyc = [j for j in range(1, len(scen) - 1) if st[j] == S_NEGCYCLE and scen[j - 1][0] == scen[j][0] == scen[j + 1][0] and st[j - 1] == 0 and st[j + 1] == 0]
    assert cyc, st.tolist()
    for j in np.nonzero(st == S_NEGCYCLE)[0]:
        assert offs[j + 1] == offs[j] and delta[j] == np.inf and unmet[j] == len(set(as_list(scen[j][2])))
    # the same call again: the cached solve, the same bytes (the scenarios() call above took the cache: this one solves, the next does not)
    assert result_digest(ann.pinned_scenarios(scen)) == result_digest(res)
    assert result_digest(ann.pinned_scenarios(scen)) == result_digest(res)
    ms = ann.scenarios_ms()
    assert set(ms) == {"mask", "solve", "finish"} and ms["solve"] > 0 and ann.scenario_chunks() == 1


# ---- 2. independent of the sibling ----
def test_the_9kb_contigs_scenarios_against_the_in_place_bellman_ford(case1):
    t = helpers()
    ann, dl, scen, res, chunks = case1
    assert result_digest(ann.pinned_scenarios(scen)) == result_digest(res)  # (the path tap serves the last solve)
    st, offs, genes, delta, unmet = res
    ref = t.Ref(ann, 1)
    D = ann.path(1)[1]
    n = pinned = 0
    for j, (i, F, R) in enumerate(scen):
        if i != 1:
            continue
        F, R = as_list(F), sorted(set(as_list(R)))
        sol = ref.solve(F, R)
        got_path, got_W = ann.scenario_path(j, 1)
        if sol["cycle"] or sol["W"] is None:
            assert st[j] == (S_NEGCYCLE if sol["cycle"] else S_NOPATH) and delta[j] == np.inf and offs[j + 1] == offs[j] and len(got_path) == 0 and unmet[j] == len(R), j
        else:
            assert st[j] == 0, (j, int(st[j]))
            assert got_W == sol["W"], (j, got_W, sol["W"])
            assert float(delta[j]) == float(sol["W"] - D) / 1000.0, (j, float(delta[j]), sol["W"] - D)
            assert unmet[j] == len(R) - sol["count"], (j, int(unmet[j]), len(R), sol["count"])
            assert got_path.tolist() == sol["path"], j
            assert t.gene_tuples(genes[offs[j]:offs[j + 1]]) == sol["genes"], j
        n += 1
        pinned += len(R) > 0
    assert n >= 15 and pinned >= 8, (n, pinned)


# ---- 3. chunking does not matter ----
def test_three_or_more_chunks_give_the_same_bytes(case1):
    ann, dl, scen, res, chunks = case1
    # a slot of the 20 kb contig needs some hundred KB: the budget holds one or two slots, and a pinned one (one limb more per node, a
    # second bitmap slice) counts for more than a plain one
    code = "import sys; sys.path.insert(0, %r); import test_pinned_scenarios_gpu as t; t.child_main()" % HERE
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=600, env=dict(os.environ, PHX_SCEN_BYTES="300000"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("PSCEN ")][-1].split()
    assert int(line[1]) == len(scen)
    assert int(line[2]) >= 3, line
    assert line[3] == result_digest(res)


# ---- 4. wide classes and an untiled window ----
def check_three(ann, i, k, refused):
    scen = [(i, [], []), (i, None, [k]), (i, [refused], [k])]
    res = ann.pinned_scenarios(scen)
    got = quads(res)
    for j, (_, F, R) in enumerate(scen):
        assert got[j] == sibling(ann, i, F, R), (j, as_list(F), as_list(R), got[j][:3])
    return got


@pytest.mark.parametrize("ncodons,limbs", [(3000, 4), (5500, 8), (12000, 17)])
def test_wide_classes(pa, ncodons, limbs):
    t, s = helpers(), scen_helpers()
    ann = pa.Annotator()
    st0, offs0, genes0 = t.run_batch(ann, [pa.synth_contig(5, 6000).decode(), t.wide_contig(pa, ncodons, 42)])
    assert st0[1] == 0 and int(ann.globals(1).n_limbs) == limbs, int(ann.globals(1).n_limbs)
    cg = s.called_orfs(ann, 1, st0, offs0, genes0)
    pool = uncalled_through(ann, 1, ann.margins(), set(cg))
    k = pool[int(np.argmax(ann.orfs(1)["length"][pool]))]  # the widest weights sit in the long ORF's group: one of its starts
    got = check_three(ann, 1, k, cg[0])
    assert got[1][0] in (0, S_NEGCYCLE) and got[0][0] == 0
    ann.close()


def test_a_required_orf_in_an_untiled_window_under_scenarios(pa):
    t = helpers()
    ann = pa.Annotator(flags=("solver_no_wave",))
    st0, offs0, genes0 = t.run_batch(ann, [t.wide_contig(pa, 6000, 6000, density=0.2)])
    indeg = np.bincount(ann.edges(0)["dst"])
    big = int(indeg.argmax())
    assert st0[0] == 0 and indeg[big] > 1024
    ref = t.Ref(ann, 0)
    mst, moffs, mrec = ann.margins()
    into = [k for k, e in enumerate(ref.orf_edge) if e is not None and e[1] == big and not mrec[k]["called"] and mrec[k]["through"]]
    assert len(into) > 1000  # the required ORF's edge is one of the untiled window's rows
    own = [g for g in genes0 if abs(int(g["frame"])) <= 3 and int(g["strand"]) == 1 and int(g["right"]) == int(ref.pos[big]) + 2]
    assert len(own) == 1
    k = into[len(into) // 2]
    got = check_three(ann, 0, k, ref.called(own)[0])
    assert got[1][0] == 0 and got[1][2] == 0 and got[1][1] == mrec[k]["margin"].tobytes() and got[1] != got[0]
    ann.close()


# ---- 5. statuses and arguments in one call ----
def raw_call(ann, contig, foff, forf, roff, rorf, oo=None):
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    contig = np.ascontiguousarray(contig, np.int32)
    foff, forf, roff, rorf = np.ascontiguousarray(foff, np.int64), np.ascontiguousarray(forf, np.int32), np.ascontiguousarray(roff, np.int64), np.ascontiguousarray(rorf, np.int32)
    oo = np.ascontiguousarray(ann.orf_offsets() if oo is None else oo, np.int64)
    S = len(contig)
    offs, st, delta, um, total = np.zeros(S + 1, np.int64), np.zeros(S + 1, np.int32), np.zeros(S + 1), np.zeros(S + 1, np.int32), C.c_int64()
    return ann.L.phx_pinned_scenarios_flat(ann.h, S, vp(contig), vp(foff), vp(forf), vp(roff), vp(rorf), vp(oo), 0, None, 0, vp(offs), vp(st), vp(delta), vp(um), C.byref(total))


def test_statuses_and_arguments_in_one_call(pa):
    t, s = helpers(), scen_helpers()
    ann = pa.Annotator()
    ann.upload([pa.synth_contig(5, 5000)])
    with pytest.raises(pa.PhxError) as e:  # before a run (orf_offsets itself needs one)
        ann.pinned_scenarios([(0, None, None)])
    assert e.value.code == E_STATE
    assert raw_call(ann, [0], [0, 0], [0], [0, 0], [0], oo=[0, 0]) == E_STATE
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops
    rng = np.random.RandomState(12)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    huge = pa.synth_contig(320, 2000).decode() + "atg" + "".join(sense[i] for i in rng.randint(0, len(sense), 24000)) + "taa" + pa.synth_contig(321, 2000).decode()
    good = [pa.synth_contig(322, 9000).decode(), pa.synth_contig(323, 7000).decode()]
    bad = pa.synth_contig(324, 3000).decode()[:1500] + "x" + pa.synth_contig(324, 3000).decode()[1500:]
    seqs = [bad, "acg", unreachable, huge, good[0], good[1]]
    st0, offs0, genes0 = t.run_batch(ann, seqs)
    assert st0.tolist()[:3] == [-2, -3, 1]
    mres = ann.margins()
    cg4, cg5 = s.called_orfs(ann, 4, st0, offs0, genes0), s.called_orfs(ann, 5, st0, offs0, genes0)
    u4, u5 = uncalled_through(ann, 4, mres, set(cg4)), uncalled_through(ann, 5, mres, set(cg5))
    ref2 = t.Ref(ann, 2)
    quiet = [k for k, e in enumerate(ref2.orf_edge) if e is None or not ref2.on_cycle({e})]
    assert len(quiet) >= 2
    R2 = [quiet[0], quiet[-1]]
    scen = [(0, None, None), (4, [cg4[0]], [u4[0]]), (2, None, R2), (4, None, [u4[1], u4[0]]), (3, None, None), (5, [cg5[1]], [u5[0]]), (1, None, None), (4, [], []), (2, None, None)]
    res = ann.pinned_scenarios(scen)
    st, offs, genes, delta, unmet = res
    assert st.tolist() == [-2, int(st[1]), 1, int(st[3]), S_OVERFLOW, int(st[5]), -3, 0, 1]
    got = quads(res)
    for j, (i, F, R) in enumerate(scen):
        assert got[j] == sibling(ann, i, F, R), (j, i, got[j][:3])
    for j in (0, 2, 4, 6, 8):  # a run error, no path, overflow: no genes, +inf, every required ORF unmet
        assert offs[j + 1] == offs[j] and delta[j] == np.inf and unmet[j] == len(as_list(scen[j][2]))
    assert unmet[2] == 2
    assert st[1] in (0, S_NEGCYCLE) and st[3] in (0, S_NEGCYCLE) and st[5] in (0, S_NEGCYCLE)
    assert got[7] == (0, np.float64(0.0).tobytes(), 0, genes0[offs0[4]:offs0[5]].tobytes())
    # argument errors, all before any kernel
    oo = ann.orf_offsets()
    n4 = int(oo[5] - oo[4])
    assert raw_call(ann, [4], [0, 1], [u4[0]], [0, 1], [u4[0]]) == E_ARG  # an ORF in both lists of one scenario
    assert raw_call(ann, [4], [0, 3], [cg4[0], u4[1], cg4[1]], [0, 3], [u4[0], u4[1], u4[0]]) == E_ARG
    assert raw_call(ann, [4], [0, 1], [n4], [0, 0], [0]) == E_ARG and raw_call(ann, [4], [0, 1], [-1], [0, 0], [0]) == E_ARG  # an index out of range, either list
    assert raw_call(ann, [4], [0, 0], [0], [0, 1], [n4]) == E_ARG and raw_call(ann, [4], [0, 0], [0], [0, 1], [-1]) == E_ARG
    assert raw_call(ann, [3], [0, 0], [0], [0, 1], [0]) == E_ARG  # (a contig without device distances counts no ORFs)
    assert raw_call(ann, [6], [0, 0], [0], [0, 0], [0]) == E_ARG and raw_call(ann, [-1], [0, 0], [0], [0, 0], [0]) == E_ARG
    assert raw_call(ann, [4, 5], [0, 2, 1], [0, 0], [0, 0, 0], [0]) == E_ARG and raw_call(ann, [4, 5], [0, 0, 0], [0], [0, 2, 1], [0, 0]) == E_ARG  # offsets that decrease
    assert raw_call(ann, [4], [1, 1], [0, 0], [0, 0], [0]) == E_ARG and raw_call(ann, [4], [0, 0], [0], [1, 1], [0, 0]) == E_ARG  # ... or do not start at 0
    assert raw_call(ann, [4], [0, 0], [0], [0, 0], [0], oo=oo + 1) == E_ARG
    assert raw_call(ann, [4], [0, 0], [0], [0, 0], [0], oo=np.concatenate([oo[:-1], [oo[-1] + 1]])) == E_ARG
    ann.scenario_path(1, 4)  # the refused calls left the cached result standing: its tap still serves
    assert result_digest(ann.pinned_scenarios(scen)) == result_digest(res)
    assert raw_call(ann, [4, 5], [0, 1, 1], [cg4[0]], [0, 1, 2], [u4[0], u5[0]]) == 0
    assert raw_call(ann, [4, 4], [0, 1, 1], [u4[0]], [0, 0, 1], [u4[0]]) == 0  # refused in one scenario, required in another: fine
    assert result_digest(ann.pinned_scenarios(scen)) == result_digest(res)
    ann.scenario_path(1, 4)
    # the next upload invalidates the result
    ann.upload(seqs[4:])
    with pytest.raises(pa.PhxError) as e:
        ann.scenario_path(1, 0)
    assert e.value.code == E_STATE
    assert raw_call(ann, [0], [0, 0], [0], [0, 0], [0], oo=[0, 0, 0]) == E_STATE
    ann.close()


# ---- 6. the tie rule ----
def test_tie_rule_one_pinned_scenario_per_called_gene(pa):
    t, s = helpers(), scen_helpers()
    ann = pa.Annotator()
    st0, offs0, genes0 = t.run_batch(ann, t.fuzz(101, 100))
    tied = [i for i in range(100) if st0[i] == 0 and int(ann.globals(i).tie) != 0][:3]
    assert tied  # (at most the first three; these hundred contigs hold two)
    mres = ann.margins()
    scen = []
    for i in tied:
        cg = s.called_orfs(ann, i, st0, offs0, genes0)
        group = ann.orfs(i)["group"]
        unc = uncalled_through(ann, i, mres, set(cg))
        for x, k in enumerate(cg):  # an uncalled ORF of another stop group
            pool = [u for u in unc if group[u] != group[k]]
            if pool:
                scen.append((i, None, [pool[(7 * x) % len(pool)]]))
    assert len(scen) >= 4
    res = ann.pinned_scenarios(scen)
    got = quads(res)
    for j, (i, F, R) in enumerate(scen):
        assert got[j] == sibling(ann, i, F, R), (j, i, R)
    assert (res[0] == 0).sum() >= 2
    ann.close()


# ---- 7. disturbs nothing ----
def test_pinned_scenarios_disturb_nothing(pa):
    t, s = helpers(), scen_helpers()
    ann = pa.Annotator()
    st0, offs0, genes0 = t.run_batch(ann, t.fuzz(31, 12))
    mres = ann.margins()
    mask = [s.called_orfs(ann, i, st0, offs0, genes0)[:2] or None for i in range(ann.n)]
    keep = [(uncalled_through(ann, i, mres, set(mask[i] or []))[:1] or None) if st0[i] == 0 else None for i in range(ann.n)]

    def everything(which):
        again = ann.reannotate(mask) if which == 0 else ann.constrain(mask, keep)
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()],
                [x.tobytes() for x in ann.replacements()], [x.tobytes() for x in again], [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n) if st0[i] >= 0])

    scen = [(i, mask[i][:1], keep[i]) for i in range(ann.n) if mask[i]] + [(i, None, None) for i in range(ann.n)]
    plain = [(i, m[:1]) for i, m in enumerate(mask) if m]
    for which in (0, 1):  # a cached reannotate(), then a cached constrain()
        before = everything(which)
        plain_before = result_digest(ann.scenarios(plain))
        res = ann.pinned_scenarios(scen)
        assert [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n) if st0[i] >= 0] == before[5]  # the cached result and its path tap stand
        assert everything(which) == before
        assert result_digest(ann.scenarios(plain)) == plain_before  # scenarios() after pinned_scenarios(): what it returned before
        assert result_digest(ann.pinned_scenarios(scen)) == result_digest(res)
    ann.close()


# ---- 8. alt_starts() ----
def test_alt_starts(pa):
    t, s = helpers(), scen_helpers()
    ann = pa.Annotator()
    t.run_batch(ann, s.case1_seqs(pa) + t.fuzz(11, 6))
    n = ann.n
    dst, doffs, drec = ann.drop_margins()
    mst, moffs, mrec = ann.margins()
    st, offs, rec, soffs, genes = ann.alt_starts()
    assert st.tolist() == dst.tolist() and offs[0] == 0 and offs[n] == len(rec) == len(soffs) - 1
    clean = 0
    firsts = []  # the first alternative of every gene that has one
    for i in range(n):
        # the records of contig i: for every record of drop_margins(), in order, every other ORF of its stop group in orfs(i) order — the
        # offsets follow from drop_margins()' own
        orfs = ann.orfs(i)
        want = []
        for d in drec[doffs[i]:doffs[i + 1]]:
            k = ann.orf_index(i, int(d["left"]), int(d["right"]), int(d["strand"]))
            if (orfs["group"] == orfs["group"][k]).sum() > 1:
                firsts.append(int(offs[i]) + len(want))
            want += [(int(d["left"]), int(d["right"]), int(d["strand"]), k, int(a)) for a in np.nonzero(orfs["group"] == orfs["group"][k])[0] if a != k]
        mine = rec[offs[i]:offs[i + 1]]
        assert [(int(r["left"]), int(r["right"]), int(r["strand"]), int(r["orf"]), int(r["alt"])) for r in mine] == want, i
        if not len(mine):
            continue
        ref = t.Ref(ann, i)
        run_called = None
        for x in range(int(offs[i]), int(offs[i + 1])):
            r = rec[x]
            o, a = orfs[r["orf"]], orfs[r["alt"]]
            assert r["alt"] != r["orf"] and a["group"] == o["group"] and a["stop"] == o["stop"]
            assert ref.by_ends[(int(r["alt_left"]), int(r["alt_right"]), int(r["strand"]))] == r["alt"]
            new = genes[soffs[x]:soffs[x + 1]]
            if r["status"] == 0 and r["unmet"] == 0:
                called = ref.called(new)
                assert r["alt"] in called and r["orf"] not in called, (i, x)
                assert r["delta"].tobytes() == mrec[moffs[i] + r["alt"]]["margin"].tobytes(), (i, x, float(r["delta"]))  # §16's identity
                assert r["n_removed"] >= 1 and r["n_added"] >= 1
                clean += 1
            else:
                assert r["status"] in (0, S_NEGCYCLE, S_NOPATH)
                if r["status"] != 0:
                    assert r["unmet"] == 1 and r["delta"] == np.inf and len(new) == 0
    assert clean >= 20, clean
    i = 1  # every record of one contig against a one-ORF constrain()
    assert offs[i + 1] - offs[i] >= 5
    for x in range(int(offs[i]), int(offs[i + 1])):
        want = sibling(ann, i, None, [int(rec[x]["alt"])])
        assert (int(rec[x]["status"]), rec[x]["delta"].tobytes(), int(rec[x]["unmet"]), genes[soffs[x]:soffs[x + 1]].tobytes()) == want, x
    # max_alts: at most that many alternatives per gene, the first ones
    st1, offs1, rec1, soffs1, genes1 = ann.alt_starts(max_alts=1)
    assert rec1.tolist() == rec[firsts].tolist() and offs1[n] == len(firsts) and st1.tolist() == st.tolist()  # (field by field: the records have padding)
    ann.close()


# ---- 9. the CLI ----
def test_cli_alt_starts(pa, tmp_path):
    from phanotate_amd.cli import format_alt_starts

    seqs = {"c1": pa.synth_contig(71, 20000).decode(), "c2": pa.synth_contig(72, 9000).decode()}
    fasta = tmp_path / "two.fasta"
    fasta.write_text("".join(">%s\n%s\n" % (k, v) for k, v in seqs.items()))
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    plain = subprocess.run(exe, capture_output=True, timeout=600)
    out = tmp_path / "two.alt"
    run = subprocess.run(exe + ["--alt-starts", str(out)], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert plain.returncode == 0 and run.stdout == plain.stdout  # stdout unchanged
    text = out.read_text()
    assert [ln for ln in text.splitlines() if ln.startswith("#id:")] == ["#id:\tc1", "#id:\tc2"]
    called = {tuple(ln.split("\t")[:3]) for ln in run.stdout.decode().splitlines() if ln and not ln.startswith("#")}
    rows = [ln.split("\t") for ln in text.splitlines() if not ln.startswith("#")]
    assert rows and all(len(r) == 7 and tuple(r[:3]) in called for r in rows)
    ann = pa.Annotator()
    ann.upload(list(seqs.values()))
    ann.set_trnas(None)
    ann.run()
    st, offs, rec, soffs, genes = ann.alt_starts()
    assert text == format_alt_starts(list(seqs), st, offs, rec)
    ann.close()
    many = subprocess.run(exe + ["--alt-starts", str(tmp_path / "many.alt"), "--batch-bases", "21000"], capture_output=True, timeout=600)
    assert many.returncode == 0 and (tmp_path / "many.alt").read_text() == text and many.stdout == run.stdout
