"""Scenario batches on the device (phx_scenarios_flat, Annotator.scenarios / start_drops): S masked re-annotations of the
batch last run in one call, one workgroup per scenario.  Every scenario is, by definition, reannotate() of its contig with its mask
alone, so the sibling is the yardstick byte for byte; on one contig the in-place Bellman-Ford of conftest is the independent one."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_cases, load_golden

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def helpers():
    import test_reannotate_gpu as t  # its generators and its yardstick, unchanged

    return t


def sibling(ann, i, F, solve_all=True):
    """(status, delta bits, gene bytes) of contig i from reannotate() with the mask F on that contig alone."""
    forbid = [None] * ann.n
    forbid[i] = None if F is None or len(F) == 0 else np.asarray(F)
    st, offs, genes, delta = ann.reannotate(forbid, solve_all=solve_all)
    return int(st[i]), delta[i].tobytes(), genes[offs[i]:offs[i + 1]].tobytes()


def scenario_triples(res):
    st, offs, genes, delta = res
    return [(int(st[j]), delta[j].tobytes(), genes[offs[j]:offs[j + 1]].tobytes()) for j in range(len(st))]


def called_orfs(ann, i, st0, offs0, genes0):
    if st0[i] != 0:
        return []
    return [ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in genes0[offs0[i]:offs0[i + 1]] if abs(int(g["frame"])) <= 3]


# ---- the batch and the scenarios of cases 1-3 ----
def case1_seqs(pa):
    seqs = [pa.synth_contig(71, 20000), pa.synth_contig(72, 9000)]
    assert "phiX174" in golden_cases()
    seqs.append(load_golden("phiX174")[2])
    return seqs


def case1_scenarios(ann, dl):
    """About 40 scenarios over the three contigs: empty lists, one called ORF, a whole stop group, three random called ORFs, a random
    uncalled ORF, duplicates inside a list, and the 9 kb contig ten times in a row."""
    st0, offs0, genes0 = dl
    rng = np.random.RandomState(1701)
    scen = []
    for i in range(ann.n):
        cg = called_orfs(ann, i, st0, offs0, genes0)
        orfs = ann.orfs(i)
        assert len(cg) >= 4
        scen.append((i, []))
        scen.append((i, [cg[len(cg) // 2]]))
        k = cg[1]
        scen.append((i, np.nonzero(orfs["group"] == orfs["group"][k])[0]))
        scen.append((i, sorted(rng.choice(cg, 3, replace=False).tolist())))
        uncalled = sorted(set(range(len(orfs))) - set(cg))
        scen.append((i, [uncalled[rng.randint(len(uncalled))]]))
        scen.append((i, [cg[0], cg[0], cg[-1], cg[0], cg[-1]]))
        scen.append((i, [cg[-2]]))
        scen.append((i, None))
        scen.append((i, [cg[2], uncalled[0]]))
    cg = called_orfs(ann, 1, st0, offs0, genes0)
    for r in range(10):  # the same contig ten times in a row
        scen.append((1, [cg[r % len(cg)]] if r != 4 else []))
    return scen


def result_digest(res):
    h = hashlib.sha256()
    for x in res:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def case1(pa):
    ann = pa.Annotator()
    ann.upload(case1_seqs(pa))
    ann.run()
    dl = ann.download_flat(exact=False)
    scen = case1_scenarios(ann, dl)
    res = ann.scenarios(scen)
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
    res = ann.scenarios(scen)
    print("SCEN %d %d %s" % (len(scen), ann.scenario_chunks(), result_digest(res)))
    ann.close()


# ---- 1. equals the sibling, byte for byte ----
def test_every_scenario_equals_reannotate_with_its_mask_alone(case1):
    ann, dl, scen, res, chunks = case1
    st0, offs0, genes0 = dl
    assert 35 <= len(scen) <= 45 and chunks == 1
    got = scenario_triples(res)
    st, offs, genes, delta = res
    assert offs[0] == 0 and offs[-1] == len(genes) and (np.diff(offs) >= 0).all()
    kinds = set()
    for j, (i, F) in enumerate(scen):
        assert got[j] == sibling(ann, i, F), (j, i, F)
        if F is None or len(F) == 0:  # the device path
            assert got[j] == (int(st0[i]), np.float64(0.0).tobytes(), genes0[offs0[i]:offs0[i + 1]].tobytes()), j
        kinds.add(0 if F is None or len(F) == 0 else 1 if len(F) == 1 else 2)
    assert kinds == {0, 1, 2}
    assert any(got[j][2] != genes0[offs0[i]:offs0[i + 1]].tobytes() for j, (i, F) in enumerate(scen))  # some mask changes the annotation
    # the same call again: the cached solve, the same bytes
    assert result_digest(ann.scenarios(scen)) == result_digest(res)
    ms = ann.scenarios_ms()
    assert set(ms) == {"mask", "solve", "finish"} and ms["solve"] > 0


# ---- 2. independent of the sibling ----
def test_the_9kb_contigs_scenarios_against_the_in_place_bellman_ford(case1):
    t = helpers()
    ann, dl, scen, res, chunks = case1
    st, offs, genes, delta = res
    ref = t.Ref(ann, 1)
    D = ann.path(1)[1]
    n = 0
    for j, (i, F) in enumerate(scen):
        if i != 1:
            continue
        F = [] if F is None else [int(k) for k in F]
        DF, path, want = ref.solve(F)[:3]
        got_path, got_D = ann.scenario_path(j, 1)
        if DF is None:
            assert st[j] == 1 and delta[j] == np.inf and offs[j + 1] == offs[j] and len(got_path) == 0, j
        else:
            assert st[j] == 0, (j, int(st[j]))
            assert got_D == DF and DF >= D, (j, got_D, DF, D)
            assert float(delta[j]) == float(DF - D) / 1000.0, (j, float(delta[j]), DF - D)
            assert got_path.tolist() == path, j
            assert t.gene_tuples(genes[offs[j]:offs[j + 1]]) == want, j
        n += 1
    assert n >= 15


# ---- 3. chunking does not matter ----
def test_three_or_more_chunks_give_the_same_bytes(case1):
    ann, dl, scen, res, chunks = case1
    # a slot of the 20 kb contig needs some hundred KB; a budget of one such slot forces a chunk per one or two scenarios
    code = "import sys; sys.path.insert(0, %r); import test_scenarios_gpu as t; t.child_main()" % HERE
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=600, env=dict(os.environ, PHX_SCEN_BYTES="300000"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("SCEN ")][-1].split()
    assert int(line[1]) == len(scen)
    assert int(line[2]) >= 3, line
    assert line[3] == result_digest(res)


# ---- 4. wide classes and an untiled window ----
def check_three_scenarios(ann, i, want_limbs=None):
    st0, offs0, genes0 = ann.download_flat(exact=False)
    assert st0[i] == 0
    if want_limbs is not None:
        assert int(ann.globals(i).n_limbs) == want_limbs, int(ann.globals(i).n_limbs)
    cg = called_orfs(ann, i, st0, offs0, genes0)
    scen = [(i, []), (i, [cg[len(cg) // 2]]), (i, [cg[0], cg[-1]])]
    got = scenario_triples(ann.scenarios(scen))
    for j, (_, F) in enumerate(scen):
        assert got[j] == sibling(ann, i, F), (j, F)
    return scen


@pytest.mark.parametrize("ncodons,limbs", [(3000, 4), (5500, 8)])
def test_wide_classes(pa, ncodons, limbs):
    t = helpers()
    ann = pa.Annotator()
    t.run_batch(ann, [pa.synth_contig(5, 6000).decode(), t.wide_contig(pa, ncodons, 42)])
    check_three_scenarios(ann, 1, limbs)
    ann.close()


def test_the_1088_bit_class(pa):
    t = helpers()
    ann = pa.Annotator()
    t.run_batch(ann, [t.wide_contig(pa, 12000, 42)])
    st0, offs0, genes0 = ann.download_flat(exact=False)
    assert st0[0] == 0 and int(ann.globals(0).n_limbs) == 17
    cg = called_orfs(ann, 0, st0, offs0, genes0)
    F = [cg[len(cg) // 2]]
    assert scenario_triples(ann.scenarios([(0, F)])) == [sibling(ann, 0, F)]
    ann.close()


def test_an_untiled_window_under_scenarios(pa):
    t = helpers()
    ann = pa.Annotator(flags=("solver_no_wave",))
    st0, offs0, genes0 = t.run_batch(ann, [t.wide_contig(pa, 6000, 6000, density=0.2)])
    indeg = np.bincount(ann.edges(0)["dst"])
    big = int(indeg.argmax())
    assert st0[0] == 0 and indeg[big] > 1024
    pos = ann.nodes(0)["pos"]
    own = [g for g in genes0 if abs(int(g["frame"])) <= 3 and int(g["strand"]) == 1 and int(g["right"]) == int(pos[big]) + 2]
    assert len(own) == 1  # the called gene whose edge is one of the untiled window's rows
    k = ann.orf_index(0, int(own[0]["left"]), int(own[0]["right"]), 1)
    cg = called_orfs(ann, 0, st0, offs0, genes0)
    scen = [(0, []), (0, [k]), (0, [k, cg[0]])]
    got = scenario_triples(ann.scenarios(scen))
    for j, (_, F) in enumerate(scen):
        assert got[j] == sibling(ann, 0, F), j
    assert got[1] != got[0]
    ann.close()


# ---- 5. statuses in one call ----
def test_statuses_in_one_call(pa):
    t = helpers()
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops
    rng = np.random.RandomState(12)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    huge = pa.synth_contig(320, 2000).decode() + "atg" + "".join(sense[i] for i in rng.randint(0, len(sense), 24000)) + "taa" + pa.synth_contig(321, 2000).decode()
    good = [pa.synth_contig(322, 9000).decode(), pa.synth_contig(323, 7000).decode()]
    bad = pa.synth_contig(324, 3000).decode()[:1500] + "x" + pa.synth_contig(324, 3000).decode()[1500:]
    ann = pa.Annotator()
    st0, offs0, genes0 = t.run_batch(ann, [bad, "acg", unreachable, huge, good[0], good[1]])
    assert st0.tolist()[:3] == [-2, -3, 1]
    k4 = called_orfs(ann, 4, st0, offs0, genes0)[0]
    k5 = called_orfs(ann, 5, st0, offs0, genes0)[0]
    everything = np.arange(len(ann.orfs(4)))
    scen = [(0, []), (4, [k4]), (4, everything), (4, [k4]), (2, []), (3, []), (5, [k5]), (1, None), (4, [])]
    st, offs, genes, delta = ann.scenarios(scen)
    assert st.tolist() == [-2, 0, int(st[2]), 0, 1, -7, 0, -3, 0]
    assert st[2] in (0, 1)
    got = scenario_triples((st, offs, genes, delta))
    for j, (i, F) in enumerate(scen):
        assert got[j] == sibling(ann, i, F), (j, i)
    for j in (0, 4, 5, 7):  # a run error, no path, overflow: no genes, +inf
        assert offs[j + 1] == offs[j] and delta[j] == np.inf
    assert got[1] == got[3] and got[1][0] == 0 and np.isfinite(delta[1])  # the healthy neighbour on both sides of the mask that refuses everything
    assert got[8] == (0, np.float64(0.0).tobytes(), genes0[offs0[4]:offs0[5]].tobytes())
    # a mask that leaves no path: every ORF of a contig whose connectors alone do not reach the target
    lone = pa.Annotator()
    t.run_batch(lone, [pa.synth_contig(410, 6000)])
    n0 = len(lone.orfs(0))
    res = lone.scenarios([(0, np.arange(n0)), (0, [])])
    assert scenario_triples(res)[0] == sibling(lone, 0, np.arange(n0))
    ref = t.Ref(lone, 0)
    if ref.solve(list(range(n0)))[0] is None:
        assert res[0][0] == 1 and res[3][0] == np.inf and res[1][1] == res[1][0]
    assert res[0][1] == 0 and res[3][1] == 0.0
    lone.close()
    ann.close()


def test_a_stop_group_without_bypass_is_nopath_in_a_scenario(pa):
    t = helpers()
    ann = pa.Annotator()
    t.run_batch(ann, t.fuzz(11, 60))
    dst, doffs, drec = ann.drop_margins()
    scen = []
    for i in range(60):
        if dst[i] != 0:
            continue
        for r in drec[doffs[i]:doffs[i + 1]]:
            if not r["bypass"]:
                orfs = ann.orfs(i)
                k = ann.orf_index(i, int(r["left"]), int(r["right"]), int(r["strand"]))
                scen.append((i, np.nonzero(orfs["group"] == orfs["group"][k])[0]))
                break
        if len(scen) >= 3:
            break
    assert scen, "no gene without a bypass among these contigs"
    st, offs, genes, delta = ann.scenarios(scen)
    assert (st == 1).all() and (delta == np.inf).all() and len(genes) == 0
    ann.close()


# ---- 6. the tie rule ----
def test_tie_rule_one_scenario_per_alternative(pa):
    t = helpers()
    ann = pa.Annotator()
    st0, offs0, genes0 = t.run_batch(ann, t.fuzz(101, 100))
    tied = [i for i in range(100) if st0[i] == 0 and int(ann.globals(i).tie) != 0][:3]
    assert tied
    scen = [(i, [k]) for i in tied for k in called_orfs(ann, i, st0, offs0, genes0)]
    got = scenario_triples(ann.scenarios(scen))
    for j, (i, F) in enumerate(scen):
        assert got[j] == sibling(ann, i, F, solve_all=False), (j, i, F)
    ann.close()


# ---- 7. start drops ----
def test_start_drops(pa):
    t = helpers()
    ann = pa.Annotator()
    t.run_batch(ann, case1_seqs(pa) + t.fuzz(11, 6))
    n = ann.n
    dst, doffs, drec = ann.drop_margins()
    st, offs, rec, soffs, genes = ann.start_drops()
    assert st.tolist() == dst.tolist() and offs.tolist() == doffs.tolist() and len(rec) == len(drec) == len(soffs) - 1
    single = restarted = 0
    for i in range(n):
        if offs[i + 1] == offs[i]:
            continue
        orfs = ann.orfs(i)
        ref = t.Ref(ann, i)
        for k in range(int(offs[i]), int(offs[i + 1])):
            r, d = rec[k], drec[k]
            assert (r["left"], r["right"], r["strand"]) == (d["left"], d["right"], d["strand"])
            assert r["orf"] == ann.orf_index(i, int(d["left"]), int(d["right"]), int(d["strand"]))
            assert 0.0 <= r["drop"] <= d["drop"], (i, k, float(r["drop"]), float(d["drop"]))  # one start refused: a subset of what the drop margin refuses
            grp = np.nonzero(orfs["group"] == orfs["group"][r["orf"]])[0]
            if [g for g in grp if ref.orf_edge[g] is not None] == [r["orf"]]:
                assert r["drop"].tobytes() == d["drop"].tobytes(), (i, k)
                single += 1
            new = genes[soffs[k]:soffs[k + 1]]
            assert (r["status"] == 1) == (r["drop"] == np.inf)
            if r["restart"] >= 0:
                o, o2 = orfs[r["orf"]], orfs[r["restart"]]
                assert r["restart"] != r["orf"] and o2["stop"] == o["stop"] and (o2["frame"] > 0) == (o["frame"] > 0)
                assert r["restart"] in ref.called(new)
                restarted += 1
            else:
                stops = {(int(orfs[x]["stop"]), bool(orfs[x]["frame"] > 0)) for x in ref.called(new)}
                assert (int(orfs[r["orf"]]["stop"]), bool(orfs[r["orf"]]["frame"] > 0)) not in stops
            assert r["orf"] not in ref.called(new)
    assert single >= 3 and restarted >= 3, (single, restarted)
    i = 1  # every record of one contig against reannotate() with the one-ORF mask
    for k in range(int(offs[i]), int(offs[i + 1])):
        s, dbits, gbytes = sibling(ann, i, [int(rec[k]["orf"])], solve_all=False)
        assert (int(rec[k]["status"]), rec[k]["drop"].tobytes(), genes[soffs[k]:soffs[k + 1]].tobytes()) == (s, dbits, gbytes), k
    ann.close()


# ---- 8. disturbs nothing; state and argument errors ----
def raw_call(ann, contig, off, orf, oo=None):
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    contig, off, orf = np.ascontiguousarray(contig, np.int32), np.ascontiguousarray(off, np.int64), np.ascontiguousarray(orf, np.int32)
    oo = np.ascontiguousarray(ann.orf_offsets() if oo is None else oo, np.int64)
    S = len(contig)
    offs, st, delta, total = np.zeros(S + 1, np.int64), np.zeros(S + 1, np.int32), np.zeros(S + 1), C.c_int64()
    return ann.L.phx_scenarios_flat(ann.h, S, vp(contig), vp(off), vp(orf), vp(oo), 0, None, 0, vp(offs), vp(st), vp(delta), C.byref(total))


def test_scenarios_disturb_nothing_and_state_and_argument_errors(pa):
    t = helpers()
    ann = pa.Annotator()
    ann.upload([pa.synth_contig(5, 5000)])
    with pytest.raises(pa.PhxError) as e:  # before a run (orf_offsets itself needs one)
        ann.scenarios([(0, [])])
    assert e.value.code == -13
    assert raw_call(ann, [0], [0, 0], [0], oo=[0, 0]) == -13
    seqs = t.fuzz(31, 12)
    ann.upload(seqs)
    ann.run()
    st0, offs0, genes0 = ann.download_flat(exact=False)
    mask = [called_orfs(ann, i, st0, offs0, genes0)[:2] or None for i in range(ann.n)]

    def everything():
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()],
                [x.tobytes() for x in ann.replacements()], [x.tobytes() for x in ann.reannotate(mask)], [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n)])

    before = everything()
    scen = [(i, m[:1]) for i, m in enumerate(mask) if m] + [(i, []) for i in range(ann.n)]
    res = ann.scenarios(scen)
    assert [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n)] == before[5]  # reannotate()'s cached result stands
    assert everything() == before
    assert result_digest(ann.scenarios(scen)) == result_digest(res)
    # argument errors, all before any kernel
    oo = ann.orf_offsets()
    n0 = int(oo[1] - oo[0])
    assert raw_call(ann, [0, 1], [0, 1, 2], [0, 0]) == 0
    assert raw_call(ann, [ann.n], [0, 0], [0]) == -1 and raw_call(ann, [-1], [0, 0], [0]) == -1  # a contig outside the batch
    assert raw_call(ann, [0], [0, 1], [n0]) == -1 and raw_call(ann, [0], [0, 1], [-1]) == -1  # an ORF outside its contig
    assert raw_call(ann, [0, 1], [0, 2, 1], [0, 0]) == -1  # offsets that decrease
    assert raw_call(ann, [0], [1, 1], [0, 0]) == -1  # ... or do not start at 0
    assert raw_call(ann, [0], [0, 0], [0], oo=oo + 1) == -1 and raw_call(ann, [0], [0, 0], [0], oo=np.concatenate([oo[:-1], [oo[-1] + 1]])) == -1
    assert result_digest(ann.scenarios(scen)) == result_digest(res) and everything() == before  # the refused calls left nothing behind
    # the next upload invalidates the result
    ann.scenario_path(0, scen[0][0])
    ann.upload(seqs[:3])
    with pytest.raises(pa.PhxError) as e:
        ann.scenario_path(0, 0)
    assert e.value.code == -13
    assert raw_call(ann, [0], [0, 0], [0], oo=oo[:4]) == -13
    ann.run()
    with pytest.raises(pa.PhxError) as e:
        ann.scenario_path(0, 0)
    assert e.value.code == -13
    fresh = pa.Annotator()
    fresh.upload(seqs[:3])
    fresh.run()
    small = [s for s in scen if s[0] < 3]
    assert result_digest(ann.scenarios(small)) == result_digest(fresh.scenarios(small))
    fresh.close()
    ann.close()


# ---- 9. the CLI ----
def test_cli_start_drops(pa, tmp_path):
    from phanotate_amd.cli import format_start_drops

    seqs = {"c1": pa.synth_contig(71, 20000).decode(), "c2": pa.synth_contig(72, 9000).decode()}
    fasta = tmp_path / "two.fasta"
    fasta.write_text("".join(">%s\n%s\n" % (k, v) for k, v in seqs.items()))
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    out = tmp_path / "two.sd"
    run = subprocess.run(exe + ["--start-drops", str(out)], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    called = [ln.split("\t")[:3] for ln in run.stdout.decode().splitlines() if ln and not ln.startswith("#")]
    text = out.read_text()
    rows = [ln.split("\t") for ln in text.splitlines() if not ln.startswith("#")]
    assert [ln for ln in text.splitlines() if ln.startswith("#id:")] == ["#id:\tc1", "#id:\tc2"]
    assert [r[:3] for r in rows] == called  # one line per called gene, in the order of the tabular output
    for r in rows:
        assert len(r) in (5, 6) and float(r[3]) >= 0.0 and (r[4] == "-" if len(r) == 5 else (int(r[4]) > 0 and int(r[5]) == int(r[1])))
    ann = pa.Annotator()
    ann.upload(list(seqs.values()))
    ann.set_trnas(None)
    ann.run()
    st, offs, rec, soffs, genes = ann.start_drops()
    assert text == format_start_drops(list(seqs), st, offs, rec)
    ann.close()
    # several batches give the same file
    many = subprocess.run(exe + ["--start-drops", str(tmp_path / "many.sd"), "--batch-bases", "21000"], capture_output=True, timeout=600)
    assert many.returncode == 0 and (tmp_path / "many.sd").read_text() == text and many.stdout == run.stdout
    for bad, word in ((["--start-drops", str(out), "-d"], b"-d/--dump"), (["--start-drops", str(out), "--gpus", "2"], b"--gpus above 1")):
        r = subprocess.run(exe + bad, capture_output=True, timeout=600)
        assert r.returncode == 2 and word in r.stderr
    r = subprocess.run(exe + ["--start-drops", str(out)], capture_output=True, timeout=600, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and b"multi-rank" in r.stderr
