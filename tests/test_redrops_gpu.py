"""Re-annotation drop margins on the device (phx_redrops_flat) against python integers.  The yardstick is EvRef.solve of
tests/test_evidence_gpu.py: for every CDS gene g of the re-annotation's path, in path order, the target's distance under
(forbid + every ORF of g's stop group, bias) minus the one under (forbid, bias), converted as the record converts it; no path: bypass = 0
and +inf.  Every field of every record is compared.  Also the identities with drop_margins(), the layered trees in a fresh process, the
wide classes, statuses, isolation, the cache and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_evidence_gpu import NEGCYCLE, EvRef, called_orfs, draw_orfs, evidence, solved_contigs
from test_remargins_gpu import cycle_orf, draw_penalties, some_evidence
from test_reannotate_gpu import fuzz, mask_rounds, run_batch, wide_cases
from test_scenarios_gpu import case1_seqs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def out_bytes(out, i=None):
    st, offs, rec = out
    if i is None:
        return st.tobytes(), offs.tobytes(), rec.tobytes()
    return int(st[i]), rec[offs[i]:offs[i + 1]].tobytes()


_solved = {}  # (id of the yardstick, refused set, bias) -> EvRef.solve's result: computed once, shared by the tests of a batch, never changed


def solve(ref, forbid, bias):
    key = (id(ref), frozenset(forbid or ()), frozenset((bias or {}).items()))
    if key not in _solved:
        _solved[key] = (ref, ref.solve(sorted(key[1]), dict(key[2]) or None))  # (the yardstick is kept alive: its id stays its own)
    return _solved[key][1]


def check_contig(ann, ref, forbid, bias, st, rec, genes):
    """One contig's records against the yardstick; returns NEGCYCLE, None (no path) or (D', records compared, the path's node list)."""
    i = ref.i
    sol = solve(ref, forbid, bias)
    if sol == NEGCYCLE:
        assert st == -9 and len(rec) == 0, (i, forbid, bias, st)
        return NEGCYCLE
    DB, path = sol[0], sol[1]
    if DB is None:
        assert st == 1 and len(rec) == 0, (i, forbid, bias, st)
        return None
    assert st == 0, (i, forbid, bias, st)
    assert ann.reannotated_path(i)[0].tolist() == path, i
    orfs = ref.orfs
    returned = {(int(g["left"]), int(g["right"]), int(g["strand"])) for g in genes if abs(int(g["frame"])) <= 3}
    seen = 0
    for k in range((len(path) - 1) // 2):  # the pairs of P', in path order
        a, b = path[2 * k + 1], path[2 * k + 2]
        left, right, fr = ref.pos[a], ref.pos[b] + 2, ref.frame[a]
        if abs(fr) > 3:
            continue  # (a tRNA edge is no CDS gene)
        strand = -1 if fr < 0 else 1
        o = ref.by_ends[(left, right, strand)]
        group = np.nonzero(orfs["group"] == orfs["group"][o])[0].tolist()
        assert o in group
        without = solve(ref, set(forbid or ()) | set(group), bias)
        assert without != NEGCYCLE  # (taking edges away makes no cycle negative)
        assert seen < len(rec), (i, k, len(rec))
        r = rec[seen]
        assert (int(r["left"]), int(r["right"]), int(r["strand"]), int(r["frame"])) == (left, right, strand, fr), (i, k)
        assert float(r["score"]) == ref.weight[(left, right, strand)], (i, k)
        assert int(r["called"]) == (1 if (left, right, strand) in returned else 0) == 1, (i, k)
        if without[0] is None:
            assert r["bypass"] == 0 and r["drop"] == np.inf, (i, k, float(r["drop"]))
        else:
            assert without[0] >= DB, (i, k)
            assert r["bypass"] == 1 and float(r["drop"]) == float(without[0] - DB) / 1000.0, (i, k, float(r["drop"]), without[0] - DB)
        seen += 1
    assert seen == len(rec), (i, seen, len(rec))
    return DB, seen, path


def check_batch(ann, refs, forbid, bias, solve_all=False):
    """evidence(bias, forbid) — reannotate(forbid) where there is no bias —, redrops(), every solved-again contig of refs against the
    yardstick.  {contig: check_contig's result}; at least one record was compared per contig that was solved again with a path."""
    n = ann.n
    if bias is None:
        st, offs, genes, delta = ann.reannotate(forbid, solve_all=solve_all)
    else:
        st, offs, genes, delta = evidence(ann, bias, forbid, solve_all=solve_all)
    dst, doffs, drec = ann.redrops()
    out = {}
    for i in refs:
        f = None if forbid is None else forbid[i]
        b = None if bias is None else bias[i]
        if f is None and b is None and not solve_all:
            continue
        out[i] = check_contig(ann, refs[i], f, b, int(dst[i]), drec[doffs[i]:doffs[i + 1]], genes[offs[i]:offs[i + 1]])
        assert int(dst[i]) == int(st[i]), i
        assert out[i] in (NEGCYCLE, None) or out[i][1] >= 1, i  # no solved-again contig passes without a compared record
    return out


@pytest.fixture(scope="module")
def big(pa):
    """case1_seqs + fuzz(11, 6), run once: one contig of one chunk and eight of several.  (ann, the run's download, yardsticks, the run's
    paths, the called ORFs.)  The tests leave the batch resident."""
    ann = pa.Annotator()
    dl = run_batch(ann, case1_seqs(pa) + fuzz(11, 6))
    idx = solved_contigs(ann, dl[0])
    V = {i: int(ann.globals(i).n_node) for i in idx}
    print("nodes per contig:", sorted(V.items()))
    assert any(v <= 256 for v in V.values()) and sum(v > 256 for v in V.values()) >= 8, sorted(V.items())
    refs = {i: EvRef(ann, i) for i in idx}
    called = {i: called_orfs(ann, i, dl[2][dl[1][i]:dl[1][i + 1]]) for i in idx}
    yield ann, dl, refs, {i: ann.path(i)[0].tolist() for i in idx}, called
    ann.close()
    _solved.clear()


# ---- 1. masks ----
def test_every_mask_round_against_the_yardstick(big):
    ann, dl, refs, P, called = big
    n = ann.n
    rng = np.random.RandomState(2901)
    order = sorted(refs)
    plans = dict(zip(order, mask_rounds([refs[i] for i in order], [called[i] for i in order], rng)))
    have = [i for i in order if called[i]]
    assert len(have) >= len(order) - 1
    records = moved = 0
    for r in range(max(len(plans[i]) for i in have)):
        forbid = [plans[i][r] if i in have and r < len(plans[i]) else None for i in range(n)]
        got = check_batch(ann, refs, forbid, None)
        assert set(got) == {i for i in have if r < len(plans[i])} and NEGCYCLE not in got.values()
        for i, g in got.items():
            if g is not None:
                records += g[1]
                moved += g[2] != P[i]  # (a refused called gene: P' is another path)
    print("masks: %d records, %d re-annotations with another path" % (records, moved))
    assert records >= 100 and moved >= len(have)


# ---- 2. penalties and bonuses ----
def test_penalties_alone_and_with_a_mask(big):
    ann, dl, refs, P, called = big
    bias, forbid = draw_penalties(ann, refs, called, np.random.RandomState(2902))
    assert any(f for f in forbid)
    for fb in (None, forbid):
        got = check_batch(ann, refs, fb, bias)
        assert set(got) == set(refs) and NEGCYCLE not in got.values()  # a penalty cannot make a cycle negative: no point is left out
        assert sum(g is not None for g in got.values()) >= len(refs) - 1


def test_bonuses_of_the_titration_draw(big):
    """§19's titration draw at -Delta - 1: the uncalled ORF comes in, P' changes, and the new gene has a record with a drop >= 0."""
    ann, dl, refs, P, called = big
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
        got = check_batch(ann, refs, None, bias)
        assert NEGCYCLE not in got.values() and None not in got.values(), (r, got)
        dst, doffs, drec = ann.redrops()
        for i, g in got.items():
            assert g[2] != P[i], (i, r)  # the bonus wins by one unit: another path
            o = refs[i].orfs[picks[i][r][0]]
            ends = (int(o["start"]), int(o["stop"]) + 2) if o["frame"] > 0 else (int(o["stop"]), int(o["start"]) + 2)
            mine = [x for x in drec[doffs[i]:doffs[i + 1]] if (int(x["left"]), int(x["right"])) == ends and (x["strand"] > 0) == (o["frame"] > 0)]
            assert len(mine) == 1 and mine[0]["called"] == 1 and mine[0]["drop"] >= 0.0, (i, r, ends)
        points += len(got)
    print("bonuses: %d points of the titration draw" % points)
    assert points == sum(len(p) for p in picks.values()) >= 60


# ---- 3. / 4. nothing refused, no bias ----
def check_equals_drops(ann):
    """Nothing refused, no bias.  solve_all: every contig through the conditioned kernels on an unchanged graph — the records are
    drop_margins()' byte for byte (`called` apart on a contig whose delivered genes are the host's: there drop_margins() marks those,
    redrops() the device's list) and the counters are drop_stats().  Without: drop_margins()' arrays byte for byte (no contig is solved again)."""
    n = ann.n
    want = ann.drop_margins()
    cert = ann.certified()
    ann.reannotate([None] * n, solve_all=True)
    got = ann.redrops()
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
    seen = 0
    for i in range(n):
        a, b = got[2][got[1][i]:got[1][i + 1]], want[2][want[1][i]:want[1][i + 1]]
        if cert[i] == 1:
            assert a.tobytes() == b.tobytes(), i
            seen += len(a) > 0
        else:
            for f in ("left", "right", "strand", "frame", "score", "drop", "bypass"):
                assert a[f].tobytes() == b[f].tobytes(), (i, f)
    assert ann.redrop_stats() == ann.drop_stats()
    assert all(v > 0 for k, v in ann.redrops_ms().items() if k != "download") or len(want[2]) == 0
    ann.reannotate([None] * n)
    assert out_bytes(ann.redrops()) == out_bytes(want)
    assert ann.redrops_ms() == dict(trees=0.0, candidates=0.0, fixups=0.0, download=0.0)  # (no conditioned kernel ran)
    return seen


def test_nothing_refused_no_bias_is_drop_margins_byte_for_byte(pa, big):
    assert check_equals_drops(big[0]) >= 5
    ann = pa.Annotator()
    run_batch(ann, fuzz(101, 150))  # the cross-node batch of tests/test_drop_gpu.py: step 4 and the rescan run as often as in the run's drops
    assert check_equals_drops(ann) >= 75
    print("cross-node batch:", ann.drop_stats())
    ann.close()


# ---- 5. the layered rebuild, in a fresh process ----
LAYERED_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tools")
import phanotate_amd as pa, fuzz_gpu
rng = np.random.RandomState(101)
seqs = [fuzz_gpu.make(rng) for _ in range(150)]
ann = pa.Annotator()
ann.upload(seqs)
ann.run()
want = [x.tobytes().hex() for x in ann.drop_margins()]
cert = ann.certified().tolist()
ann.reannotate([None] * ann.n, solve_all=True)
same = [x.tobytes().hex() for x in ann.redrops()]
stats = (ann.drop_stats(), ann.redrop_stats())
st0, offs0, genes0 = ann.download_flat(exact=False)
bias, forbid = [], []
for i in range(ann.n):  # per solved contig a refused called gene, a penalised one and three ORFs with a bonus
    cg = [ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in genes0[offs0[i]:offs0[i + 1]] if abs(int(g["frame"])) <= 3] if st0[i] == 0 else []
    if len(cg) < 2:
        bias.append(None); forbid.append(None)
        continue
    b = {int(k): -float(rng.randint(1, 3000)) / 1000.0 for k in rng.choice(len(ann.orfs(i)), min(3, len(ann.orfs(i))), replace=False)}
    b[cg[len(cg) // 2]] = 5.0
    bias.append(sorted(b.items())); forbid.append([cg[0]])
ann.evidence(bias, forbid)
under = [x.tobytes().hex() for x in ann.redrops()]
print(json.dumps({"want": want, "same": same, "cert": cert, "stats": stats, "under": under, "ustats": ann.redrop_stats(), "solved": sum(b is not None for b in bias)}))
"""


def test_layered_trees_give_the_same_records(pa):
    outs = []
    for env in ({}, {"PHX_DROP_LAYERED": "1"}):
        r = subprocess.run([sys.executable, "-c", LAYERED_CHILD, ROOT], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    a, b = outs
    for o in outs:  # the comparison of test 3, in either mode
        assert o["same"][:2] == o["want"][:2] and o["stats"][0] == o["stats"][1]
        if all(c == 1 for c in o["cert"]):  # (else `called` may differ on a contig whose delivered genes are the host's: test 3 looks closer)
            assert o["same"][2] == o["want"][2]
    assert a["want"] == b["want"] and a["same"] == b["same"] and a["under"] == b["under"]
    assert a["solved"] >= 100 and len(a["under"][2]) > 0
    assert a["stats"][1]["layered"] < 50 and b["stats"][1]["layered"] >= 100 and b["ustats"]["layered"] >= 100 > a["ustats"]["layered"]
    assert a["ustats"]["slots"] == b["ustats"]["slots"] > 0


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
    rng = np.random.RandomState(2906 + case)
    forbid = [None] * len(seqs)
    forbid[i] = [cg[int(rng.randint(len(cg)))]]
    got = check_batch(ann, refs, forbid, None)
    assert got[i] is not NEGCYCLE
    bias = [None] * len(seqs)
    bias[i] = {k: int(10 ** rng.uniform(1, 6)) for k in draw_orfs(refs[i], cg, rng, 6)}
    got = check_batch(ann, refs, None, bias)
    assert got[i] not in (NEGCYCLE, None) and got[i][1] >= 1
    ann.close()
    _solved.clear()


# ---- 7. statuses ----
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
    good = [pa.synth_contig(322, 9000).decode(), pa.synth_contig(323, 7000).decode(), pa.synth_contig(325, 8000).decode()]
    bad = pa.synth_contig(324, 3000).decode()[:1500] + "x" + pa.synth_contig(324, 3000).decode()[1500:]
    # a run error, too short, a mask that leaves no path, a negative cycle, one that is not solved again, two clean ones
    seqs = [bad, "acg", pa.synth_contig(410, 6000), neg[0], good[2], good[0], good[1]]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    with pytest.raises(pa.PhxError) as e:  # before any re-annotation of the run
        ann.redrops()
    assert e.value.code == -13 and "no re-annotation" in str(e.value)
    assert st0.tolist() == [-2, -3, 0, 0, 0, 0, 0]
    forbid = [None, None, np.arange(len(ann.orfs(2))), None, None, None, None]
    bias = [None, None, None, {neg[1]: -10 ** 9}, None, None, None]
    for i in (5, 6):
        bias[i] = {called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])[0]: 4000, 3: -2500}
    st, offs, genes, delta = evidence(ann, bias, forbid)
    assert st.tolist() == [-2, -3, 1, -9, 0, 0, 0]
    dst, doffs, drec = ann.redrops()
    assert dst.tolist() == [-2, -3, 1, -9, 0, 0, 0]
    assert np.diff(doffs).tolist()[:4] == [0, 0, 0, 0] and all(doffs[i + 1] > doffs[i] for i in (4, 5, 6))
    run = ann.drop_margins()
    assert out_bytes((dst, doffs, drec), 4) == out_bytes(run, 4)  # not solved again: the run's records byte for byte
    for k, i in enumerate((5, 6)):  # the neighbours are unaffected
        got = check_contig(ann, EvRef(ann, i), None, bias[i], int(dst[i]), drec[doffs[i]:doffs[i + 1]], genes[offs[i]:offs[i + 1]])
        assert got[1] >= 1
        lone = pa.Annotator()
        run_batch(lone, [good[k]])
        evidence(lone, [bias[i]])
        assert out_bytes(lone.redrops(), 0) == out_bytes((dst, doffs, drec), i)
        lone.close()
    # required ORFs on any contig: PHX_E_STATE, and the text says why
    req = [None] * 7
    req[6] = [called_orfs(ann, 6, genes0[offs0[6]:offs0[7]])[0]]
    ann.constrain(require=req)
    with pytest.raises(pa.PhxError) as e:
        ann.redrops()
    assert e.value.code == -13 and "required" in str(e.value)
    ann.constrain(forbid=req)  # nothing required: phx_constrain_flat serves too
    got = ann.redrops()
    assert got[0].tolist() == [-2, -3, 0, 0, 0, 0, 0]
    cst, coffs, cgenes = ann.constrain(forbid=req)[:3]
    assert check_contig(ann, EvRef(ann, 6), req[6], None, 0, got[2][got[1][6]:got[1][7]], cgenes[coffs[6]:coffs[7]])[1] >= 1
    ann.close()
    _solved.clear()


# ---- 8. isolation and the cache ----
def test_redrops_disturb_nothing_are_cached_and_invalidated(pa):
    a, b = fuzz(31, 20), fuzz(32, 20)

    def everything(ann, bias, forbid):
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()],
                [x.tobytes() for x in ann.replacements()], [x.tobytes() for x in evidence(ann, bias, forbid)], [x.tobytes() for x in ann.remargins()],
                [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n)])

    ann = pa.Annotator()
    run_batch(ann, a)
    bias, forbid = some_evidence(ann, 2908)
    before = everything(ann, bias, forbid)
    assert ann.redrops_ms() == dict(trees=0.0, candidates=0.0, fixups=0.0, download=0.0)
    r1 = out_bytes(ann.redrops())
    ms = ann.redrops_ms()
    assert ms["trees"] > 0 and ms["candidates"] > 0 and ms["fixups"] > 0
    assert out_bytes(ann.redrops()) == r1 and ann.redrops_ms() == ms  # the second call launches nothing
    assert everything(ann, bias, forbid) == before  # (the same re-annotation hits its cache ...)
    assert out_bytes(ann.redrops()) == r1 and ann.redrops_ms() == ms  # ... and keeps the drops
    other = pa.Annotator()  # the drops of the re-annotation first, everything else behind them
    run_batch(other, a)
    evidence(other, bias, forbid)
    assert out_bytes(other.redrops()) == r1 and everything(other, bias, forbid) == before
    # a different re-annotation invalidates them
    bias2, forbid2 = some_evidence(ann, 2909)
    evidence(ann, bias2, forbid2)
    evidence(other, bias2, forbid2)
    r2 = out_bytes(ann.redrops())
    assert r2 != r1 and r2 == out_bytes(other.redrops())
    other.close()
    # ... and so does the next run, whose own results are a fresh context's
    ann.upload(b)
    with pytest.raises(pa.PhxError) as e:
        ann.redrops()
    assert e.value.code == -13
    ann.run()
    with pytest.raises(pa.PhxError) as e:
        ann.redrops()
    assert e.value.code == -13
    fresh = pa.Annotator()
    run_batch(fresh, b)
    assert [x.tobytes() for x in ann.download_flat()] == [x.tobytes() for x in fresh.download_flat()]
    bias, forbid = some_evidence(fresh, 2910)
    evidence(ann, bias, forbid)
    evidence(fresh, bias, forbid)
    assert out_bytes(ann.redrops()) == out_bytes(fresh.redrops())
    for x in (ann, fresh):
        x.close()


def test_the_two_drop_sets_stay_apart_across_orders_and_batches(pa):
    """The run's drop set and the re-annotation's share one host pass (drop_pass) and must not share state.  One context, two batches (3
    contigs, then 20: both sets grow); per batch one evidence() call that solves contig 0 alone again, then rereplacements() first — it
    brings the re-annotation's set up with its trees and, through the contigs that were not solved again, the run's set without trees and
    then with the late tree launch —, then the other analyses.  Everything equals, byte for byte and counter for counter, what a fresh
    context gives in the plain order; the run's counters are the same before and after the re-annotation's pass."""

    def the_evidence(ann, st0, offs0, genes0):
        assert st0[0] == 0
        cg = called_orfs(ann, 0, genes0[offs0[0]:offs0[1]])
        k = next(k for k in range(len(ann.orfs(0))) if k not in cg)
        n = ann.n
        return [[(k, 1.5)]] + [None] * (n - 1), [[cg[len(cg) // 2]]] + [None] * (n - 1)

    def flat(out):
        return [x.tobytes() for x in out]

    ann = pa.Annotator()
    for seqs in (fuzz(41, 3), fuzz(42, 20)):
        bias, forbid = the_evidence(ann, *run_batch(ann, seqs))
        st = ann.evidence(bias, forbid)[0]
        rr = ann.rereplacements()  # the first analysis call after the solve
        got = dict(rr=flat(rr), rd=flat(ann.redrops()), rp=flat(ann.replacements()), dp=flat(ann.drop_margins()),
                   stats=(ann.drop_stats(), ann.redrop_stats(), ann.replacement_stats(), ann.rereplacement_stats()))
        offs = rr[1]
        assert st[0] == 0 and rr[0][0] == 0 and offs[1] > offs[0] and offs[-1] > offs[1]  # contig 0 solved again, the run's records beside it
        fresh = pa.Annotator()
        assert flat(run_batch(fresh, seqs)) == flat(ann.download_flat(exact=False))
        want = dict(dp=flat(fresh.drop_margins()), rp=flat(fresh.replacements()))
        run_stats = (fresh.drop_stats(), fresh.replacement_stats())
        fresh.evidence(bias, forbid)
        want.update(rd=flat(fresh.redrops()), rr=flat(fresh.rereplacements()))
        want["stats"] = (fresh.drop_stats(), fresh.redrop_stats(), fresh.replacement_stats(), fresh.rereplacement_stats())
        assert run_stats == (want["stats"][0], want["stats"][2])  # the re-annotation's pass left the run's counters alone
        for key in ("dp", "rp", "rd", "rr", "stats"):
            assert got[key] == want[key], (len(seqs), key)
        assert got["stats"][0]["slots"] > 0 and got["stats"][1]["slots"] > 0
        fresh.close()
    ann.close()


# ---- 9. batch size and create flags ----
def test_lone_contig_and_batch_of_300_give_the_same_bytes(pa):
    seqs = fuzz(23, 300)
    ann = pa.Annotator()
    run_batch(ann, seqs)
    only = set(range(2, 300, 37))
    bias, forbid = some_evidence(ann, 2911, only)
    evidence(ann, bias, forbid, solve_all=True)
    out = ann.redrops()
    got = {i: out_bytes(out, i) for i in only if bias[i] is not None}
    assert len(got) >= 5 and all(st == 0 and len(b) > 0 for st, b in got.values())
    for i, want in got.items():
        lone = pa.Annotator()
        run_batch(lone, [seqs[i]])
        evidence(lone, [bias[i]], [forbid[i]])
        assert out_bytes(lone.redrops(), 0) == want, i
        lone.close()
    ann.close()


def test_create_flags_give_the_same_bytes(pa):
    batches = ([pa.synth_contig(61, 14000), pa.synth_contig(62, 9000)], fuzz(5, 20))

    def outs(flags):
        ann = pa.Annotator(flags=flags)
        res = []
        for seqs in batches:
            run_batch(ann, seqs)
            bias, forbid = some_evidence(ann, 2912)
            evidence(ann, bias, forbid)
            res.append(out_bytes(ann.redrops()))
        ann.close()
        return res

    want = outs(())
    assert all(len(r[2]) > 0 for r in want)
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        assert outs((fl,)) == want, fl


# ---- 10. the CLI ----
def parse_drops_file(path):
    """{contig: rows} of a --drop-margins / --redrop-margins file (the rendering tests/test_drop_gpu.py::test_cli_drop_margins pins)."""
    blocks, cur = {}, None
    for ln in open(path).read().splitlines():
        if ln.startswith("#id:\t"):
            cur = blocks.setdefault(ln.split("\t", 1)[1], [])
        elif ln.startswith("#"):
            assert ln == "#START\tSTOP\tFRAME\tCONTIG\tSCORE\tDROP\tCALLED"
        else:
            cur.append(ln.split("\t"))
    return blocks


def test_cli_redrop_margins(pa, tmp_path):
    g, name, phix = load_golden("phiX174")
    fasta = tmp_path / "phix.fasta"
    fasta.write_text(">%s\n%s\n" % (name, phix))
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, [phix])
    orfs = ann.orfs(0)
    cds = [x for x in genes0 if abs(int(x["frame"])) <= 3]
    rows = []  # (ORF index, the line's first four columns)
    for k in [int(x) for x in np.random.RandomState(2913).choice(len(orfs), 4, replace=False)] + called_orfs(ann, 0, cds[:2]):
        o = orfs[k]
        a, z = (int(o["start"]), int(o["stop"]) + 2) if o["frame"] > 0 else (int(o["start"]) + 2, int(o["stop"]))
        rows.append((k, "%d\t%d\t%s\t%s" % (a, z, "+" if o["frame"] > 0 else "-", name)))
    vals = [-30.0, -2.5, 1.25, -8.0, 4.0]
    ev, fb, out, df = tmp_path / "ev.txt", tmp_path / "fb.txt", tmp_path / "out.txt", tmp_path / "rd.txt"
    ev.write_text("".join("%s\t%r\n" % (ln, b) for (k, ln), b in zip(rows, vals)))
    fb.write_text(rows[5][1] + "\n")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta), "--evidence", str(ev), "--forbid", str(fb), "--reannotation", str(out), "--redrop-margins", str(df)],
                         capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    ann.evidence([[(k, b) for (k, ln), b in zip(rows, vals)]], [[rows[5][0]]])
    st, offs, rec = ann.redrops()
    assert st.tolist() == [0] and len(rec) > 3
    want = [[str(x["right"] if x["strand"] < 0 else x["left"]), str(x["left"] if x["strand"] < 0 else x["right"]), "+" if x["strand"] > 0 else "-", name,
             "%E" % float(x["score"]), "%E" % float(x["drop"]), str(int(x["called"]))] for x in rec]
    blocks = parse_drops_file(str(df))
    assert list(blocks) == [name] and blocks[name] == want
    ann.close()
