"""Pinned drop margins on the device (phx_pindrops_flat, Annotator.pindrops) against python integers.  The yardstick is the
equivalence of §32 through CuRef.solve (tests/test_curate_gpu.py), once per called gene: with grp the ORFs of the gene's stop group,
(S1, c1) = solve(F, R, B) and (S2, c2) = solve(F + grp, R - grp, B) give lost = c1 - c2 and drop = float(S2 - S1) / 1000.0; no path in the
second solve: bypass = 0, drop = +inf, lost = 0.  Every field of every record and every `lost` is compared, and every test that reaches
the yardstick asserts at least one compared record per pinned contig."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_constrain_gpu import bytes_of, fuzz, run_batch, wide_cases
from test_curate_gpu import Batch, CuRef, DeviceGraph, NoGraph, curate, evidence, sets_of

import curate_draws as cd

pytestmark = pytest.mark.gpu

E_STATE, S_NEGCYCLE, S_NOPATH = -13, -9, 1


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


@pytest.fixture(scope="module")
def small(pa):
    """curate_draws.mix_seqs, run once (the batch of tests/test_pinmargins_gpu.py): one contig of 179 nodes, eight of 272-1004.  The tests
    leave the batch resident."""
    ann = pa.Annotator()
    b = Batch(ann, cd.mix_seqs(pa))
    V = sorted(int(ann.globals(i).n_node) for i in b.idx)
    print("nodes per contig:", V)
    assert len(b.idx) >= 8 and V[0] <= 256 and V[-1] > 768
    yield b
    ann.close()


# ---- the yardstick ----
def solve(ref, forbid, require, bias):
    """ref.solve, once per (refused, required, biased) triple of a yardstick; a solve handed out is never changed."""
    memo = ref.__dict__.setdefault("_pd_memo", {})
    key = (tuple(sorted(forbid or ())), tuple(sorted(require or ())), tuple(sorted((bias or {}).items())))
    if key not in memo:
        memo[key] = ref.solve(key[0], key[1], dict(key[2]) or None)
    return memo[key]


def rec_of(out, i):
    st, offs, rec, lost = out
    return int(st[i]), rec[offs[i]:offs[i + 1]], lost[offs[i]:offs[i + 1]]


def out_bytes(out, i=None):
    if i is None:
        return [x.tobytes() for x in out]
    st, rec, lost = rec_of(out, i)
    return st, rec.tobytes(), lost.tobytes()


def check_contig(ann, ref, forbid, require, bias, st, rec, lost, genes, limit=None):
    """One contig's records and `lost` against the yardstick.  "cycle", None (no path) or dict(records: those compared, gave_up: records
    with lost > 0, cheaper: of those with drop < 0, by_orf: {ORF index: (lost, drop)}).  limit: on a contig whose solve takes seconds in
    python, only the records of the required ORFs and the first `limit` others get their second solve; the rest are held to the
    path, field by field."""
    i = ref.i
    what = (i, list(forbid or ()), list(require or ()), bias)
    sol = solve(ref, forbid, require, bias)
    assert len(rec) == len(lost), what
    if sol["cycle"]:
        assert st == S_NEGCYCLE and len(rec) == 0, (what, st)
        return "cycle"
    if sol["S"] is None:
        assert st == S_NOPATH and len(rec) == 0, (what, st)
        return None
    assert st == 0, (what, st)
    path = sol["path"]
    assert ann.reannotated_path(i)[0].tolist() == path, what
    orfs = ref.orfs
    returned = {(int(g["left"]), int(g["right"]), int(g["strand"])) for g in genes if abs(int(g["frame"])) <= 3}
    out = dict(records=0, gave_up=0, cheaper=0, by_orf={})
    n = others = 0
    for k in range((len(path) - 1) // 2):  # the pairs of P', in path order
        a, z = path[2 * k + 1], path[2 * k + 2]
        left, right, fr = ref.pos[a], ref.pos[z] + 2, ref.frame[a]
        if abs(fr) > 3:
            continue  # (a tRNA pair gets no record)
        strand = -1 if fr < 0 else 1
        o = ref.by_ends[(left, right, strand)]
        assert n < len(rec), (what, k, len(rec))
        r, lo = rec[n], int(lost[n])
        n += 1
        assert (int(r["left"]), int(r["right"]), int(r["strand"]), int(r["frame"])) == (left, right, strand, fr), (what, k)
        assert float(r["score"]) == ref.weight[(left, right, strand)], (what, k)
        assert int(r["called"]) == (1 if (left, right, strand) in returned else 0) == 1, (what, k)
        out["by_orf"][o] = (lo, float(r["drop"]))
        if limit is not None and o not in (require or ()):
            others += 1
            if others > limit:
                continue
        grp = set(np.nonzero(orfs["group"] == orfs["group"][o])[0].tolist())
        assert o in grp
        without = solve(ref, set(forbid or ()) | grp, [x for x in (require or ()) if x not in grp], bias)
        assert not without["cycle"], (what, k)  # (taking edges away makes no cycle negative)
        if without["S"] is None:
            assert r["bypass"] == 0 and r["drop"] == np.inf and lo == 0, (what, k, float(r["drop"]), lo)
        else:
            want = (sol["count"] - without["count"], without["S"] - sol["S"])
            assert want >= (0, 0), (what, k, want)
            assert r["bypass"] == 1 and lo == want[0] and float(r["drop"]) == float(want[1]) / 1000.0, (what, k, lo, float(r["drop"]), want)
            out["gave_up"] += lo > 0
            out["cheaper"] += lo > 0 and want[1] < 0
        out["records"] += 1
    assert n == len(rec), (what, n, len(rec))
    return out


def pin_drop_batch(b, bias, forbid, require, solve_all=False, limit=None):
    """curate(), pindrops(), every contig with a required ORF against the yardstick: ({contig: check_contig's result}, the two results).
    No pinned contig with a path passes without a compared record.  (limit: check_contig's.)"""
    ann = b.ann
    res = curate(ann, bias, forbid, require, solve_all)
    st, offs, genes, delta, unmet = res
    pd = ann.pindrops()
    out = {}
    for i in b.idx:
        if not (require and require[i]):
            continue
        dst, rec, lost = rec_of(pd, i)
        out[i] = check_contig(ann, b.refs[i], forbid and forbid[i], require[i], bias and bias[i], dst, rec, lost, genes[offs[i]:offs[i + 1]], limit)
        assert dst == int(st[i]), i
        assert out[i] in ("cycle", None) or out[i]["records"] >= 1, i
    return out, res, pd


def with_path(sols):
    return [s for s in sols.values() if s not in ("cycle", None)]


# ---- 1. the seeded mixes ----
@pytest.mark.parametrize("rnd", range(cd.ROUNDS))
def test_the_seeded_mixes_against_the_yardstick(small, rnd):
    b = small
    graphs = [DeviceGraph(b.refs[i], b.called[i]) if i in b.refs else NoGraph() for i in range(b.n)]
    row = cd.mixes(graphs)[rnd]
    forbid, require, bias = [None] * b.n, [None] * b.n, [None] * b.n
    for i, d in enumerate(row):
        if d is not None:
            by = b.refs[i].by_ends
            forbid[i], require[i], bias[i] = [by[k] for k in d["forbid"]], [by[k] for k in d["require"]], {by[k]: B for k, B in d["bias"].items()}
    sols, res, pd = pin_drop_batch(b, bias, forbid, require)
    ok = with_path(sols)
    print("round %d: %d draws, %d settle with a path; %d records, %d give up a pin, %d of them with a negative drop"
          % (rnd, len(sols), len(ok), sum(s["records"] for s in ok), sum(s["gave_up"] for s in ok), sum(s["cheaper"] for s in ok)))
    assert len(sols) == sum(d is not None and bool(d["require"]) for d in row) and len(ok) >= 8
    assert sum(s["records"] for s in ok) >= 50 and sum(s["gave_up"] for s in ok) > 0


# ---- 2. constrain() alone and curate() ----
def test_constrain_alone_against_the_yardstick(small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 3210)
    assert sum(r is not None for r in require) >= 6
    res = ann.constrain(forbid, require)  # mode 2
    pd = ann.pindrops()
    run = ann.drop_margins()
    seen = 0
    for i in range(b.n):
        dst, rec, lost = rec_of(pd, i)
        if i in b.refs and require[i]:
            sol = check_contig(ann, b.refs[i], forbid[i], require[i], None, dst, rec, lost, res[2][res[1][i]:res[1][i + 1]])
            seen += sol not in ("cycle", None) and sol["records"] >= 1
        else:  # the run's result stands: drop_margins()' records, lost 0
            assert (dst, rec.tobytes()) == (int(run[0][i]), run[2][run[1][i]:run[1][i + 1]].tobytes()) and not lost.any(), i
    assert seen >= 5


def test_curate_against_the_yardstick(small):
    b = small
    forbid, require, bias = sets_of(b, 3210)
    sols, _, _ = pin_drop_batch(b, bias, forbid, require)  # mode 4
    assert len(with_path(sols)) >= 5


# ---- 3. a required called gene; a required uncalled ORF that displaces a call ----
def test_a_required_called_gene_loses_itself(small):
    b, ann = small, small.ann
    require = b.per_contig(lambda i: [b.called[i][len(b.called[i]) // 2]] if b.called[i] else None)
    sols, res, pd = pin_drop_batch(b, None, None, require)
    seen = 0
    for i, s in sols.items():
        assert s not in ("cycle", None) and res[4][i] == 0, i  # a called gene is kept
        lo, drop = s["by_orf"][require[i][0]]
        assert lo == 1 or (lo == 0 and drop == np.inf), (i, lo, drop)  # the only pin goes with its stop
        seen += lo == 1
        assert all(x[0] in (0, 1) for x in s["by_orf"].values()), i
    assert seen >= 6


def test_a_required_uncalled_orf_that_displaces_a_call(small):
    b, ann = small, small.ann
    rec0 = {i: b.rec(i) for i in b.idx}
    # the reachable uncalled ORF with the largest margin: the path has to give something up for it
    require = b.per_contig(lambda i: [max(b.reachable(i), key=lambda k: (float(rec0[i]["margin"][k]) if np.isfinite(rec0[i]["margin"][k]) else -1.0, k))] if b.reachable(i) else None)
    sols, res, pd = pin_drop_batch(b, None, None, require)
    st, offs, genes, delta, unmet = res
    moved = seen = 0
    for i, s in sols.items():
        if s in ("cycle", None) or unmet[i] != 0:
            continue
        called = b.refs[i].called(genes[offs[i]:offs[i + 1]])
        assert require[i][0] in called
        moved += any(k not in called for k in b.called[i])  # a gene of the run is no longer called
        lo, drop = s["by_orf"][require[i][0]]
        assert lo == 1 or (lo == 0 and drop == np.inf), (i, lo, drop)
        seen += 1
    assert seen >= 6 and moved >= 4, (seen, moved)


# ---- 4. two required starts of one stop group ----
def test_two_required_starts_of_one_stop_group(small):
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
    sols, res, pd = pin_drop_batch(b, None, None, require)
    st, offs, genes, delta, unmet = [x.copy() for x in res]
    pd = [x.copy() for x in pd]
    kept_only, own = [None] * b.n, {}
    seen = 0
    for i, s in sols.items():
        if s in ("cycle", None):
            continue
        called = b.refs[i].called(genes[offs[i]:offs[i + 1]])
        kept = [k for k in pairs[i] if k in called]
        assert unmet[i] == 1 and len(kept) == 1  # a path takes one start per stop
        lo, drop = s["by_orf"][kept[0]]
        assert lo == 1 or (lo == 0 and drop == np.inf), (i, lo, drop)  # dropping the stop loses the kept one, and only it
        kept_only[i], own[i] = kept, (lo, drop)
        seen += 1
    assert seen >= 5
    # the unmet one changes nothing there: the stop's record is the same without it (both starts go with the stop either way)
    sols2, _, _ = pin_drop_batch(b, None, None, kept_only, limit=0)
    for i in own:
        assert sols2[i]["by_orf"][kept_only[i][0]] == own[i], i


# ---- 5. a batch of every mode and both reductions ----
def test_a_batch_of_every_mode_and_both_reductions(pa, small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 3211)
    full = [i for i in b.idx if require[i]]
    assert len(full) >= 6
    role = {full[0]: 0, full[1]: 1, full[2]: 2, full[3]: 3}  # the run's result, refused only, required only, biased only; the others all three
    F = [forbid[i] if role.get(i, 4) in (1, 4) and i in full else None for i in range(b.n)]
    R = [require[i] if role.get(i, 4) in (2, 4) and i in full else None for i in range(b.n)]
    Bs = [bias[i] if role.get(i, 4) in (3, 4) and i in full else None for i in range(b.n)]
    sols, res, pd = pin_drop_batch(b, Bs, F, R)
    assert sorted(sols) == sorted(i for i in full if role.get(i, 4) in (2, 4)) and len(with_path(sols)) >= 3
    pd = [x.copy() for x in pd]
    run = ann.drop_margins()
    # second reduction: a contig of mode 1 or 3 has what redrops() gives once every required list is emptied, one of mode 0 drop_margins()' records
    curate(ann, Bs, F, None)
    want = ann.redrops()
    for i in range(b.n):
        if not R[i]:
            dst, rec, lost = rec_of(pd, i)
            assert (dst, rec.tobytes()) == (int(want[0][i]), want[2][want[1][i]:want[1][i + 1]].tobytes()), (i, role.get(i))
            assert not lost.any()
            if not F[i] and not Bs[i]:
                assert (dst, rec.tobytes()) == (int(run[0][i]), run[2][run[1][i]:run[1][i + 1]].tobytes()), i
    assert any(want[2][want[1][i]:want[1][i + 1]].tobytes() != run[2][run[1][i]:run[1][i + 1]].tobytes() for i in (full[1], full[3]))  # (the refused / biased contigs differ from the run)
    # first reduction: no contig pinned — redrops()' three arrays byte for byte, lost all 0
    got = ann.pindrops()
    assert out_bytes(got[:3]) == out_bytes(want) and len(got[3]) == len(want[2]) and not got[3].any()
    assert ann.pindrop_stats() == ann.redrop_stats() and ann.pindrops_ms() == ann.redrops_ms()
    # ... and after a solve that pinned a contig redrops() and rereplacements() keep refusing, with their message
    curate(ann, Bs, F, R)
    for call in (ann.redrops, ann.rereplacements):
        with pytest.raises(pa.PhxError) as e:
            call()
        assert e.value.code == E_STATE and "required" in str(e.value)
    assert [out_bytes(ann.pindrops(), i) for i in range(b.n)] == [out_bytes(pd, i) for i in range(b.n)]


def test_nothing_required_under_solve_all_is_redrops(small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 3212)
    curate(ann, bias, forbid, None, solve_all=True)
    got = ann.pindrops()
    want = ann.redrops()
    assert out_bytes(got[:3]) == out_bytes(want) and len(got[2]) > 50 and not got[3].any()
    assert ann.pindrop_stats() == ann.redrop_stats()
    ann.curate(None, None, None, solve_all=True)  # ... and on the unchanged graph
    got = ann.pindrops()
    assert out_bytes(got[:3]) == out_bytes(ann.redrops()) and not got[3].any() and ann.pindrop_stats() == ann.redrop_stats() == ann.drop_stats()


# ---- 6. the cross-node batch: step 4 and the rescan in the new instantiations ----
def test_the_cross_node_batch_with_one_orf_required_per_contig(pa):
    """tests/test_drop_gpu.py's cross-node batch, a called gene required on every contig: its own slot has lost = 1, so the rescan runs on
    every pinned contig, and the cross nodes are the run's.  The small contigs go against the python yardstick; every record of every
    contig goes against the definition through the device's own solver — for record r of all contigs at once one
    constrain(F + grp, R - grp) —, exact in integers: delta = float(S - D) / 1000.0 gives S - D back where it is below 2^50."""
    ann = pa.Annotator()
    seqs = fuzz(101, 150)
    st0, offs0, genes0 = run_batch(ann, seqs)
    n = ann.n
    mst = ann.margins()[0]
    idx = [i for i in range(n) if st0[i] == 0 and int(ann.globals(i).n_node) > 2 and mst[i] == 0]
    called, orfs = {}, {}
    for i in idx:
        cds = [g for g in genes0[offs0[i]:offs0[i + 1]] if abs(int(g["frame"])) <= 3]
        called[i] = [ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds]
        orfs[i] = ann.orfs(i)
    require = [[called[i][len(called[i]) // 2]] if i in called and called[i] else None for i in range(n)]
    st, offs, genes, delta, unmet = [x.copy() for x in ann.constrain(None, require)]
    pinned = [i for i in range(n) if require[i] and st[i] == 0 and unmet[i] == 0]  # (a gene on a cycle the source reaches: PHX_S_NEGCYCLE, no records)
    assert len(pinned) >= 100
    pd = [x.copy() for x in ann.pindrops()]
    stats = ann.pindrop_stats()
    print("cross-node batch under pins:", stats, "the run's:", ann.drop_stats())
    assert stats["slots"] == len(pd[2]) and stats["cross"] > 0
    assert all(pd[0][i] == st[i] and (st[i] == 0 or pd[1][i + 1] == pd[1][i]) for i in range(n) if require[i])
    # the python yardstick on the small contigs
    seen = 0
    for i in sorted(pinned, key=lambda i: int(ann.globals(i).n_node))[:12]:
        dst, rec, lost = rec_of(pd, i)
        s = check_contig(ann, CuRef(ann, i), None, require[i], None, dst, rec, lost, genes[offs[i]:offs[i + 1]])
        assert s not in ("cycle", None) and s["records"] >= 1
        seen += s["records"]
    assert seen >= 12
    # every record through the device's own solver
    exact = lambda d: int(round(float(d) * 1000.0))
    nrec = {i: int(pd[1][i + 1] - pd[1][i]) for i in pinned}
    compared = skipped = gave_up = 0
    for r in range(max(nrec.values())):
        F, R, who = [None] * n, [None] * n, []
        for i in pinned:
            if r >= nrec[i]:
                continue
            x = pd[2][pd[1][i] + r]
            o = ann.orf_index(i, int(x["left"]), int(x["right"]), int(x["strand"]))
            grp = np.nonzero(orfs[i]["group"] == orfs[i]["group"][o])[0].tolist()
            F[i], R[i] = grp, [k for k in require[i] if k not in grp]
            who.append(i)
        st2, offs2, genes2, delta2, unmet2 = ann.constrain(F, R)
        for i in who:
            x, lo = pd[2][pd[1][i] + r], int(pd[3][pd[1][i] + r])
            if st2[i] == S_NOPATH:
                assert x["bypass"] == 0 and x["drop"] == np.inf and lo == 0, (i, r)
                continue
            assert st2[i] == 0 and x["bypass"] == 1, (i, r, int(st2[i]))
            assert lo == (1 - int(unmet[i])) - (len(R[i]) - int(unmet2[i])), (i, r, lo)
            gave_up += lo > 0
            if max(abs(float(delta[i])), abs(float(delta2[i]))) * 1000.0 >= 2.0 ** 50:
                skipped += 1
                continue
            assert float(x["drop"]) == float(exact(delta2[i]) - exact(delta[i])) / 1000.0, (i, r, float(x["drop"]), float(delta2[i]), float(delta[i]))
            compared += 1
    print("cross-node batch: %d records compared through the solver, %d beyond 2^50, %d give up the pin" % (compared, skipped, gave_up))
    assert compared >= 1000 and skipped * 20 <= compared and stats["rescanned"] >= gave_up >= len(pinned) // 2
    ann.close()


# ---- 7. the layered rebuild, in a fresh process ----
LAYERED_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import phanotate_amd as pa
import curate_draws as cd
ann = pa.Annotator()
ann.upload(cd.mix_seqs(pa))
ann.run()
req = json.loads(sys.argv[2])
ann.constrain(None, req)
out = [x.tobytes().hex() for x in ann.pindrops()]
print(json.dumps({"out": out, "stats": ann.pindrop_stats()}))
"""


def test_layered_trees_give_the_same_records(small):
    b, ann = small, small.ann
    require = b.per_contig(lambda i: b.reachable(i)[len(b.reachable(i)) // 3:][:1] or None)
    sols, res, pd = pin_drop_batch(b, None, None, require)
    assert len(with_path(sols)) >= 6
    here = ann.pindrop_stats()
    r = subprocess.run([sys.executable, "-c", LAYERED_CHILD, ROOT, json.dumps(require)], capture_output=True, text=True, timeout=600, env=dict(os.environ, PHX_DROP_LAYERED="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    assert child["out"] == [x.tobytes().hex() for x in pd]
    covered = sum(int(pd[1][i + 1] - pd[1][i]) > 0 for i in sols)
    assert child["stats"]["layered"] == covered > here["layered"] and child["stats"]["slots"] == here["slots"] > 0


# ---- 8. the wide classes ----
@pytest.mark.parametrize("case", range(4))
def test_the_wide_classes(pa, case):
    seqs = wide_cases(pa)[case][0]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    want = (4, 8, 8, 17)[case]  # 320, 576 twice and 1152 bits under MgPinDrop
    c = next(i for i in range(len(seqs)) if st0[i] == 0 and int(ann.globals(i).n_limbs) == want)
    mst, moffs, mrec = ann.margins()
    assert mst[c] == 0
    run = ann.drop_margins()
    ref = CuRef(ann, c)
    rec = mrec[moffs[c]:moffs[c + 1]]
    pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0]
    long_one = int(pool[np.argmax(ref.orfs["length"][pool])])  # the widest ORF weights sit in the long ORF's group
    rng = np.random.RandomState(3230 + case)
    other = int(pool[rng.randint(len(pool))])
    cg = ref.called(genes0[offs0[c]:offs0[c + 1]])
    seen = 0
    for req, bias in (([long_one], {other: -2500, cg[0]: 4000}), ([cg[len(cg) // 2]], None)):
        require, bb = [None] * len(seqs), [None] * len(seqs)
        require[c], bb[c] = req, bias
        st, offs, genes, delta, unmet = curate(ann, bb, None, require)
        pd = ann.pindrops()
        dst, prec, lost = rec_of(pd, c)
        sol = check_contig(ann, ref, None, req, bias, dst, prec, lost, genes[offs[c]:offs[c + 1]], limit=2)  # (a solve of these contigs takes seconds)
        seen += sol not in ("cycle", None) and sol["records"] >= 1
        for j in range(len(seqs)):  # neighbours keep the run's records
            if j != c:
                assert out_bytes(pd, j)[:2] == (int(run[0][j]), run[2][run[1][j]:run[1][j + 1]].tobytes()) and not rec_of(pd, j)[2].any()
    ann.close()
    assert seen >= 1


# ---- 9. statuses ----
def test_a_negative_cycle_and_no_path_have_no_records(pa):
    from phanotate_amd.fasta import read_fasta

    seqs = [seq for name, seq in read_fasta(os.path.join(ROOT, "tests", "golden", "constrain_cycle.fasta"))]
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops  # no path: what lies behind the first stops is out of the source's reach
    seqs = seqs + [pa.synth_contig(61, 9000), unreachable]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    assert st0.tolist() == [0, 0, 0, 1]
    with pytest.raises(pa.PhxError) as e:  # before any re-annotation of the run
        ann.pindrops()
    assert e.value.code == E_STATE and "no re-annotation" in str(e.value)
    refs = {i: CuRef(ann, i) for i in range(4)}
    cyc = {i: [k for k, e in enumerate(refs[i].orf_edge) if e is not None and refs[i].on_cycle({e})] for i in (0, 1)}
    free = [k for k, e in enumerate(refs[2].orf_edge) if e is not None][:2]
    quiet = [k for k, e in enumerate(refs[3].orf_edge) if e is None or not refs[3].on_cycle({e})]
    require = [[cyc[0][0]], [cyc[1][-1]], free, quiet[:1]]
    st, offs, genes, delta, unmet = ann.constrain(None, require)
    assert st.tolist()[:2] == [S_NEGCYCLE, S_NEGCYCLE] and st[3] == S_NOPATH
    pd = ann.pindrops()
    assert pd[0].tolist() == st.tolist()
    assert np.diff(pd[1]).tolist()[:2] == [0, 0] and pd[1][4] == pd[1][3]  # PHX_S_NEGCYCLE, PHX_S_NOPATH: no records
    s = check_contig(ann, refs[2], None, require[2], None, *rec_of(pd, 2), genes[offs[2]:offs[3]])
    assert s not in ("cycle", None) and s["records"] >= 1
    assert check_contig(ann, refs[3], None, require[3], None, *rec_of(pd, 3), genes[offs[3]:offs[4]]) is None
    ann.close()


# ---- 10. side effects, the cache, its invalidation ----
def test_pindrops_disturb_nothing_are_cached_and_invalidated(pa):
    a, nxt = fuzz(31, 12), fuzz(32, 12)
    ann = pa.Annotator()
    b = Batch(ann, a)

    def everything():
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()],
                [x.tobytes() for x in ann.replacements()], [ann.path(i)[0].tobytes() for i in range(ann.n)], ann.drop_stats())

    forbid, require, bias = sets_of(b, 3240)
    assert sum(r is not None for r in require) >= 5
    # the re-annotation's own drop state, from a solve without required ORFs
    evidence(ann, bias, forbid)
    rd0 = [x.tobytes() for x in ann.redrops()]
    rd_stats = ann.redrop_stats()
    before = everything()
    r0 = bytes_of(curate(ann, bias, forbid, require))
    pm0 = bytes_of(ann.pinmargins())
    pm_ms = ann.pinmargins_ms()
    p1 = out_bytes(ann.pindrops())
    ms = ann.pindrops_ms()
    assert ms["trees"] > 0 and ms["candidates"] > 0 and ms["fixups"] > 0
    assert out_bytes(ann.pindrops()) == p1 and ann.pindrops_ms() == ms  # the second call launches nothing
    assert everything() == before  # the run's drops, replacements and counters are as they were
    assert bytes_of(ann.pinmargins()) == pm0 and ann.pinmargins_ms() == pm_ms
    assert bytes_of(curate(ann, bias, forbid, require)) == r0  # (the same re-annotation hits its cache ...)
    assert out_bytes(ann.pindrops()) == p1 and ann.pindrops_ms() == ms  # ... and keeps the drops
    for call in (ann.redrops, ann.rereplacements):  # still PHX_E_STATE after a pinned solve
        with pytest.raises(pa.PhxError) as e:
            call()
        assert e.value.code == E_STATE and "required" in str(e.value)
    other = pa.Annotator()  # the pinned drops first, everything else behind them
    run_batch(other, a)
    curate(other, bias, forbid, require)
    assert out_bytes(other.pindrops()) == p1 and bytes_of(other.pinmargins()) == pm0 and [x.tobytes() for x in other.drop_margins()] == before[2]
    other.close()
    # a different solve invalidates them
    ann.constrain(forbid, require)
    p2 = out_bytes(ann.pindrops())
    assert p2 != p1
    curate(ann, bias, forbid, require)
    assert out_bytes(ann.pindrops()) == p1
    # redrops() of the solve without required ORFs is what it was
    evidence(ann, bias, forbid)
    assert [x.tobytes() for x in ann.redrops()] == rd0 and ann.redrop_stats() == rd_stats
    # ... and the next batch invalidates them too
    ann.upload(nxt)
    with pytest.raises(pa.PhxError) as e:
        ann.pindrops()
    assert e.value.code == E_STATE
    ann.run()
    with pytest.raises(pa.PhxError) as e:
        ann.pindrops()
    assert e.value.code == E_STATE
    ann.curate(None, None, None)
    got = ann.pindrops()
    assert out_bytes(got[:3]) == [x.tobytes() for x in ann.drop_margins()] and not got[3].any()
    ann.close()


# ---- 11. batch size and create flags ----
def reachable_of(ann, i, mrec, moffs):
    rec = mrec[moffs[i]:moffs[i + 1]]
    return sorted(np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0].tolist(), key=lambda k: (int(rec["left"][k]), int(rec["right"][k]), int(rec["strand"][k])))


def some_pins(ann, seed, only=None):
    """Per solved contig (of `only`) a reachable uncalled ORF to require and another to give a bonus."""
    st0 = ann.download_flat(exact=False)[0]
    mst, moffs, mrec = ann.margins()
    rng = np.random.RandomState(seed)
    require, bias = [None] * ann.n, [None] * ann.n
    for i in range(ann.n):
        if st0[i] != 0 or mst[i] != 0 or (only is not None and i not in only):
            continue
        pool = reachable_of(ann, i, mrec, moffs)
        if len(pool) < 2:
            continue
        a = int(rng.randint(len(pool) - 1))
        require[i], bias[i] = [pool[a]], {pool[a + 1]: -int(rng.randint(1, 30000))}
    return require, bias


def test_lone_contig_and_batch_of_300_give_the_same_bytes(pa):
    seqs = fuzz(23, 300)
    ann = pa.Annotator()
    run_batch(ann, seqs)
    only = set(range(2, 300, 37))
    require, bias = some_pins(ann, 3250, only)
    curate(ann, bias, None, require)
    out = ann.pindrops()
    got = {i: out_bytes(out, i) for i in only if require[i] is not None}
    assert len(got) >= 5 and sum(st == 0 and len(r) > 0 for st, r, lo in got.values()) >= 5
    for i, want in got.items():
        lone = pa.Annotator()
        run_batch(lone, [seqs[i]])
        curate(lone, [bias[i]], None, [require[i]])
        assert out_bytes(lone.pindrops(), 0) == want, i
        lone.close()
    ann.close()


def test_create_flags_give_the_same_bytes(pa):
    batches = ([pa.synth_contig(61, 14000), pa.synth_contig(62, 9000)], fuzz(5, 20))

    def outs(flags):
        ann = pa.Annotator(flags=flags)
        res = []
        for seqs in batches:
            run_batch(ann, seqs)
            require, bias = some_pins(ann, 3251)
            curate(ann, bias, None, require)
            res.append(out_bytes(ann.pindrops()))
        ann.close()
        return res

    want = outs(())
    assert all(len(r[2]) > 0 for r in want)
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        assert outs((fl,)) == want, fl


# ---- 12. the CLI ----
def test_cli_pin_drop_margins(pa, tmp_path):
    from phanotate_amd.cli import format_pin_drops

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
        require[i] = [pool[len(pool) // 3], b.called[i][0]]
        forbid[i] = [b.called[i][1]]
        rq_lines += [line(k) for k in require[i]]
        fb_lines += [line(k) for k in forbid[i]]
    rq, fb, out, pf = tmp_path / "rq.txt", tmp_path / "fb.txt", tmp_path / "out.txt", tmp_path / "pd.txt"
    rq.write_text("\n".join(rq_lines) + "\n")
    fb.write_text("\n".join(fb_lines) + "\n")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta), "--require", str(rq), "--forbid", str(fb), "--reannotation", str(out), "--pin-drop-margins", str(pf)],
                         capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    res = ann.constrain(forbid, require)
    pd = st, offs, rec, lost = ann.pindrops()
    assert st.tolist() == [0, 0]
    for i in (0, 1):
        s = check_contig(ann, b.refs[i], forbid[i], require[i], None, *rec_of(pd, i), res[2][res[1][i]:res[1][i + 1]])
        assert s not in ("cycle", None) and s["records"] >= 1
    text = open(pf, "rb").read()
    assert text == format_pin_drops(list(seqs), st, offs, rec, lost)
    rows = [ln.split("\t") for ln in text.decode().splitlines() if not ln.startswith("#")]
    assert len(rows) == len(rec) and all(len(r) == 8 for r in rows)
    assert sum(int(r[6]) > 0 for r in rows) == int((lost > 0).sum()) > 0
    ann.close()
