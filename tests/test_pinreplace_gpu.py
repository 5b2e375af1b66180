"""Pinned replacements on the device (phx_pinreplacements_flat, phx_tap_pinreplacement) against python integers.  Every
record is held bit for bit against pindrops() — which tests/test_pindrops_gpu.py holds against curate() —, and every witness is weighed
from the one edge list of G' that the yardstick (CuRef of tests/test_curate_gpu.py) solves on: an edge that is not in it fails the test,
the required ORF edges on the witness number c(P') - lost, and float(S(R') - S(P')) / 1000 is the record's drop.  Properties 1, 3 and 4 are
checked as tests/test_replace_gpu.py::check_contig checks them, on P' = reannotated_path(i).  A bounded sample per contig is also held
exactly against one CuRef solve of curate(B, F + grp, R - grp); every test that reaches the yardstick asserts at least one such record per
pinned contig that has a path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_constrain_gpu import bytes_of, fuzz, run_batch, wide_cases
from test_curate_gpu import Batch, CuRef, DeviceGraph, NoGraph, curate, evidence, sets_of
from test_pindrops_gpu import rec_of, solve, some_pins
from test_replace_gpu import pair_gene, pairs
from test_rereplace_gpu import CROSS_SEEDS, contig_bytes

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
    assert len(b.idx) >= 8 and V[0] <= 256 and V[-1] > 768
    yield b
    ann.close()


# ---- the yardstick ----
def graph_of(ref, forbid, require, bias):
    """G' as CuRef.solve builds it from its one edge list: ({(u, v): W + B} without the refused ORF edges, the required ORF edges)."""
    gone = {ref.orf_edge[k] for k in forbid or ()} - {None}
    req = {ref.orf_edge[k] for k in require or ()} - {None} - gone
    add = {}
    for k, B in (bias or {}).items():
        if ref.orf_edge[k] is not None:
            add[ref.orf_edge[k]] = add.get(ref.orf_edge[k], 0) + B
    W = {(u, v): w + add.get((u, v), 0) for u, v, w in ref.edges if (u, v) not in gone}
    assert len(W) == sum((u, v) not in gone for u, v, _ in ref.edges)
    return W, req


def out_of(out, i):
    """Contig i of pinreplacements(): (status, records, lost)."""
    st, offs, rec, genes, lost = out
    return int(st[i]), rec[offs[i]:offs[i + 1]], lost[offs[i]:offs[i + 1]]


def pin_bytes(out, i):
    """contig_bytes of tests/test_rereplace_gpu.py with the contig's `lost`."""
    return contig_bytes(out[:4], i) + (out_of(out, i)[2].tobytes(),)


def all_bytes(out):
    return [x.tobytes() for x in out]


def check_records(ann, ref, forbid, require, bias, pd_i, pr_i, genes, limit=None):
    """One pinned contig.  pd_i / pr_i: (status, records, lost) of pindrops() / pinreplacements().  "cycle", None (no path) or dict(exact:
    bypass records also held against their own solve, bypass, gave_up: bypass records with lost > 0, cheaper: of those with drop < 0,
    by_orf: {ORF index: (lost, required edges on the witness)}).  limit: at most that many records beside those of the required ORFs
    get their own solve; every record is weighed."""
    i = ref.i
    what = (i, list(forbid or ()), list(require or ()), bias)
    (dst, drec, dlost), (rst, rrec, rlost) = pd_i, pr_i
    assert rst == dst and len(rrec) == len(drec) == len(rlost) == len(dlost), what
    for f in ("left", "right", "strand", "frame", "called", "bypass"):
        assert (rrec[f] == drec[f]).all(), (what, f)
    assert rrec["drop"].tobytes() == drec["drop"].tobytes() and rlost.tobytes() == dlost.tobytes(), what
    sol = solve(ref, forbid, require, bias)
    if sol["cycle"]:
        assert rst == S_NEGCYCLE and len(rrec) == 0, (what, rst)
        return "cycle"
    if sol["S"] is None:
        assert rst == S_NOPATH and len(rrec) == 0, (what, rst)
        return None
    assert rst == 0, (what, rst)
    P, S, cP = sol["path"], sol["S"], sol["count"]
    assert ann.reannotated_path(i)[0].tolist() == P, what
    W, req = graph_of(ref, forbid, require, bias)
    assert cP == sum(e in req for e in zip(P, P[1:])) and S == sum(W[e] for e in zip(P, P[1:])), what
    pidx = {v: t for t, v in enumerate(P)}
    V, nd, orfs = ref.V, ref.nd, ref.orfs
    pg = []  # the CDS genes of P' in path order: (left, right, strand, frame, stop node)
    for k in range((len(P) - 1) // 2):
        a, b = P[2 * k + 1], P[2 * k + 2]
        fa = int(nd["frame"][a])
        if abs(fa) <= 3:
            pg.append(pair_gene(nd, a, b) + (b if fa > 0 else a,))
    assert [(int(r["left"]), int(r["right"]), int(r["strand"]), int(r["frame"])) for r in rrec] == [g[:4] for g in pg], what
    out = dict(exact=0, bypass=0, gave_up=0, cheaper=0, by_orf={})
    others = 0
    for k in range(len(pg)):
        r, lo = rrec[k], int(rlost[k])
        R = ann.pinreplacement_path(i, k).tolist()
        if not r["bypass"]:
            assert R == [] and r["n_removed"] == 0 and r["n_added"] == 0 and r["drop"] == np.inf and lo == 0, (what, k)
            continue
        out["bypass"] += 1
        stop = pg[k][4]
        j = pidx[stop]
        o = ref.by_ends[pg[k][:3]]
        # 1. a simple source -> target path of G' - p_j
        assert R[0] == V - 2 and R[-1] == V - 1 and stop not in R and len(set(R)) == len(R), (what, k)
        assert all(e in W for e in zip(R, R[1:])), (what, k, [e for e in zip(R, R[1:]) if e not in W])  # an edge of G', none refused
        L, cR = sum(W[e] for e in zip(R, R[1:])), sum(e in req for e in zip(R, R[1:]))
        # 2. exact: the pins it carries and the sum, as the record has them
        assert lo >= 0 and cR == cP - lo, (what, k, cR, cP, lo)
        assert float(L - S) / 1000.0 == float(r["drop"]) and (lo, L - S) >= (0, 0), (what, k, L - S, float(r["drop"]))
        out["gave_up"] += lo > 0
        out["cheaper"] += lo > 0 and L < S
        out["by_orf"][o] = (lo, cR)
        take = True
        if limit is not None and o not in (require or ()):
            others += 1
            take = others <= limit
        if take:
            grp = set(np.nonzero(orfs["group"] == orfs["group"][o])[0].tolist())
            without = solve(ref, set(forbid or ()) | grp, [x for x in (require or ()) if x not in grp], bias)
            assert not without["cycle"] and (without["count"], without["S"]) == (cR, L), (what, k, cR, L, without["count"], without["S"])
            out["exact"] += 1
        # 3. prefix / detour / suffix
        a = 0
        while R[a + 1] == P[a + 1]:
            a += 1
        tail, b = len(R) - 1, len(P) - 1
        while R[tail - 1] == P[b - 1]:
            tail -= 1
            b -= 1
        det = R[a + 1: tail]
        assert a < j < b and not any(x in pidx for x in det), (what, k, a, j, b)
        assert len(R) == (a + 1) + len(det) + (len(P) - b)
        # 4. the splice
        removed = [pair_gene(nd, u, v) for u, v in pairs(P[a:b + 1], a, b)]
        added = [pair_gene(nd, u, v) for u, v in pairs([P[a]] + det + [P[b]], a, a + len(det) + 1)]
        g = genes[int(r["gene_off"]): int(r["gene_off"]) + int(r["n_removed"]) + int(r["n_added"])]
        got = [(int(x["left"]), int(x["right"]), int(x["strand"]), int(x["frame"])) for x in g]
        assert r["n_removed"] == len(removed) and r["n_added"] == len(added) and got == removed + added, (what, k)
        assert pg[k][:4] in removed
        for x, t in zip(g, got):  # rp_gene's score: the ORF's weight without the bias, -20 for a tRNA pair
            assert float(x["score"]) == (-20.0 if abs(t[3]) == 4 else ref.weight.get(t[:3], 0.0)), (what, k, t)
        assert r["span_left"] == min(x[0] for x in removed + added) and r["span_right"] == max(x[1] for x in removed + added)
        gr = [pair_gene(nd, u, v) for u, v in pairs(R, 0, len(R) - 1)]
        gp = [pair_gene(nd, u, v) for u, v in pairs(P, 0, len(P) - 1)]
        assert gr == gp[:a // 2] + added + gp[a // 2 + len(removed):], (what, k)
    return out


def pin_repl_batch(b, bias, forbid, require, solve_all=False, limit=3):
    """curate(), pindrops(), pinreplacements(): statuses and offsets equal, every contig with a required ORF through check_records.
    ({contig: its result}, the three results).  No pinned contig with a bypass passes without an exactly compared record."""
    ann = b.ann
    res = curate(ann, bias, forbid, require, solve_all)
    st, offs, genes, delta, unmet = res
    pd = ann.pindrops()
    pr = ann.pinreplacements()
    assert pr[0].tobytes() == pd[0].tobytes() and pr[1].tobytes() == pd[1].tobytes() and pr[4].tobytes() == pd[3].tobytes()
    out = {}
    for i in b.idx:
        if not (require and require[i]):
            continue
        out[i] = check_records(ann, b.refs[i], forbid and forbid[i], require[i], bias and bias[i], rec_of(pd, i), out_of(pr, i), pr[3], limit)
        assert int(pr[0][i]) == int(st[i]), i
        assert out[i] in ("cycle", None) or out[i]["bypass"] == 0 or out[i]["exact"] >= 1, i
    return out, res, pd, pr


def with_path(sols):
    return [s for s in sols.values() if s not in ("cycle", None)]


# ---- 1. the seeded mixes ----
@pytest.mark.parametrize("rnd", (0, 2, 4))
def test_seeded_mixes_against_the_yardstick(small, rnd):
    b = small
    graphs = [DeviceGraph(b.refs[i], b.called[i]) if i in b.refs else NoGraph() for i in range(b.n)]
    row = cd.mixes(graphs)[rnd]
    forbid, require, bias = [None] * b.n, [None] * b.n, [None] * b.n
    for i, d in enumerate(row):
        if d is not None:
            by = b.refs[i].by_ends
            forbid[i], require[i], bias[i] = [by[k] for k in d["forbid"]], [by[k] for k in d["require"]], {by[k]: B for k, B in d["bias"].items()}
    sols, res, pd, pr = pin_repl_batch(b, bias, forbid, require)
    ok = with_path(sols)
    print("round %d: %d draws, %d with a path; %d witnesses weighed, %d also solved, %d give up a pin, %d of them with a negative drop"
          % (rnd, len(sols), len(ok), sum(s["bypass"] for s in ok), sum(s["exact"] for s in ok), sum(s["gave_up"] for s in ok), sum(s["cheaper"] for s in ok)))
    assert len(sols) == sum(d is not None and bool(d["require"]) for d in row) and len(ok) >= 8
    assert sum(s["bypass"] for s in ok) >= 50 and sum(s["exact"] for s in ok) >= len(ok) and sum(s["gave_up"] for s in ok) > 0


# ---- 2. constrain() alone and curate() ----
def test_constrain_alone_and_curate(small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 3310)
    assert sum(r is not None for r in require) >= 6
    ann.constrain(forbid, require)  # mode 2
    pd, pr, run = ann.pindrops(), ann.pinreplacements(), ann.replacements()
    assert pr[0].tobytes() == pd[0].tobytes() and pr[1].tobytes() == pd[1].tobytes() and pr[4].tobytes() == pd[3].tobytes()
    seen = 0
    for i in range(b.n):
        if i in b.refs and require[i]:
            s = check_records(ann, b.refs[i], forbid[i], require[i], None, rec_of(pd, i), out_of(pr, i), pr[3], limit=3)
            seen += s not in ("cycle", None) and s["exact"] >= 1
        else:  # the run's result stands: replacements()' records and genes, gene_off rebased, lost 0, the same path
            assert pin_bytes(pr, i) == contig_bytes(run, i) + (b"\0" * 4 * len(out_of(pr, i)[1]),), i
            if len(out_of(pr, i)[1]):
                assert ann.pinreplacement_path(i, 0).tobytes() == ann.replacement_path(i, 0).tobytes()
    assert seen >= 5
    sols, _, _, _ = pin_repl_batch(b, bias, forbid, require)  # mode 4
    assert sum(s["exact"] >= 1 for s in with_path(sols)) >= 5


# ---- 3. a required called gene; a required uncalled ORF that displaces a call ----
def test_a_required_called_gene_is_given_up_at_its_own_stop(small):
    b = small
    require = b.per_contig(lambda i: [b.called[i][len(b.called[i]) // 2]] if b.called[i] else None)
    sols, res, pd, pr = pin_repl_batch(b, None, None, require)
    seen = 0
    for i, s in sols.items():
        assert s not in ("cycle", None) and res[4][i] == 0, i  # a called gene is kept
        if require[i][0] in s["by_orf"]:  # (its stop has a bypass)
            assert s["by_orf"][require[i][0]] == (1, 0), (i, s["by_orf"][require[i][0]])  # the only pin goes with its stop: the witness carries none
            seen += 1
        assert all((lo, c) in ((0, 1), (1, 0)) for lo, c in s["by_orf"].values()), i  # a witness keeps the pin or gives it up
    assert seen >= 6


def test_a_required_uncalled_orf_that_displaces_a_call(small):
    b = small
    rec0 = {i: b.rec(i) for i in b.idx}
    require = b.per_contig(lambda i: [max(b.reachable(i), key=lambda k: (float(rec0[i]["margin"][k]) if np.isfinite(rec0[i]["margin"][k]) else -1.0, k))] if b.reachable(i) else None)
    sols, res, pd, pr = pin_repl_batch(b, None, None, require)
    st, offs, genes, delta, unmet = res
    moved = seen = 0
    for i, s in sols.items():
        if s in ("cycle", None) or unmet[i] != 0:
            continue
        called = b.refs[i].called(genes[offs[i]:offs[i + 1]])
        assert require[i][0] in called
        moved += any(k not in called for k in b.called[i])
        if require[i][0] in s["by_orf"]:
            assert s["by_orf"][require[i][0]] == (1, 0), i
            seen += 1
    assert seen >= 6 and moved >= 4, (seen, moved)


# ---- 4. two required starts of one stop group ----
def test_two_required_starts_of_one_stop_group(small):
    b, ann = small, small.ann
    require, pairs_ = [None] * b.n, {}
    for i in b.idx:
        orfs = ann.orfs(i)
        grp = {}
        for k in b.reachable(i):
            grp.setdefault(int(orfs["group"][k]), []).append(int(k))
        same = [ks for ks in grp.values() if len(ks) >= 2]
        if same:
            pairs_[i] = tuple(same[len(same) // 2][:2])
            require[i] = list(pairs_[i])
    assert len(pairs_) >= 6
    sols, res, pd, pr = pin_repl_batch(b, None, None, require)
    st, offs, genes, delta, unmet = res
    seen = 0
    for i, s in sols.items():
        if s in ("cycle", None):
            continue
        called = b.refs[i].called(genes[offs[i]:offs[i + 1]])
        kept = [k for k in pairs_[i] if k in called]
        assert unmet[i] == 1 and len(kept) == 1  # a path takes one start per stop
        if kept[0] in s["by_orf"]:
            assert s["by_orf"][kept[0]] == (1, 0), i  # the witness without the stop carries neither start
            seen += 1
    assert seen >= 5


# ---- 5. a batch of every mode and both reductions ----
def test_a_batch_of_every_mode_and_both_reductions(pa, small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 3311)
    full = [i for i in b.idx if require[i]]
    assert len(full) >= 6
    role = {full[0]: 0, full[1]: 1, full[2]: 2, full[3]: 3}  # the run's result, refused only, required only, biased only; the others all three
    F = [forbid[i] if role.get(i, 4) in (1, 4) and i in full else None for i in range(b.n)]
    R = [require[i] if role.get(i, 4) in (2, 4) and i in full else None for i in range(b.n)]
    Bs = [bias[i] if role.get(i, 4) in (3, 4) and i in full else None for i in range(b.n)]
    sols, res, pd, pr = pin_repl_batch(b, Bs, F, R)
    assert sorted(sols) == sorted(i for i in full if role.get(i, 4) in (2, 4)) and sum(s["exact"] >= 1 for s in with_path(sols)) >= 3
    pr = [x.copy() for x in pr]
    paths = {i: [ann.pinreplacement_path(i, k).tobytes() for k in range(len(out_of(pr, i)[1]))] for i in range(b.n)}
    run = ann.replacements()
    # second reduction: a contig of mode 1 or 3 has what rereplacements() gives once every required list is emptied, one of mode 0 replacements()' records
    curate(ann, Bs, F, None)
    want = ann.rereplacements()
    for i in range(b.n):
        if not R[i]:
            assert pin_bytes(pr, i) == contig_bytes(want, i) + (b"\0" * 4 * len(out_of(pr, i)[1]),), (i, role.get(i))
            assert paths[i] == [ann.rereplacement_path(i, k).tobytes() for k in range(len(paths[i]))], i
            if not F[i] and not Bs[i]:
                assert pin_bytes(pr, i)[:3] == contig_bytes(run, i), i
    assert any(contig_bytes(want, i) != contig_bytes(run, i) for i in (full[1], full[3]))  # (the refused / biased contigs differ from the run)
    # first reduction: no contig pinned — rereplacements()' four arrays byte for byte, lost all 0, the counters and times its own
    got = ann.pinreplacements()
    assert all_bytes(got[:4]) == all_bytes(want) and len(got[4]) == len(want[2]) and not got[4].any()
    assert ann.pinreplacement_stats() == ann.rereplacement_stats() and ann.pinreplacements_ms() == ann.rereplacements_ms()
    # ... and after a solve that pinned a contig rereplacements(), its tap and redrops() keep refusing, with their message
    curate(ann, Bs, F, R)
    for call in (ann.redrops, ann.rereplacements, lambda: ann.rereplacement_path(full[1], 0)):
        with pytest.raises(pa.PhxError) as e:
            call()
        assert e.value.code == E_STATE and "required" in str(e.value)
    again = ann.pinreplacements()
    assert [pin_bytes(again, i) for i in range(b.n)] == [pin_bytes(pr, i) for i in range(b.n)]
    assert {i: [ann.pinreplacement_path(i, k).tobytes() for k in range(len(paths[i]))] for i in range(b.n)} == paths


def test_nothing_required_under_solve_all_is_rereplacements(small):
    b, ann = small, small.ann
    forbid, require, bias = sets_of(b, 3312)
    curate(ann, bias, forbid, None, solve_all=True)
    got, want = ann.pinreplacements(), ann.rereplacements()
    assert all_bytes(got[:4]) == all_bytes(want) and len(got[2]) > 50 and got[2]["bypass"].any() and not got[4].any()
    for i in range(b.n):
        for k in range(int(want[1][i + 1] - want[1][i])):
            assert ann.pinreplacement_path(i, k).tobytes() == ann.rereplacement_path(i, k).tobytes(), (i, k)
    assert ann.pinreplacement_stats() == ann.rereplacement_stats() and ann.pinreplacements_ms() == ann.rereplacements_ms()
    ann.curate(None, None, None, solve_all=True)  # ... and on the unchanged graph
    got = ann.pinreplacements()
    assert all_bytes(got[:4]) == all_bytes(ann.rereplacements()) and not got[4].any()
    assert ann.pinreplacement_stats() == ann.rereplacement_stats() == ann.replacement_stats()


# ---- 6. a cross-won slot under a pin ----
@pytest.mark.parametrize("case", range(len(CROSS_SEEDS)))
def test_a_cross_won_slot_under_a_pin(pa, case):
    """A contig of tests/test_rereplace_gpu.py's CROSS_SEEDS: one record won by a cross candidate near the contig's far end; the required
    called gene is the contig's first (outside that record's span), so the cross-won slot is computed by k_rp_cross<NL, MgPinDrop>."""
    seed, gk, _ = CROSS_SEEDS[case]
    ann = pa.Annotator()
    b = Batch(ann, [pa.synth_contig(seed, 50000)])
    ann.replacements()
    assert ann.replacement_stats()["cross"] > 0  # (a stale constant shows itself)
    require = [[b.called[0][gk]]]
    sols, res, pd, pr = pin_repl_batch(b, None, None, require, limit=2)
    s = sols[0]
    assert s not in ("cycle", None) and s["exact"] >= 2 and s["bypass"] > 10 and res[4][0] == 0
    stats = ann.pinreplacement_stats()
    print("seed %d under a pin:" % seed, stats)
    assert stats["cross"] > 0 and stats["chain_nodes"] >= stats["cross"] and stats["regrown"] == 0
    assert ann.rereplacement_stats()["cross"] == 0  # (no contig of mode 1 / 3: the counters are the pinned kernels')
    ann.close()


# ---- 7. regrowth of the delta-chain buffer and the layered trees, in fresh processes ----
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import phanotate_amd as pa
import test_pinreplace_gpu as t
kind, want_bytes = sys.argv[2], sys.argv[3] == "bytes"
ann = pa.Annotator()
if kind == "cross":
    b = t.Batch(ann, [pa.synth_contig(s, 50000) for s, _, _ in t.CROSS_SEEDS])
    require = [[b.called[i][gk]] for i, (_, gk, _) in enumerate(t.CROSS_SEEDS)]
else:
    b = t.Batch(ann, t.cd.mix_seqs(pa))
    require = b.per_contig(lambda i: b.reachable(i)[len(b.reachable(i)) // 3:][:1] + b.called[i][:1] or None)
if want_bytes:
    ann.constrain(None, require)
    out = {"bytes": [x.tobytes().hex() for x in ann.pinreplacements()]}
else:
    sols, res, pd, pr = t.pin_repl_batch(b, None, None, require, limit=1)
    ok = t.with_path(sols)
    out = {"contigs": len(ok), "exact": sum(s["exact"] for s in ok), "bypass": sum(s["bypass"] for s in ok), "gave_up": sum(s["gave_up"] for s in ok)}
out["stats"] = ann.pinreplacement_stats()
out["layered"] = ann.pindrop_stats()["layered"]
print(json.dumps(out))
"""


def child(kind, what, **env):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, kind, what], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_delta_chain_buffer_regrowth(pa):
    """The pr set's delta-chain buffer starts with room for one node (env PHX_REPL_CHAIN_CAP=1): the host grows it, runs the cross winners
    again, and the bytes equal a child whose buffer was large enough."""
    a, b = child("cross", "bytes"), child("cross", "bytes", PHX_REPL_CHAIN_CAP="1")
    assert a["stats"]["regrown"] == 0 and b["stats"]["regrown"] == 1 and a["stats"]["chain_nodes"] > 1 and a["stats"]["cross"] > 0
    assert a["bytes"] == b["bytes"] and a["stats"] == dict(b["stats"], regrown=0)


def test_layered_trees_keep_the_properties(pa):
    out = child("mix", "check", PHX_DROP_LAYERED="1")
    print(out)
    assert out["layered"] > 0 and out["contigs"] >= 8 and out["exact"] >= out["contigs"] and out["bypass"] > out["exact"] and out["gave_up"] > 0


# ---- 8. the wide classes ----
@pytest.mark.parametrize("case", range(4))
def test_a_required_called_gene_in_the_wide_classes(pa, case):
    seqs = wide_cases(pa)[case][0]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    want = (4, 8, 8, 17)[case]  # 320, 576 twice and 1152 bits under MgPinDrop
    c = next(i for i in range(len(seqs)) if st0[i] == 0 and int(ann.globals(i).n_limbs) == want)
    assert ann.margins()[0][c] == 0
    run = ann.replacements()
    ref = CuRef(ann, c)
    cg = ref.called(genes0[offs0[c]:offs0[c + 1]])
    require = [None] * len(seqs)
    require[c] = [cg[len(cg) // 2]]
    ann.constrain(None, require)
    pd, pr = ann.pindrops(), ann.pinreplacements()
    s = check_records(ann, ref, None, require[c], None, rec_of(pd, c), out_of(pr, c), pr[3], limit=1)  # (a solve of these contigs takes seconds)
    assert s not in ("cycle", None) and s["exact"] >= 1 and s["gave_up"] >= 1
    for j in range(len(seqs)):  # neighbours keep the run's records
        if j != c:
            assert pin_bytes(pr, j)[:3] == contig_bytes(run, j) and not out_of(pr, j)[2].any()
    ann.close()


# ---- 9. statuses ----
def test_statuses_and_the_state_rule(pa):
    from phanotate_amd.fasta import read_fasta

    seqs = [seq for name, seq in read_fasta(os.path.join(ROOT, "tests", "golden", "constrain_cycle.fasta"))]
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops  # no path: what lies behind the first stops is out of the source's reach
    seqs = seqs + [pa.synth_contig(61, 9000), unreachable]
    ann = pa.Annotator()
    st0, offs0, genes0 = run_batch(ann, seqs)
    assert st0.tolist() == [0, 0, 0, 1]
    for call in (ann.pinreplacements, lambda: ann.pinreplacement_path(2, 0)):  # before any re-annotation of the run
        with pytest.raises(pa.PhxError) as e:
            call()
        assert e.value.code == E_STATE and "no re-annotation" in str(e.value)
    refs = {i: CuRef(ann, i) for i in range(4)}
    cyc = {i: [k for k, e in enumerate(refs[i].orf_edge) if e is not None and refs[i].on_cycle({e})] for i in (0, 1)}
    free = [k for k, e in enumerate(refs[2].orf_edge) if e is not None][:2]
    quiet = [k for k, e in enumerate(refs[3].orf_edge) if e is None or not refs[3].on_cycle({e})]
    require = [[cyc[0][0]], [cyc[1][-1]], free, quiet[:1]]
    st, offs, genes, delta, unmet = ann.constrain(None, require)
    assert st.tolist()[:2] == [S_NEGCYCLE, S_NEGCYCLE] and st[3] == S_NOPATH
    pd, pr = ann.pindrops(), ann.pinreplacements()
    assert pr[0].tolist() == st.tolist() and pr[1].tobytes() == pd[1].tobytes()
    assert np.diff(pr[1]).tolist()[:2] == [0, 0] and pr[1][4] == pr[1][3]  # PHX_S_NEGCYCLE, PHX_S_NOPATH: no records
    s = check_records(ann, refs[2], None, require[2], None, rec_of(pd, 2), out_of(pr, 2), pr[3], limit=2)
    assert s not in ("cycle", None) and s["exact"] >= 1
    assert check_records(ann, refs[3], None, require[3], None, rec_of(pd, 3), out_of(pr, 3), pr[3]) is None
    with pytest.raises(pa.PhxError):  # no such record
        ann.pinreplacement_path(2, len(out_of(pr, 2)[1]))
    for call in (ann.rereplacements, lambda: ann.rereplacement_path(2, 0), ann.redrops):  # still refused after a pinned solve
        with pytest.raises(pa.PhxError) as e:
            call()
        assert e.value.code == E_STATE and "required" in str(e.value)
    ann.close()


# ---- 10. isolation, the cache, its invalidation ----
def test_pinreplacements_disturb_nothing_are_cached_and_invalidated(pa):
    a, nxt = fuzz(31, 12), fuzz(32, 12)
    ann = pa.Annotator()
    b = Batch(ann, a)

    def the_run():
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()],
                [x.tobytes() for x in ann.replacements()], [ann.path(i)[0].tobytes() for i in range(ann.n)], ann.drop_stats(), ann.replacement_stats())

    forbid, require, bias = sets_of(b, 3340)
    assert sum(r is not None for r in require) >= 5
    # the re-annotation's own state, from a solve without required ORFs
    evidence(ann, bias, forbid)
    plain = ([x.tobytes() for x in ann.remargins()], [x.tobytes() for x in ann.redrops()], [x.tobytes() for x in ann.rereplacements()], ann.redrop_stats(), ann.rereplacement_stats())
    before = the_run()
    r0 = bytes_of(curate(ann, bias, forbid, require))
    pm0 = bytes_of(ann.pinmargins())
    pd0 = [x.tobytes() for x in ann.pindrops()]  # (without the trees)
    pd_stats, pd_ms = ann.pindrop_stats(), ann.pindrops_ms()
    p1 = all_bytes(ann.pinreplacements())  # (the trees once more)
    ms = ann.pinreplacements_ms()
    assert ms["argmin"] > 0 and ms["walk"] > 0
    assert all_bytes(ann.pinreplacements()) == p1 and ann.pinreplacements_ms() == ms  # the second call launches nothing
    assert the_run() == before  # the run's analyses and counters are as they were
    assert bytes_of(ann.pinmargins()) == pm0 and [x.tobytes() for x in ann.pindrops()] == pd0 and ann.pindrop_stats() == pd_stats and ann.pindrops_ms() == pd_ms
    assert bytes_of(curate(ann, bias, forbid, require)) == r0  # (the same re-annotation hits its cache ...)
    assert all_bytes(ann.pinreplacements()) == p1 and ann.pinreplacements_ms() == ms  # ... and keeps the replacements
    other = pa.Annotator()  # the pinned replacements first (the drops come with the trees), everything else behind them
    run_batch(other, a)
    curate(other, bias, forbid, require)
    assert all_bytes(other.pinreplacements()) == p1 and [x.tobytes() for x in other.pindrops()] == pd0 and other.pindrop_stats() == pd_stats
    assert bytes_of(other.pinmargins()) == pm0 and [x.tobytes() for x in other.replacements()] == before[3]
    other.close()
    # a different solve invalidates them
    ann.constrain(forbid, require)
    assert all_bytes(ann.pinreplacements()) != p1
    curate(ann, bias, forbid, require)
    assert all_bytes(ann.pinreplacements()) == p1
    # the analyses of the solve without required ORFs are what they were
    evidence(ann, bias, forbid)
    assert ([x.tobytes() for x in ann.remargins()], [x.tobytes() for x in ann.redrops()], [x.tobytes() for x in ann.rereplacements()], ann.redrop_stats(), ann.rereplacement_stats()) == plain
    # ... and the next batch invalidates them too
    ann.upload(nxt)
    with pytest.raises(pa.PhxError) as e:
        ann.pinreplacements()
    assert e.value.code == E_STATE
    ann.run()
    with pytest.raises(pa.PhxError) as e:
        ann.pinreplacements()
    assert e.value.code == E_STATE
    ann.curate(None, None, None)
    got = ann.pinreplacements()
    assert all_bytes(got[:4]) == [x.tobytes() for x in ann.replacements()] and not got[4].any()
    ann.close()


def test_the_three_sets_stay_apart_across_orders_and_batches(pa):
    """The run's sets, the re-annotation's and the pinned ones share one host layer and must not share state.  One context,
    two batches (fuzz(40, 3), then fuzz(42, 20): every set grows — the sizes of tests/test_redrops_gpu.py's test of this shape, with seed 40
    where that has 41, whose three contigs call 1, 1 and 118 genes: 40 is the nearest seed with two contigs of two calls); per batch one
    curate() call that pins the first contig with two called genes (a called gene of its own required), solves the second such contig again without a pin (a called gene refused, an uncalled ORF penalised)
    and leaves every other contig to the run.  pinreplacements() comes first — it brings the pinned sets up with their trees, behind them
    the re-annotation's with theirs and the run's, first without trees and then with the late tree launch —, then the other analyses and
    every pinned path tap; then evidence() with the same refusals and bias and no required ORF, redrops() and rereplacements().  Everything
    equals, byte for byte and counter for counter, what a fresh context gives in the plain order; the run's counters read the same before
    and after the upper families' passes."""
    from test_evidence_gpu import called_orfs

    def the_sets(ann, st0, offs0, genes0):
        n = ann.n
        cg = {i: called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]]) for i in range(n) if st0[i] == 0}
        two = [i for i in sorted(cg) if len(cg[i]) >= 2][:2]
        assert len(two) == 2
        p, q = two
        bias, forbid, require = [None] * n, [None] * n, [None] * n
        require[p] = [cg[p][len(cg[p]) // 2]]
        forbid[q] = [cg[q][len(cg[q]) // 2]]
        bias[q] = [(next(k for k in range(len(ann.orfs(q))) if k not in cg[q]), 1.5)]
        return p, q, bias, forbid, require

    def taps(ann, offs):
        return [ann.pinreplacement_path(i, k).tobytes() for i in range(ann.n) for k in range(int(offs[i + 1] - offs[i]))]

    def six(ann):
        return (ann.drop_stats(), ann.replacement_stats(), ann.redrop_stats(), ann.rereplacement_stats(), ann.pindrop_stats(), ann.pinreplacement_stats())

    ann = pa.Annotator()
    for seqs in (fuzz(40, 3), fuzz(42, 20)):
        p, q, bias, forbid, require = the_sets(ann, *run_batch(ann, seqs))
        st = ann.curate(bias, forbid, require)[0]
        pr = ann.pinreplacements()  # the first analysis call after the solve
        got = dict(pr=all_bytes(pr), pd=all_bytes(ann.pindrops()), rp=all_bytes(ann.replacements()), dp=all_bytes(ann.drop_margins()), taps=taps(ann, pr[1]), six=six(ann))
        ann.evidence(bias, forbid)
        got.update(rd=all_bytes(ann.redrops()), rr=all_bytes(ann.rereplacements()), six2=six(ann))
        assert st[p] == 0 and st[q] == 0 and pr[0][p] == 0 and pr[0][q] == 0
        assert (out_of(pr, p)[2] > 0).any()  # the pinned contig's records are the pinned set's
        fresh = pa.Annotator()
        assert all_bytes(run_batch(fresh, seqs)) == all_bytes(ann.download_flat(exact=False))
        want = dict(dp=all_bytes(fresh.drop_margins()))
        run = fresh.replacements()
        want.update(rp=all_bytes(run))
        run_stats = (fresh.drop_stats(), fresh.replacement_stats())
        fresh.curate(bias, forbid, require)
        want.update(pd=all_bytes(fresh.pindrops()), pr=all_bytes(fresh.pinreplacements()), taps=taps(fresh, pr[1]), six=six(fresh))
        fresh.evidence(bias, forbid)
        want.update(rd=all_bytes(fresh.redrops()), rr=all_bytes(fresh.rereplacements()), six2=six(fresh))
        assert run_stats == want["six"][:2] == want["six2"][:2]  # the upper families' passes left the run's counters alone
        for key in ("dp", "rp", "pd", "pr", "taps", "six", "rd", "rr", "six2"):
            assert got[key] == want[key], (len(seqs), key)
        assert pin_bytes(pr, q)[:3] != contig_bytes(run, q)  # the contig solved again without a pin: the re-annotation's records, not the run's
        assert all(s["slots"] > 0 for s in (got["six"][0], got["six"][2], got["six"][4]))  # every drop set covered a contig
        fresh.close()
    ann.close()


# ---- 11. batch size and create flags ----
def test_lone_contig_and_batch_of_300_give_the_same_bytes(pa):
    seqs = fuzz(23, 300)
    ann = pa.Annotator()
    run_batch(ann, seqs)
    only = set(range(2, 300, 37))
    require, bias = some_pins(ann, 3350, only)
    curate(ann, bias, None, require)
    out = ann.pinreplacements()
    got = {i: pin_bytes(out, i) for i in only if require[i] is not None}
    assert len(got) >= 5 and sum(st == 0 and len(r) > 0 and len(g) > 0 for st, r, g, lo in got.values()) >= 5
    for i, want in got.items():
        lone = pa.Annotator()
        run_batch(lone, [seqs[i]])
        curate(lone, [bias[i]], None, [require[i]])
        assert pin_bytes(lone.pinreplacements(), 0) == want, i
        lone.close()
    ann.close()


def test_create_flags_give_the_same_bytes(pa):
    batches = ([pa.synth_contig(61, 14000), pa.synth_contig(62, 9000)], fuzz(5, 20))

    def outs(flags):
        ann = pa.Annotator(flags=flags)
        res = []
        for seqs in batches:
            run_batch(ann, seqs)
            require, bias = some_pins(ann, 3351)
            curate(ann, bias, None, require)
            res.append(all_bytes(ann.pinreplacements()))
        ann.close()
        return res

    want = outs(())
    assert all(len(r[2]) > 0 and len(r[3]) > 0 for r in want)
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        assert outs((fl,)) == want, fl


# ---- 12. the CLI ----
def test_cli_pin_drop_replacements(pa, tmp_path):
    from phanotate_amd.cli import format_pin_drops, format_pin_replacements

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
    rq, fb, out, pf, df = tmp_path / "rq.txt", tmp_path / "fb.txt", tmp_path / "out.txt", tmp_path / "pr.txt", tmp_path / "pd.txt"
    rq.write_text("\n".join(rq_lines) + "\n")
    fb.write_text("\n".join(fb_lines) + "\n")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta), "--require", str(rq), "--forbid", str(fb), "--reannotation", str(out),
                          "--pin-drop-replacements", str(pf), "--pin-drop-margins", str(df)], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    ann.constrain(forbid, require)
    pd = ann.pindrops()
    pr = st, offs, rec, genes, lost = ann.pinreplacements()
    assert st.tolist() == [0, 0]
    for i in (0, 1):
        s = check_records(ann, b.refs[i], forbid[i], require[i], None, rec_of(pd, i), out_of(pr, i), genes, limit=2)
        assert s not in ("cycle", None) and s["exact"] >= 1
    text = open(pf, "rb").read()
    assert text == format_pin_replacements(list(seqs), st, offs, rec, genes, lost)
    assert open(df, "rb").read() == format_pin_drops(list(seqs), *pd)  # (both outputs of one command line)
    rows = [ln.split("\t") for ln in text.decode().splitlines() if not ln.startswith("#")]
    assert len(rows) == len(rec) and all(len(r) == 8 for r in rows)
    assert sum(int(r[5]) > 0 for r in rows) == int((lost > 0).sum()) > 0
    ann.close()
