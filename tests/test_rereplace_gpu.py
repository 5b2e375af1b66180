"""Re-annotation replacements on the device (phx_rereplacements_flat, phx_tap_rereplacement) against python integers.  The
yardstick is EvRef.solve of tests/test_evidence_gpu.py: the edge list of G' with W' it returns for (forbid, bias) weighs every edge of a
witness — an edge that is not in it is a failure —, and the D it returns for (forbid + the gene's stop group, bias) is what the witness
must weigh, exactly.  Properties 1-4 are checked as tests/test_replace_gpu.py::check_contig checks them, on the re-annotation's path.
Also the identities with replacements(), the cross winners, the regrowth of the delta-chain buffer and the layered trees in fresh
processes, the wide classes, statuses, the cache, isolation and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_evidence_gpu import NEGCYCLE, EvRef, called_orfs, draw_orfs, evidence, solved_contigs
from test_reannotate_gpu import fuzz, mask_rounds, run_batch, wide_cases
from test_redrops_gpu import solve, _solved
from test_remargins_gpu import cycle_orf, draw_penalties, some_evidence
from test_replace_gpu import pair_gene, pairs, py_render
from test_scenarios_gpu import case1_seqs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def as_bytes(x):
    return [a.tobytes() for a in x]


def contig_bytes(out, i):
    """Contig i of rereplacements() / replacements(): status, records with gene_off counted from the contig's first gene, its genes."""
    st, offs, rec, genes = out
    mine = rec[offs[i]:offs[i + 1]].copy()
    ng = int((mine["n_removed"] + mine["n_added"]).sum())
    base = int(mine["gene_off"][0]) if len(mine) else 0
    mine["gene_off"] -= base
    return int(st[i]), mine.tobytes(), genes[base:base + ng].tobytes()


def check_records(ann, ref, forbid, bias, drec, rrec, genes, sample=None, rng=None):
    """One solved-again contig: the records equal the redrops() records; every bypass record's R'_g has properties 1-4 on G' and P', and
    W'(R'_g) = D'_{-g} by the yardstick (for `sample` of them when given).  Returns (records compared exactly, bypass records)."""
    i = ref.i
    for f in ("left", "right", "strand", "frame", "called", "bypass"):
        assert (rrec[f] == drec[f]).all(), (i, f)
    assert rrec["drop"].tobytes() == drec["drop"].tobytes(), i
    if not len(rrec):
        return 0, 0
    sol = solve(ref, forbid, bias)
    assert sol != NEGCYCLE and sol[0] is not None, i
    DB, P, edges = sol[0], sol[1], sol[4]
    assert ann.reannotated_path(i)[0].tolist() == P, i
    W = {(u, v): w for u, v, w in edges}  # G' with W': a refused ORF edge is not in it, a biased one weighs W + B
    assert len(W) == len(edges)
    pidx = {v: t for t, v in enumerate(P)}
    V, nd, orfs = ref.V, ref.nd, ref.orfs
    pg = []  # the CDS genes of P' in path order: (left, right, strand, frame, stop node)
    for k in range((len(P) - 1) // 2):
        a, b = P[2 * k + 1], P[2 * k + 2]
        fa = int(nd["frame"][a])
        if abs(fa) <= 3:
            pg.append(pair_gene(nd, a, b) + (b if fa > 0 else a,))
    assert [(int(r["left"]), int(r["right"]), int(r["strand"]), int(r["frame"])) for r in rrec] == [g[:4] for g in pg], i
    ks = [k for k in range(len(pg)) if rrec[k]["bypass"]]
    exact_ks = set(ks)
    if sample is not None and len(ks) > sample:
        exact_ks = set(rng.choice(ks, sample, replace=False).tolist())
    n = 0
    for k in range(len(pg)):
        r = rrec[k]
        R = ann.rereplacement_path(i, k).tolist()
        if not r["bypass"]:
            assert R == [] and r["n_removed"] == 0 and r["n_added"] == 0 and r["drop"] == np.inf, (i, k)
            continue
        stop = pg[k][4]
        j = pidx[stop]
        # 1. a simple source -> target path of G' - p_j
        assert R[0] == V - 2 and R[-1] == V - 1 and stop not in R and len(set(R)) == len(R), (i, k)
        assert all((u, v) in W for u, v in zip(R, R[1:])), (i, k, [e for e in zip(R, R[1:]) if e not in W])  # an edge of G', none refused
        L = sum(W[(u, v)] for u, v in zip(R, R[1:]))
        # 2. exact
        assert float(L - DB) / 1000.0 == float(r["drop"]), (i, k, L - DB, float(r["drop"]))
        if k in exact_ks:
            o = ref.by_ends[pg[k][:3]]
            group = np.nonzero(orfs["group"] == orfs["group"][o])[0].tolist()
            without = solve(ref, set(forbid or ()) | set(group), bias)
            assert without != NEGCYCLE and L == without[0], (i, k, L, without[0])
            n += 1
        # 3. prefix / detour / suffix
        a = 0
        while R[a + 1] == P[a + 1]:
            a += 1
        tail = len(R) - 1
        b = len(P) - 1
        while R[tail - 1] == P[b - 1]:
            tail -= 1
            b -= 1
        det = R[a + 1: tail]
        assert a < j < b and not any(x in pidx for x in det), (i, k, a, j, b)
        assert len(R) == (a + 1) + len(det) + (len(P) - b)
        # 4. the splice
        removed = [pair_gene(nd, u, v) for u, v in pairs(P[a:b + 1], a, b)]
        added = [pair_gene(nd, u, v) for u, v in pairs([P[a]] + det + [P[b]], a, a + len(det) + 1)]
        g = genes[int(r["gene_off"]): int(r["gene_off"]) + int(r["n_removed"]) + int(r["n_added"])]
        got = [(int(x["left"]), int(x["right"]), int(x["strand"]), int(x["frame"])) for x in g]
        assert r["n_removed"] == len(removed) and r["n_added"] == len(added) and got == removed + added, (i, k)
        assert pg[k][:4] in removed
        for x, t in zip(g, got):  # the score of the re-annotation's own gene records: the weight without the bias
            assert float(x["score"]) == (-20.0 if abs(t[3]) == 4 else ref.weight.get(t[:3], 0.0)), (i, k, t)
        assert r["span_left"] == min(x[0] for x in removed + added) and r["span_right"] == max(x[1] for x in removed + added)
        gr = [pair_gene(nd, u, v) for u, v in pairs(R, 0, len(R) - 1)]
        gp = [pair_gene(nd, u, v) for u, v in pairs(P, 0, len(P) - 1)]
        i0 = a // 2
        assert gr == gp[:i0] + added + gp[i0 + len(removed):], (i, k)
    return n, len(ks)


def check_batch(ann, refs, forbid, bias, solve_all=False, sample=None, rng=None):
    """evidence(bias, forbid) — reannotate(forbid) where there is no bias —, redrops(), rereplacements(): statuses and offsets equal, every
    solved-again contig of refs through check_records.  {contig: (status, compared exactly, bypass records, P')}; a solved-again contig
    with a path has at least one compared bypass record."""
    if bias is None:
        st = ann.reannotate(forbid, solve_all=solve_all)[0]
    else:
        st = evidence(ann, bias, forbid, solve_all=solve_all)[0]
    dst, doffs, drec = ann.redrops()
    rst, roffs, rrec, genes = ann.rereplacements()
    assert rst.tobytes() == dst.tobytes() and roffs.tobytes() == doffs.tobytes()
    assert len(rrec) == len(drec)
    out = {}
    for i in refs:
        f = None if forbid is None else forbid[i]
        b = None if bias is None else bias[i]
        if f is None and b is None and not solve_all:
            continue
        n, nb = check_records(ann, refs[i], f, b, drec[doffs[i]:doffs[i + 1]], rrec[roffs[i]:roffs[i + 1]], genes, sample, rng)
        assert int(rst[i]) == int(st[i]), i
        if st[i] == 0:
            assert n >= 1, i  # no solved-again contig with a path passes without a compared bypass record
        out[i] = (int(st[i]), n, nb, ann.reannotated_path(i)[0].tolist() if st[i] == 0 else None)
    return out


@pytest.fixture(scope="module")
def big(pa):
    """case1_seqs + fuzz(11, 6), run once: one contig of one chunk and eight of several.  (ann, the run's download, yardsticks, the run's
    paths, the called ORFs.)  The tests leave the batch resident."""
    ann = pa.Annotator()
    dl = run_batch(ann, case1_seqs(pa) + fuzz(11, 6))
    idx = solved_contigs(ann, dl[0])
    V = {i: int(ann.globals(i).n_node) for i in idx}
    assert any(v <= 256 for v in V.values()) and sum(v > 256 for v in V.values()) >= 8, sorted(V.items())
    refs = {i: EvRef(ann, i) for i in idx}
    called = {i: called_orfs(ann, i, dl[2][dl[1][i]:dl[1][i + 1]]) for i in idx}
    yield ann, dl, refs, {i: ann.path(i)[0].tolist() for i in idx}, called
    ann.close()
    _solved.clear()


# ---- 1. the yardstick ----
def test_every_mask_round_against_the_yardstick(big):
    ann, dl, refs, P, called = big
    n = ann.n
    rng = np.random.RandomState(3001)
    order = sorted(refs)
    plans = dict(zip(order, mask_rounds([refs[i] for i in order], [called[i] for i in order], rng)))
    have = [i for i in order if called[i]]
    assert len(have) >= len(order) - 1
    records = moved = 0
    for r in range(max(len(plans[i]) for i in have)):
        forbid = [plans[i][r] if i in have and r < len(plans[i]) else None for i in range(n)]
        got = check_batch(ann, refs, forbid, None)
        assert set(got) == {i for i in have if r < len(plans[i])}
        for i, g in got.items():
            records += g[1]
            moved += g[0] == 0 and g[3] != P[i]  # (a refused called gene: P' is another path)
    print("masks: %d witnesses compared exactly, %d re-annotations with another path" % (records, moved))
    assert records >= 100 and moved >= 1


def test_penalties_alone_and_with_a_mask(big):
    ann, dl, refs, P, called = big
    bias, forbid = draw_penalties(ann, refs, called, np.random.RandomState(3002))
    assert any(f for f in forbid)
    for fb in (None, forbid):
        got = check_batch(ann, refs, fb, bias)
        assert set(got) == set(refs)
        assert sum(g[0] == 0 for g in got.values()) >= len(refs) - 1


def test_bonuses_of_the_titration_draw(big):
    """Ten points of §19's titration draw at -Delta - 1: the uncalled ORF comes in, P' changes, and every record of the new path —
    the new gene's among them — has its witness."""
    ann, dl, refs, P, called = big
    n = ann.n
    idx = sorted(refs)
    mst, moffs, mrec = ann.margins()
    rng = np.random.RandomState(1904)
    picks = {}
    for i in idx:
        rec = mrec[moffs[i]:moffs[i + 1]]
        ok = [k for k in range(len(rec)) if rec["through"][k] == 1 and rec["called"][k] == 0 and np.isfinite(rec["margin"][k]) and round(float(rec["margin"][k]) * 1000) < 1 << 50]
        take = sorted(rng.choice(ok, min(len(ok), 10), replace=False).tolist())
        picks[i] = [(k, int(round(float(rec["margin"][k]) * 1000))) for k in take]
    points = 0
    for r in range(10):
        bias = [{picks[i][r][0]: -picks[i][r][1] - 1} if i in picks and r < len(picks[i]) else None for i in range(n)]
        got = check_batch(ann, refs, None, bias)
        assert got and all(g[0] == 0 and g[3] != P[i] for i, g in got.items()), r  # the bonus wins by one unit: another path
        points += 1
    assert points == 10


# ---- 2. no policy is the run's ----
def check_equals_replacements(ann):
    """Nothing refused, no bias.  solve_all: every contig through the conditioned kernels on an unchanged graph — the four arrays are
    replacements()' byte for byte (`called` apart on a contig whose delivered genes are the host's, as for redrops()), the paths and the
    counters too.  Without: replacements()' arrays byte for byte and no kernel of the feature runs."""
    n = ann.n
    want = ann.replacements()
    wpaths = [[ann.replacement_path(i, k).tobytes() for k in range(int(want[1][i + 1] - want[1][i]))] for i in range(n)]
    cert = ann.certified()
    ann.reannotate([None] * n, solve_all=True)
    got = ann.rereplacements()
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[3].tobytes() == want[3].tobytes()
    seen = 0
    for i in range(n):
        a, b = got[2][got[1][i]:got[1][i + 1]], want[2][want[1][i]:want[1][i + 1]]
        if cert[i] == 1:
            assert a.tobytes() == b.tobytes(), i
            seen += len(a) > 0
        else:
            for f in a.dtype.names:
                assert f == "called" or a[f].tobytes() == b[f].tobytes(), (i, f)
        assert [ann.rereplacement_path(i, k).tobytes() for k in range(len(a))] == wpaths[i], i
    assert ann.rereplacement_stats() == ann.replacement_stats()
    ann.reannotate([None] * n)
    assert as_bytes(ann.rereplacements()) == as_bytes(want)
    assert ann.rereplacements_ms() == dict(argmin=0.0, walk=0.0, download=0.0)  # (no conditioned kernel ran)
    return seen


def test_nothing_refused_no_bias_is_replacements_byte_for_byte(pa, big):
    assert check_equals_replacements(big[0]) >= 5
    ann = pa.Annotator()
    run_batch(ann, fuzz(101, 150))  # the cross-node batch of tests/test_drop_gpu.py
    assert check_equals_replacements(ann) >= 75
    print("cross-node batch:", ann.replacement_stats())
    ann.close()


# ---- 3. cross winners ----
# Two of the benchmark's contigs synth_contig(s, 50000) that have a slot won by a cross candidate whose delta chain stays in the witness
# (replacement_stats()["cross"] > 0 and ["cross_kept"] > 0), found once on the device the way
# tests/test_replace_gpu.py::test_cross_winners_are_checked finds them: batches of 100 seeds from 0, then each contig of a batch with a
# cross winner alone.  Per seed the policy of the test: the called gene to refuse (its index among the run's called CDS genes in path
# order) and the uncalled ORF to penalise (its index in orfs(0)), both outside span_left .. span_right of the cross-won record — found
# by refusing every called gene in turn: the ones whose refusal loses the cross winner lie inside, the one chosen is the farthest from them.
# Seeds 2 and 12 (16 and 17 are the next): one cross-won record each, with 2 delta-chain nodes; it goes away only when called gene 55
# (seed 2; the spans of that record: 46491 .. 47745) or 44 (seed 12; 37052 .. 37679) is refused.  The policy is at the contig's other end:
# the first called gene (3 .. 146 and 40 .. 876) and the uncalled ORF nearest its left end (ORF 2 at 3 .. 95, ORF 8 at 40 .. 162).
CROSS_SEEDS = ((2, 0, 2), (12, 0, 8))  # (seed, refused called gene, penalised ORF)


def cross_contigs(pa):
    assert len(CROSS_SEEDS) == 2
    return [pa.synth_contig(s, 50000) for s, _, _ in CROSS_SEEDS]


def test_cross_winners_without_and_under_a_policy(pa):
    seqs = cross_contigs(pa)
    rng = np.random.RandomState(3003)
    for seq, (seed, gk, ok) in zip(seqs, CROSS_SEEDS):
        ann = pa.Annotator()
        dl = run_batch(ann, [seq])
        ann.replacements()
        st = ann.replacement_stats()
        assert st["cross"] > 0 and st["cross_kept"] > 0, (seed, st)  # (a stale constant shows itself)
        check_equals_replacements(ann)  # test 2's comparison
        assert ann.rereplacement_stats()["cross"] == 0  # (... whose last call solves nothing again)
        cg =called_orfs(ann, 0, dl[2])
        assert ok not in cg
        got = check_batch(ann, {0: EvRef(ann, 0)}, [[cg[gk]]], [{ok: 2500}], sample=4, rng=rng)
        assert got[0][0] == 0 and got[0][1] == 4
        assert ann.rereplacement_stats()["cross"] > 0, (seed, ann.rereplacement_stats())
        ann.close()
        _solved.clear()


# ---- 4. regrowth of the delta-chain buffer, in fresh processes ----
REGROW_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import phanotate_amd as pa
seqs = [pa.synth_contig(int(s), 50000) for s in sys.argv[2:]]
ann = pa.Annotator()
ann.upload(seqs)
ann.run()
ann.reannotate([None] * ann.n, solve_all=True)
out = ann.rereplacements()
print(json.dumps({"bytes": [x.tobytes().hex() for x in out], "stats": ann.rereplacement_stats()}))
"""


def test_delta_chain_buffer_regrowth(pa):
    """The new set's delta-chain buffer starts with room for one node (env PHX_REPL_CHAIN_CAP=1): the host grows it, runs the cross
    winners again, and the bytes equal a child whose buffer was large enough."""
    outs = []
    for env in ({}, {"PHX_REPL_CHAIN_CAP": "1"}):
        r = subprocess.run([sys.executable, "-c", REGROW_CHILD, ROOT] + [str(s) for s, _, _ in CROSS_SEEDS], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    a, b = outs
    assert a["stats"]["regrown"] == 0 and b["stats"]["regrown"] == 1 and a["stats"]["chain_nodes"] > 1
    assert a["bytes"] == b["bytes"] and a["stats"] == dict(b["stats"], regrown=0)


# ---- 5. the layered trees, in a fresh process ----
LAYERED_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tools"); sys.path.insert(0, sys.argv[1] + "/tests")
import phanotate_amd as pa, fuzz_gpu
import test_rereplace_gpu as t
rng = np.random.RandomState(101)
seqs = [fuzz_gpu.make(rng) for _ in range(30)]
ann = pa.Annotator()
dl = t.run_batch(ann, seqs)
st0, offs0, genes0 = dl
bias, forbid = [], []
for i in range(ann.n):  # per solved contig a refused called gene, a penalised one and three ORFs with a bonus
    cg = t.called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]]) if st0[i] == 0 and int(ann.globals(i).n_node) > 2 else []
    if len(cg) < 2:
        bias.append(None); forbid.append(None)
        continue
    b = {int(k): -int(rng.randint(1, 3000)) for k in rng.choice(len(ann.orfs(i)), min(3, len(ann.orfs(i))), replace=False)}
    b[cg[len(cg) // 2]] = 5000
    bias.append(b); forbid.append([cg[0]])
refs = {i: t.EvRef(ann, i) for i in range(ann.n) if bias[i] is not None}
negs = [i for i in refs if t.solve(refs[i], forbid[i], bias[i]) == t.NEGCYCLE]
for i in negs:
    del refs[i]
got = t.check_batch(ann, refs, forbid, bias, sample=2, rng=np.random.RandomState(5))
print(json.dumps({"contigs": len(got), "exact": sum(g[1] for g in got.values()), "bypass": sum(g[2] for g in got.values()), "negs": len(negs), "layered": ann.redrop_stats()["layered"]}))
"""


def test_layered_trees_keep_the_properties(pa):
    r = subprocess.run([sys.executable, "-c", LAYERED_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=dict(os.environ, PHX_DROP_LAYERED="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["layered"] > 0 and out["contigs"] >= 20 and out["exact"] >= 20 and out["bypass"] > out["exact"]


# ---- 6. the wide classes ----
@pytest.mark.parametrize("case", range(4))
def test_a_refused_called_gene_in_the_wide_classes(pa, case):
    seqs, nl = wide_cases(pa)[case]
    ann = pa.Annotator()
    dl = run_batch(ann, seqs)
    want = (4, 8, 8, 17)[case]  # 256, 512, 512 and 1088 bits
    i = next(i for i in range(len(seqs)) if dl[0][i] == 0 and int(ann.globals(i).n_limbs) == want)
    refs = {i: EvRef(ann, i)}
    cg = called_orfs(ann, i, dl[2][dl[1][i]:dl[1][i + 1]])
    rng = np.random.RandomState(3006 + case)
    forbid = [None] * len(seqs)
    forbid[i] = [cg[int(rng.randint(len(cg)))]]
    got = check_batch(ann, refs, forbid, None, sample=3, rng=rng)
    assert got[i][0] == 0 and got[i][1] >= 1
    ann.close()
    _solved.clear()


# ---- 7. statuses, the cache, isolation ----
def test_statuses_in_one_mixed_batch(pa):
    """The mixed batch of tests/test_redrops_gpu.py::test_statuses_in_one_mixed_batch."""
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
        ann.rereplacements()
    assert e.value.code == -13 and "no re-annotation" in str(e.value)
    with pytest.raises(pa.PhxError) as e:
        ann.rereplacement_path(5, 0)
    assert e.value.code == -13
    forbid = [None, None, np.arange(len(ann.orfs(2))), None, None, None, None]
    bias = [None, None, None, {neg[1]: -10 ** 9}, None, None, None]
    for i in (5, 6):
        bias[i] = {called_orfs(ann, i, genes0[offs0[i]:offs0[i + 1]])[0]: 4000, 3: -2500}
    evidence(ann, bias, forbid)
    dst, doffs, drec = ann.redrops()
    out = ann.rereplacements()
    assert out[0].tolist() == dst.tolist() == [-2, -3, 1, -9, 0, 0, 0] and out[1].tobytes() == doffs.tobytes()
    assert contig_bytes(out, 4) == contig_bytes(ann.replacements(), 4)  # not solved again: the run's records and genes, gene_off rebased
    assert ann.rereplacement_path(4, 0).tobytes() == ann.replacement_path(4, 0).tobytes()
    for i in (5, 6):
        n, nb = check_records(ann, EvRef(ann, i), None, bias[i], drec[doffs[i]:doffs[i + 1]], out[2][out[1][i]:out[1][i + 1]], out[3])
        assert n >= 1
    # required ORFs on any contig: PHX_E_STATE, and the text says why
    req = [None] * 7
    req[6] = [called_orfs(ann, 6, genes0[offs0[6]:offs0[7]])[0]]
    ann.constrain(require=req)
    with pytest.raises(pa.PhxError) as e:
        ann.rereplacements()
    assert e.value.code == -13 and "required" in str(e.value)
    ann.close()
    _solved.clear()


def test_rereplacements_disturb_nothing_are_cached_and_invalidated(pa):
    a, b = fuzz(31, 20), fuzz(32, 20)

    def everything(ann, bias, forbid):
        return ([x.tobytes() for x in ann.download_flat()], [x.tobytes() for x in ann.margins()], [x.tobytes() for x in ann.drop_margins()],
                [x.tobytes() for x in ann.replacements()], [x.tobytes() for x in evidence(ann, bias, forbid)], [x.tobytes() for x in ann.remargins()],
                [x.tobytes() for x in ann.redrops()], [ann.reannotated_path(i)[0].tobytes() for i in range(ann.n)])

    ann = pa.Annotator()
    run_batch(ann, a)
    bias, forbid = some_evidence(ann, 3008)
    before = everything(ann, bias, forbid)  # (redrops() first, without the trees)
    assert ann.rereplacements_ms() == dict(argmin=0.0, walk=0.0, download=0.0)
    r1 = as_bytes(ann.rereplacements())
    ms = ann.rereplacements_ms()
    assert ms["argmin"] > 0 and ms["walk"] > 0
    assert as_bytes(ann.rereplacements()) == r1 and ann.rereplacements_ms() == ms  # the second call launches nothing
    assert everything(ann, bias, forbid) == before  # (the same re-annotation hits its cache ...)
    assert as_bytes(ann.rereplacements()) == r1 and ann.rereplacements_ms() == ms  # ... and keeps the replacements
    other = pa.Annotator()  # the replacements of the re-annotation first (the drops come with the trees), everything else behind them
    run_batch(other, a)
    evidence(other, bias, forbid)
    assert as_bytes(other.rereplacements()) == r1 and everything(other, bias, forbid) == before
    assert other.redrop_stats() == ann.redrop_stats()
    # a different re-annotation invalidates them
    bias2, forbid2 = some_evidence(ann, 3009)
    evidence(ann, bias2, forbid2)
    evidence(other, bias2, forbid2)
    r2 = as_bytes(ann.rereplacements())
    assert r2 != r1 and r2 == as_bytes(other.rereplacements())
    other.close()
    # ... and so does the next run, whose own results are a fresh context's
    ann.upload(b)
    with pytest.raises(pa.PhxError) as e:
        ann.rereplacements()
    assert e.value.code == -13
    ann.run()
    with pytest.raises(pa.PhxError) as e:
        ann.rereplacements()
    assert e.value.code == -13
    fresh = pa.Annotator()
    run_batch(fresh, b)
    bias, forbid = some_evidence(fresh, 3010)
    evidence(ann, bias, forbid)
    evidence(fresh, bias, forbid)
    assert as_bytes(ann.rereplacements()) == as_bytes(fresh.rereplacements())
    for x in (ann, fresh):
        x.close()


def test_lone_contig_and_batch_of_300_give_the_same_bytes(pa):
    seqs = fuzz(23, 300)
    ann = pa.Annotator()
    run_batch(ann, seqs)
    only = set(range(2, 300, 37))
    bias, forbid = some_evidence(ann, 3011, only)
    evidence(ann, bias, forbid, solve_all=True)
    out = ann.rereplacements()
    got = {i: contig_bytes(out, i) for i in only if bias[i] is not None}
    assert len(got) >= 5 and all(st == 0 and len(r) > 0 and len(g) > 0 for st, r, g in got.values())
    for i, want in got.items():
        lone = pa.Annotator()
        run_batch(lone, [seqs[i]])
        evidence(lone, [bias[i]], [forbid[i]])
        assert contig_bytes(lone.rereplacements(), 0) == want, i
        lone.close()
    ann.close()


def test_create_flags_give_the_same_bytes(pa):
    batches = ([pa.synth_contig(61, 14000), pa.synth_contig(62, 9000)], fuzz(5, 20))

    def outs(flags):
        ann = pa.Annotator(flags=flags)
        res = []
        for seqs in batches:
            run_batch(ann, seqs)
            bias, forbid = some_evidence(ann, 3012)
            evidence(ann, bias, forbid)
            res.append(as_bytes(ann.rereplacements()))
        ann.close()
        return res

    want = outs(())
    assert all(len(r[2]) > 0 and len(r[3]) > 0 for r in want)
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        assert outs((fl,)) == want, fl


# ---- 8. the CLI ----
def test_cli_redrop_replacements(pa, tmp_path):
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
    ev, fb, out, rf, df = tmp_path / "ev.txt", tmp_path / "fb.txt", tmp_path / "out.txt", tmp_path / "rr.txt", tmp_path / "rd.txt"
    ev.write_text("".join("%s\t%r\n" % (ln, b) for (k, ln), b in zip(rows, vals)))
    fb.write_text(rows[5][1] + "\n")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta), "--forbid", str(fb), "--evidence", str(ev), "--reannotation", str(out), "--redrop-replacements", str(rf),
                          "--redrop-margins", str(df)], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    ann.evidence([[(k, b) for (k, ln), b in zip(rows, vals)]], [[rows[5][0]]])
    st, offs, rec, genes = ann.rereplacements()
    assert st.tolist() == [0] and len(rec) > 3 and rec["bypass"].any()
    assert rf.read_text() == py_render([name], st, offs, rec, genes)
    from phanotate_amd import cli

    assert rf.read_bytes() == cli.format_replacements([name], st, offs, rec, genes)
    assert df.read_bytes() == cli.format_drops([name], *ann.redrops())  # (both outputs of one command line)
    ann.close()
