"""Drop replacements on the device (phx_replacements_flat, phx_tap_replacement) against python integers over the device's
own edges (phx_tap_edges, weight = trunc(w * 1000)): every replacement path R_g is a simple source -> target path that avoids the stop
node, of length exactly D_{-g}, in prefix / detour / suffix form, and its removed / added genes are the splice of P and R_g.  Also the
records against drop_margins(), determinism over batches and flags, the layered trees, wide classes, statuses, non-interference, the
pipeline and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, exact_dist_from_device_edges, golden_cases, golden_params, golden_trnas, load_golden
from test_drop_gpu import device_graph, dist_without, fuzz, path_genes, wide_contig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def pair_gene(nd, u, v):
    f = int(nd["frame"][u])
    return (int(nd["pos"][u]), int(nd["pos"][v]) + 2, -1 if f < 0 else 1, f)


def pairs(seq, lo, hi):
    """(u, v) of the pairs (2i+1, 2i+2) of a path with lo <= 2i+1 and 2i+2 <= hi (indices of seq, which starts at index lo)."""
    return [(seq[q - lo], seq[q + 1 - lo]) for q in range(lo, hi) if q % 2 == 1 and q + 1 <= hi]


def check_contig(ann, i, drec, rrec, genes, sample=None, rng=None, exact=True):
    """Records equal the drop records; every bypass record's R_g has properties 1-4 (and, for `sample` of them, W(R_g) = D_{-g})."""
    for f in ("left", "right", "strand", "frame", "called", "bypass"):
        assert (rrec[f] == drec[f]).all(), (i, f)
    assert rrec["drop"].tobytes() == drec["drop"].tobytes(), i
    if not len(rrec):
        return 0, 0
    P = ann.path(i)[0].tolist()
    pidx = {v: t for t, v in enumerate(P)}
    V, src, dst, w = device_graph(ann, i)
    W = {(u, v): x for u, v, x in zip(src, dst, w)}
    assert len(W) == len(src)
    ds = exact_dist_from_device_edges(ann, i)
    D = ds[V - 1]
    nd = ann.nodes(i)
    pg = path_genes(ann, i)
    ks = list(range(len(pg)))
    exact_ks = set(ks)
    if sample is not None and len(ks) > sample:
        exact_ks = set(rng.choice(len(ks), sample, replace=False).tolist())
    n = 0
    for k in ks:
        r = rrec[k]
        R = ann.replacement_path(i, k).tolist()
        if not r["bypass"]:
            assert R == [] and r["n_removed"] == 0 and r["n_added"] == 0, (i, k)
            continue
        stop = pg[k][4]
        j = pidx[stop]
        # 1. a simple source -> target path of G - p_j
        assert R[0] == V - 2 and R[-1] == V - 1 and stop not in R and len(set(R)) == len(R), (i, k)
        L = sum(W[(u, v)] for u, v in zip(R, R[1:]))  # (KeyError: not an edge)
        # 2. exact
        assert float(L - D) / 1000.0 == float(r["drop"]), (i, k)
        if exact and k in exact_ks:
            assert L == dist_without(V, src, dst, w, stop), (i, k)
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
        assert all(x["score"] == -20.0 for x in g if abs(int(x["frame"])) == 4)
        assert r["span_left"] == min(x[0] for x in removed + added) and r["span_right"] == max(x[1] for x in removed + added)
        gr = [pair_gene(nd, u, v) for u, v in pairs(R, 0, len(R) - 1)]
        gp = [pair_gene(nd, u, v) for u, v in pairs(P, 0, len(P) - 1)]
        i0 = a // 2
        assert gr == gp[:i0] + added + gp[i0 + len(removed):], (i, k)
    return n, len(ks)


def run_and_check(ann, seqs, trnas=None, full=None, sample=None, seed=0, exact=True):
    ann.upload(seqs)
    ann.set_trnas(trnas)
    ann.run()
    dst_, doffs, drec = ann.drop_margins()
    rst, roffs, rrec, genes = ann.replacements()
    assert rst.tobytes() == dst_.tobytes() and roffs.tobytes() == doffs.tobytes()
    rng = np.random.RandomState(seed)
    n = 0
    for i in range(len(seqs)):
        if rst[i] != 0 or (full is not None and i not in full):
            continue
        n += check_contig(ann, i, drec[doffs[i]:doffs[i + 1]], rrec[roffs[i]:roffs[i + 1]], genes, sample, rng, exact)[0]
    return rst, roffs, rrec, genes, n


def as_bytes(x):
    return [a.tobytes() for a in x]


def test_golden_fixtures(pa):
    n = 0
    for case in golden_cases():
        g, name, seq = load_golden(case)
        if str(g["error"]) or case == "edge_huge":
            continue
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        tr = golden_trnas(g)
        rst, roffs, rrec, genes, k = run_and_check(ann, [seq], trnas=None if tr is None else [tr], sample=6)
        n += k
        ann.close()
    assert n >= 40


def test_fuzz_batch_lone_and_flags(pa):
    seqs = fuzz(11, 120)
    ann = pa.Annotator()
    rst, roffs, rrec, genes, n = run_and_check(ann, seqs, full=set(range(0, 120, 4)), sample=3, seed=1)
    assert (rst == 0).sum() > 80 and n > 30
    ms = ann.replacements_ms()
    assert set(ms) == {"argmin", "walk", "download"} and all(v > 0 for v in ms.values())
    for i in range(0, 120, 13):
        lone = pa.Annotator()
        lone.upload([seqs[i]])
        lone.run()
        s1, o1, r1, g1 = lone.replacements()
        mine = rrec[roffs[i]:roffs[i + 1]].copy()
        base = mine["gene_off"][0] if len(mine) else 0
        mine["gene_off"] -= base
        assert s1[0] == rst[i] and r1.tobytes() == mine.tobytes(), i
        assert g1.tobytes() == genes[base: base + len(g1)].tobytes(), i
        lone.close()
    want = as_bytes((rst, roffs, rrec, genes))
    assert as_bytes(ann.replacements()) == want  # (kept)
    ann.close()
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        other = pa.Annotator(flags=(fl,))
        other.upload(seqs)
        other.run()
        assert as_bytes(other.replacements()) == want, fl
        other.close()


def test_wide_integer_classes_and_cross_winners(pa):
    rng = np.random.RandomState(3000)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    c256 = [pa.synth_contig(900 + k, 20000).decode() + "atg" + "".join(rng.choice(sense, 3000)) + "taa" + pa.synth_contig(1900 + k, 20000).decode() for k in range(6)]
    cases = [(c256, 2), ([wide_contig(pa, 8000, 8000, density=0.01)], 8), ([wide_contig(pa, 5500, 42)], 8), ([wide_contig(pa, 12000, 42)], 17)]
    seen, rescanned = set(), 0
    for seqs, nl in cases:
        ann = pa.Annotator()
        run_and_check(ann, seqs, sample=4, seed=nl)
        seen.update(int(ann.globals(i).n_limbs) for i in range(len(seqs)))
        rescanned += ann.drop_stats()["rescanned"]
        ann.close()
    assert {4, 8, 17} <= seen and rescanned > 0


def test_cross_winners_are_checked(pa):
    """Slots won by a cross candidate that only step 4 attains, with their delta chains kept in the path (phx_replacement_stats): found
    batch by batch among the benchmark contigs, then every contig that has one (each run alone: the bytes do not depend on the batch) is
    checked in full — properties 1-4 on every record, W(R_g) = D_{-g} exactly on a sample."""
    seqs = [pa.synth_contig(s, 50000) for s in range(1000)]
    ann = pa.Annotator()
    found, kept = [], 0
    for lo in range(0, 1000, 100):
        ann.upload(seqs[lo:lo + 100])
        ann.run()
        ann.replacements()
        if ann.replacement_stats()["cross"] == 0:
            continue
        for i in range(lo, lo + 100):
            ann.upload([seqs[i]])
            ann.run()
            ann.replacements()
            st = ann.replacement_stats()
            if st["cross"]:
                found.append(i)
                kept += st["cross_kept"]
                assert st["chain_nodes"] >= st["cross"]
                run_and_check(ann, [seqs[i]], sample=2, seed=i)
        if len(found) >= 2 and kept:
            break
    assert found and kept > 0, (found, kept)
    ann.close()


REGROW_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import phanotate_amd as pa
seqs = [pa.synth_contig(s, 50000) for s in range(1000)]
ann = pa.Annotator()
ann.upload(seqs)
ann.run()
out = ann.replacements()
print(json.dumps({"bytes": [x.tobytes().hex() for x in out], "stats": ann.replacement_stats()}))
"""


def test_delta_chain_buffer_regrowth(pa):
    """The delta-chain buffer starts with room for one node (env PHX_REPL_CHAIN_CAP=1, a fresh child process): the host grows it, runs
    the cross winners again, and the bytes equal a run whose buffer was large enough."""
    outs = []
    for env in ({}, {"PHX_REPL_CHAIN_CAP": "1"}):
        r = subprocess.run([sys.executable, "-c", REGROW_CHILD, ROOT], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    a, b = outs
    assert a["stats"]["regrown"] == 0 and b["stats"]["regrown"] == 1 and a["stats"]["chain_nodes"] > 1
    assert a["bytes"] == b["bytes"] and a["stats"] == dict(b["stats"], regrown=0)


LAYERED_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tools"); sys.path.insert(0, sys.argv[1] + "/tests")
import phanotate_amd as pa, fuzz_gpu
import test_replace_gpu as t
rng = np.random.RandomState(101)
seqs = [fuzz_gpu.make(rng) for _ in range(60)]
ann = pa.Annotator()
rst, roffs, rrec, genes, n = t.run_and_check(ann, seqs, full=set(range(0, 60, 3)), sample=2, seed=4)
print(json.dumps({"n": n, "layered": ann.drop_stats()["layered"], "recs": int(len(rrec))}))
"""


def test_layered_trees_keep_the_properties(pa):
    r = subprocess.run([sys.executable, "-c", LAYERED_CHILD, ROOT], capture_output=True, text=True, timeout=900, env=dict(os.environ, PHX_DROP_LAYERED="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["layered"] >= 40 and out["n"] > 10


def test_long_contigs(pa):
    seqs = [pa.synth_contig(5100, 60000), pa.synth_contig(5101, 12000), pa.synth_contig(5102, 400000)]
    ann = pa.Annotator()
    rst, roffs, rrec, genes, n = run_and_check(ann, seqs, sample=3, seed=5)
    assert (rst == 0).all() and ann.seg_runs() >= 1
    ann.close()


def test_mixed_statuses_and_neartie(pa):
    cyc = fuzz(949, 177)[176]
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops
    good = [pa.synth_contig(322, 9000).decode(), pa.synth_contig(323, 7000).decode()]
    bad = pa.synth_contig(324, 3000).decode()[:1500] + "x" + pa.synth_contig(324, 3000).decode()[1500:]
    seqs = [bad, "acg", cyc, unreachable, good[0], good[1]]
    ann = pa.Annotator()
    rst, roffs, rrec, genes, n = run_and_check(ann, seqs)
    assert rst.tolist() == [-2, -3, -9, 1, 0, 0] and n > 0
    ann.close()
    seen = set()
    for case in ("neartie_lo", "neartie_hi"):
        g, name, seq = load_golden(case)
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        run_and_check(ann, [seq])
        seen.add(int(ann.certified()[0]))
        ann.close()
    assert 2 in seen


def test_replacements_do_not_disturb_downloads_margins_or_drops(pa):
    a = fuzz(31, 30)
    ann = pa.Annotator()
    ann.upload(a)
    ann.run()
    before = as_bytes(ann.download_flat())
    d1 = as_bytes(ann.drop_margins())
    m1 = as_bytes(ann.margins())
    r1 = as_bytes(ann.replacements())  # drops first (without the trees), then the replacements
    assert as_bytes(ann.download_flat()) == before and as_bytes(ann.drop_margins()) == d1 and as_bytes(ann.margins()) == m1
    other = pa.Annotator()  # replacements first
    other.upload(a)
    other.run()
    assert as_bytes(other.replacements()) == r1
    assert as_bytes(other.drop_margins()) == d1 and as_bytes(other.margins()) == m1 and as_bytes(other.download_flat()) == before
    s1 = ann.drop_stats()
    assert other.drop_stats() == s1
    other.close()
    ann.close()


def test_pipeline_replacements_equal_per_batch_annotator(pa):
    from phanotate_amd.pipeline import Pipeline

    batches = [fuzz(40 + k, 20) for k in range(3)]
    with Pipeline(depth=2) as pipe:
        got = list(pipe.run(batches, drop_margins=True, replacements=True))
    assert all(len(x) == 5 for x in got)
    for bt, g in zip(batches, got):
        ann = pa.Annotator()
        want = ann.annotate_flat(bt)
        assert as_bytes(g[:3]) == as_bytes(want)
        assert as_bytes(g[3]) == as_bytes(ann.drop_margins()) and as_bytes(g[4]) == as_bytes(ann.replacements())
        ann.close()


def py_render(names, st, offs, rec, genes):
    def lst(g):
        if not len(g):
            return "-"
        return ",".join(("tRNA:" if abs(int(x["frame"])) == 4 else "") + ("%d..%d" % ((x["right"], x["left"]) if x["strand"] < 0 else (x["left"], x["right"]))) for x in g)

    out = []
    for i, nm in enumerate(names):
        if st[i] < 0:
            continue
        out.append("#id:\t%s\n#START\tSTOP\tFRAME\tCONTIG\tDROP\tREMOVED\tADDED\n" % nm)
        for x in rec[offs[i]:offs[i + 1]]:
            a, z = (x["right"], x["left"]) if x["strand"] < 0 else (x["left"], x["right"])
            g = genes[int(x["gene_off"]): int(x["gene_off"]) + int(x["n_removed"]) + int(x["n_added"])]
            out.append("%d\t%d\t%s\t%s\t%E\t%s\t%s\n" % (a, z, "+" if x["strand"] > 0 else "-", nm, float(x["drop"]), lst(g[: int(x["n_removed"])]), lst(g[int(x["n_removed"]):])))
    return "".join(out)


def test_cli_drop_replacements(pa, tmp_path):
    multi = tmp_path / "multi.fasta"
    seqs = {"c1": pa.synth_contig(71, 20000).decode(), "c2": pa.synth_contig(72, 9000).decode(), "bad": "acgtx" * 300, "c3": pa.synth_contig(73, 30000).decode()}
    multi.write_text("".join(">%s\n%s\n" % (k, v) for k, v in seqs.items()))
    cmd = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(multi)]
    out0 = subprocess.run(cmd, capture_output=True, timeout=600)
    rf, df = tmp_path / "r.tsv", tmp_path / "d.tsv"
    out1 = subprocess.run(cmd + ["--drop-replacements", str(rf), "--drop-margins", str(df)], capture_output=True, timeout=600)
    assert out0.returncode == out1.returncode and out0.stdout == out1.stdout
    rf2 = tmp_path / "r2.tsv"
    out2 = subprocess.run(cmd + ["--drop-replacements", str(rf2), "--batch-bases", "25000"], capture_output=True, timeout=600)
    assert out2.stdout == out0.stdout and rf2.read_bytes() == rf.read_bytes()
    ann = pa.Annotator()
    ann.upload(list(seqs.values()))
    ann.run()
    st, offs, rec, genes = ann.replacements()
    assert rf.read_text() == py_render(list(seqs), st, offs, rec, genes)
    assert len(rec) > 10 and "bad" not in rf.read_text()
    ann.close()


def test_benchmark_slice(pa):
    seqs = [pa.synth_contig(s, 50000) for s in range(1000)]
    rng = np.random.RandomState(1000)
    full = set(rng.choice(1000, 3, replace=False).tolist())
    ann = pa.Annotator()
    rst, roffs, rrec, genes, n = run_and_check(ann, seqs, full=full, sample=3, seed=3)
    assert (rst == 0).all() and len(rrec) > 50_000 and n >= 6
    assert ((rrec["bypass"] == 1) == (rrec["n_removed"] > 0)).all()
    ms = ann.replacements_ms()
    assert all(v > 0 for v in ms.values())
    ann.close()
