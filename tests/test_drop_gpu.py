"""Gene drop margins on the device (phx_drop_margins_flat) against python integers over the device's own edges
(phx_tap_edges: weight = trunc(w * 1000), edges.py:22, as conftest.exact_dist_from_device_edges): for a called gene with stop node p_j,
D_{-g} is the shortest source -> target distance with p_j's edges removed and drop = float(D_{-g} - D) / 1000.0 bit for bit.  Also the
stop-node property the definition rests on, the wide classes, statuses, the layered trees, create flags, non-interference, the pipeline and
the CLI."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, exact_dist_from_device_edges, golden_cases, golden_params, golden_trnas, load_golden

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


def device_graph(ann, i):
    ed = ann.edges(i)
    V = int(ann.globals(i).n_node)
    return V, ed["src"].tolist(), ed["dst"].tolist(), [int(math.trunc(float(x) * 1000.0)) for x in ed["w"]]


def dist_without(V, src, dst, w, skip):
    """Shortest source -> target distance (python ints) with node `skip` and its edges removed; None: no path."""
    d = [None] * V
    d[V - 2] = 0
    for _ in range(V + 1):  # (edges grouped by destination in position order: a handful of sweeps)
        ch = False
        for k in range(len(src)):
            u, v = src[k], dst[k]
            if u == skip or v == skip or d[u] is None:
                continue
            c = d[u] + w[k]
            if d[v] is None or c < d[v]:
                d[v] = c
                ch = True
        if not ch:
            return d[V - 1]
    raise AssertionError("no fixed point")


def path_genes(ann, i):
    """The CDS genes of the device path in path order: (left, right, strand, frame, stop node)."""
    P = ann.path(i)[0].tolist()
    nd = ann.nodes(i)
    out = []
    for k in range((len(P) - 1) // 2):
        a, b = P[2 * k + 1], P[2 * k + 2]
        ta, fa, tb = int(nd["type"][a]), int(nd["frame"][a]), int(nd["type"][b])
        if ta == 0 and 1 <= fa <= 3 and tb == 1:
            stop = b
        elif ta == 1 and -3 <= fa <= -1 and tb == 0:
            stop = a
        else:
            continue  # (a tRNA pair)
        out.append((int(nd["pos"][a]), int(nd["pos"][b]) + 2, 1 if fa > 0 else -1, fa, stop))
    return out


def check_contig(ann, i, st, rec, genes, sample=None, rng=None):
    """Records = the CDS genes of the device path; drop / bypass exact for every gene (or `sample` of them); `called` = delivery."""
    pg = path_genes(ann, i) if st == 0 else []
    assert [(int(r["left"]), int(r["right"]), int(r["strand"]), int(r["frame"])) for r in rec] == [g[:4] for g in pg], i
    delivered = {(int(g["left"]), int(g["right"]), int(g["strand"])) for g in genes if abs(int(g["frame"])) <= 3}
    assert [int(r["called"]) for r in rec] == [int((g[0], g[1], g[2]) in delivered) for g in pg], i
    assert (rec["drop"] >= 0).all() and ((rec["bypass"] == 1) == np.isfinite(rec["drop"])).all()
    if not len(rec):
        return 0
    V, src, dst, w = device_graph(ann, i)
    ds = exact_dist_from_device_edges(ann, i)
    D = ds[V - 1]
    assert D == ann.path(i)[1]
    ks = range(len(pg))
    if sample is not None and len(pg) > sample:
        ks = sorted(rng.choice(len(pg), sample, replace=False).tolist())
    for k in ks:
        Dg = dist_without(V, src, dst, w, pg[k][4])
        r = rec[k]
        if Dg is None:
            assert r["bypass"] == 0 and r["drop"] == np.inf, (i, k)
        else:
            assert Dg >= D
            assert r["bypass"] == 1 and float(r["drop"]) == float(Dg - D) / 1000.0, (i, k, Dg - D, float(r["drop"]))
    return len(ks)


def run_and_check(ann, seqs, full=None, trnas=None, sample=None, seed=0):
    ann.upload(seqs)
    ann.set_trnas(trnas)
    ann.run()
    gst, goffs, genes = ann.download_flat()
    dst_, doffs, rec = ann.drop_margins()
    rng = np.random.RandomState(seed)
    for i in range(len(seqs)):
        if dst_[i] != 0:
            assert doffs[i + 1] == doffs[i]
            if dst_[i] < 0 and gst[i] < 0:
                assert dst_[i] == gst[i]
            continue
        assert gst[i] == 0
        if full is None or i in full:
            check_contig(ann, i, int(dst_[i]), rec[doffs[i]:doffs[i + 1]], genes[goffs[i]:goffs[i + 1]], sample, rng)
    return dst_, doffs, rec


def check_stop_property(ann, i):
    """In-edges of a forward stop and out-edges of a reverse stop are exactly the ORF edges of its group (functions.py:311-318)."""
    V, src, dst, w = device_graph(ann, i)
    nd = ann.nodes(i)
    orfs = ann.orfs(i)
    ids = {(int(p), int(t), 1 if f > 0 else -1): v for v, (p, t, f) in enumerate(zip(nd["pos"], nd["type"], nd["frame"])) if t in (0, 1) and abs(int(f)) <= 3}
    groups = {}
    for o in orfs:
        fwd = o["frame"] > 0
        stop = ids[(int(o["stop"]), 1, 1 if fwd else -1)]
        start = ids[(int(o["start"]), 0, 1 if fwd else -1)]
        groups.setdefault(stop, set()).add((start, stop) if fwd else (stop, start))
    ins, outs = {}, {}
    for u, v in zip(src, dst):
        ins.setdefault(v, set()).add((u, v))
        outs.setdefault(u, set()).add((u, v))
    for stop, es in groups.items():
        fwd = int(nd["frame"][stop]) > 0
        assert (ins.get(stop, set()) if fwd else outs.get(stop, set())) == es, (i, stop)
    return len(groups)


def test_golden_fixtures(pa):
    """Every non-error golden fixture, the tRNA fixtures included (their tRNA pairs get no record); the stop-node property on each."""
    n = 0
    for case in golden_cases():
        g, name, seq = load_golden(case)
        if str(g["error"]):
            continue
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        tr = golden_trnas(g)
        st, offs, rec = run_and_check(ann, [seq], trnas=None if tr is None else [tr])
        if case == "edge_huge":
            assert st.tolist() == [-7] and len(rec) == 0
        else:
            assert st[0] >= 0, case
            if int(ann.globals(0).n_node) > 2:
                check_stop_property(ann, 0)
            n += 1
        ann.close()
    assert n >= 15


def test_fuzz_contigs_in_batches_and_lone(pa):
    seqs = fuzz(11, 120)
    ann = pa.Annotator()
    st, offs, rec = run_and_check(ann, seqs, sample=12, seed=1)
    assert (st == 0).sum() > 80
    stats = ann.drop_stats()
    assert stats["slots"] == len(rec)
    for i in range(0, 120, 13):
        lone = pa.Annotator()
        lone.upload([seqs[i]])
        lone.run()
        s1, o1, r1 = lone.drop_margins()
        assert s1[0] == st[i] and r1.tobytes() == rec[offs[i]:offs[i + 1]].tobytes(), i
        lone.close()
    ann.close()


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


def test_wide_integer_classes(pa):
    """The 256 / 512 / 1088-bit constructions of test_margins_gpu.py: exact, and their saturated slots rescanned."""
    rng = np.random.RandomState(3000)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    c256 = [pa.synth_contig(900 + k, 20000).decode() + "atg" + "".join(rng.choice(sense, 3000)) + "taa" + pa.synth_contig(1900 + k, 20000).decode() for k in range(6)]
    cases = [(c256, 2), ([wide_contig(pa, 8000, 8000, density=0.01)], 8), ([wide_contig(pa, 5500, 42)], 8), ([wide_contig(pa, 12000, 42)], 17)]
    seen, rescanned = set(), 0
    for seqs, nl in cases:
        ann = pa.Annotator()
        run_and_check(ann, seqs, sample=10, seed=nl)
        limbs = [int(ann.globals(i).n_limbs) for i in range(len(seqs))]
        assert max(limbs) >= nl
        seen.update(limbs)
        rescanned += ann.drop_stats()["rescanned"]
        ann.close()
    assert {4, 8, 17} <= seen
    assert rescanned > 0


def drops_of(pa, batches, flags=()):
    ann = pa.Annotator(flags=flags)
    out = []
    for seqs in batches:
        ann.upload(seqs)
        ann.run()
        out.append([x.tobytes() for x in ann.drop_margins()])
    ann.close()
    return out


def test_create_flags_give_the_same_drops(pa):
    small = [pa.synth_contig(61, 14000), pa.synth_contig(62, 9000)]
    medium = fuzz(5, 40)
    want = drops_of(pa, [small, medium])
    for fl in ("no_seg", "solver_no_wave", "no_duo"):
        assert drops_of(pa, [small, medium], (fl,)) == want, fl


def test_long_contigs_segments_and_global_table(pa):
    """A 60 kb contig through the segment solvers; a 400 kb one whose sparse table is beyond LDS (the global-memory table)."""
    seqs = [pa.synth_contig(5100, 60000), pa.synth_contig(5101, 12000), pa.synth_contig(5102, 400000)]
    ann = pa.Annotator()
    st, offs, rec = run_and_check(ann, seqs, sample=8, seed=5)
    assert ann.seg_runs() >= 1
    n_path = len(ann.path(2)[0])
    assert n_path * (int(math.log2(n_path)) + 1) > 4096 and (st == 0).all()
    ann.close()


def test_batch_of_720_contigs(pa):
    seqs = fuzz(23, 720)
    rng = np.random.RandomState(77)
    sample = set(rng.choice(720, 25, replace=False).tolist())
    ann = pa.Annotator()
    run_and_check(ann, seqs, full=sample, sample=6, seed=2)
    ann.close()


def test_benchmark_slice(pa):
    seqs = [pa.synth_contig(s, 50000) for s in range(1000)]
    rng = np.random.RandomState(1000)
    sample = set(rng.choice(1000, 4, replace=False).tolist())
    ann = pa.Annotator()
    st, offs, rec = run_and_check(ann, seqs, full=sample, sample=6, seed=3)
    assert (st == 0).all() and len(rec) > 50_000
    ms = ann.drop_ms()
    assert set(ms) == {"trees", "candidates", "fixups", "download"} and all(v > 0 for v in ms.values())
    ann.close()


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
st, offs, rec = ann.drop_margins()
print(json.dumps({"st": st.tolist(), "offs": offs.tolist(), "rec": rec.tobytes().hex(), "stats": ann.drop_stats()}))
"""


def test_cross_nodes_and_layered_trees(pa):
    """Step 4 runs on real contigs (equal-length alternatives and backward edges), and forcing the layered trees (PHX_DROP_LAYERED=1,
    in a fresh child process) gives the same records."""
    outs = []
    for env in ({}, {"PHX_DROP_LAYERED": "1"}):
        r = subprocess.run([sys.executable, "-c", LAYERED_CHILD, ROOT], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    a, b = outs
    assert a["st"] == b["st"] and a["offs"] == b["offs"] and a["rec"] == b["rec"]
    assert b["stats"]["layered"] >= 100 and a["stats"]["slots"] == b["stats"]["slots"] == len(a["rec"]) // 80
    seqs = fuzz(101, 150)
    ann = pa.Annotator()
    run_and_check(ann, seqs, full=set(range(0, 150, 5)), sample=8, seed=9)
    cross = ann.drop_stats()["cross"]
    ann.close()
    assert cross > 0 or a["stats"]["cross"] > 0


def test_status_handling_in_one_mixed_batch(pa):
    cyc = fuzz(949, 177)[176]
    dense_stops = "".join("tagctaactgattaa"[i % 15] for i in range(2700))
    unreachable = dense_stops + pa.synth_contig(77, 1500).decode() + dense_stops
    rng = np.random.RandomState(12)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    huge = pa.synth_contig(320, 2000).decode() + "atg" + "".join(sense[i] for i in rng.randint(0, len(sense), 24000)) + "taa" + pa.synth_contig(321, 2000).decode()
    good = [pa.synth_contig(322, 9000).decode(), pa.synth_contig(323, 7000).decode()]
    bad = pa.synth_contig(324, 3000).decode()[:1500] + "x" + pa.synth_contig(324, 3000).decode()[1500:]
    seqs = [bad, "acg", cyc, unreachable, huge, good[0], good[1]]
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    st, offs, rec = ann.drop_margins()
    assert st.tolist() == [-2, -3, -9, 1, -7, 0, 0]
    assert np.diff(offs).tolist()[:5] == [0] * 5 and offs[7] > offs[5]
    for k, i in enumerate((5, 6)):
        lone = pa.Annotator()
        lone.upload([good[k]])
        lone.run()
        s1, o1, r1 = lone.drop_margins()
        assert s1[0] == 0 and r1.tobytes() == rec[offs[i]:offs[i + 1]].tobytes()
        lone.close()
    ann.close()


def test_neartie_records_follow_the_device_path(pa):
    seen = set()
    for case in ("neartie_lo", "neartie_hi"):
        g, name, seq = load_golden(case)
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        run_and_check(ann, [seq])
        seen.add(int(ann.certified()[0]))
        ann.close()
    assert 2 in seen


def test_drops_do_not_disturb_the_run_the_downloads_or_the_margins(pa):
    a, b = fuzz(31, 30), fuzz(32, 30)
    ann = pa.Annotator()
    ann.upload(a)
    ann.run()
    before = [x.tobytes() for x in ann.download_flat()]
    d1 = [x.tobytes() for x in ann.drop_margins()]
    m1 = [x.tobytes() for x in ann.margins()]  # drops first, then margins
    assert [x.tobytes() for x in ann.download_flat()] == before
    assert [x.tobytes() for x in ann.drop_margins()] == d1
    ms = ann.margins_ms()
    assert all(v > 0 for v in ms.values())
    other = pa.Annotator()  # margins first, then drops
    other.upload(a)
    other.run()
    assert [x.tobytes() for x in other.margins()] == m1
    assert [x.tobytes() for x in other.drop_margins()] == d1
    assert [x.tobytes() for x in other.margins()] == m1
    other.close()
    ann.upload(b)
    ann.run()
    fb = pa.Annotator()
    assert [x.tobytes() for x in ann.download_flat()] == [x.tobytes() for x in fb.annotate_flat(b)]
    assert [x.tobytes() for x in ann.drop_margins()] == [x.tobytes() for x in fb.drop_margins()]
    ann.upload(a)
    ann.run_async()
    assert [x.tobytes() for x in ann.drop_margins()] == d1
    assert [x.tobytes() for x in ann.download_flat()] == before
    for x in (ann, fb):
        x.close()


def test_pipeline_drops_equal_per_batch_annotator(pa):
    from phanotate_amd.pipeline import Pipeline

    batches = [fuzz(40 + k, 20) for k in range(3)]
    with Pipeline(depth=2) as pipe:
        got = list(pipe.run(batches, margins=True, drop_margins=True))
    with Pipeline(depth=2) as pipe:
        only = list(pipe.run(batches, drop_margins=True))
    assert all(len(x) == 5 for x in got) and all(len(x) == 4 for x in only)
    for bt, g, o in zip(batches, got, only):
        ann = pa.Annotator()
        want = ann.annotate_flat(bt)
        wm, wd = ann.margins(), ann.drop_margins()
        assert [x.tobytes() for x in g[:3]] == [x.tobytes() for x in want] == [x.tobytes() for x in o[:3]]
        assert [x.tobytes() for x in g[3]] == [x.tobytes() for x in wm]
        assert [x.tobytes() for x in g[4]] == [x.tobytes() for x in wd] == [x.tobytes() for x in o[3]]
        ann.close()


def test_cli_drop_margins(pa, tmp_path):
    multi = tmp_path / "multi.fasta"
    seqs = {"c1": pa.synth_contig(71, 20000).decode(), "c2": pa.synth_contig(72, 9000).decode(), "bad": "acgtx" * 300, "c3": pa.synth_contig(73, 30000).decode()}
    multi.write_text("".join(">%s\n%s\n" % (k, v) for k, v in seqs.items()))
    out0 = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(multi)], capture_output=True, timeout=600)
    df = tmp_path / "d.tsv"
    out1 = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(multi), "--drop-margins", str(df)], capture_output=True, timeout=600)
    assert out0.returncode == out1.returncode and out0.stdout == out1.stdout
    df2 = tmp_path / "d2.tsv"
    out2 = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), str(multi), "--drop-margins", str(df2), "--batch-bases", "25000"], capture_output=True, timeout=600)
    assert out2.stdout == out0.stdout and df2.read_bytes() == df.read_bytes()  # several batches: the pipeline
    ann = pa.Annotator()
    ann.upload(list(seqs.values()))
    ann.run()
    st, offs, rec = ann.drop_margins()
    want = []
    for i, nm in enumerate(seqs):
        if st[i] < 0:
            continue
        want.append("#id:\t%s\n#START\tSTOP\tFRAME\tCONTIG\tSCORE\tDROP\tCALLED\n" % nm)
        for x in rec[offs[i]:offs[i + 1]]:
            a, z = (x["right"], x["left"]) if x["strand"] < 0 else (x["left"], x["right"])
            want.append("%d\t%d\t%s\t%s\t%E\t%E\t%d\n" % (a, z, "+" if x["strand"] > 0 else "-", nm, float(x["score"]), float(x["drop"]), int(x["called"])))
    assert df.read_text() == "".join(want)
    assert "bad" not in df.read_text() and len(rec) > 10
    ann.close()
