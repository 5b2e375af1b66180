"""Per-ORF path margins on the device (phx_margins_flat, phx_tap_dist_target) against python integers computed from the
device's own edges (phx_tap_edges: weight = trunc(w * 1000), edges.py:22), the way conftest.exact_dist_from_device_edges checks d_s,
but over the reversed edges: d_t(v) node for node, every record's margin bit for bit (float(delta) / 1000.0), reachability, the
invariants, status handling, create flags, non-interference with the run and the downloads, the pipeline and the CLI."""
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


def sweep_idx(v, V):  # the reverse pass's order: target, right to left, source (any order gives the same fixed point; this one is fast)
    return 0 if v == V - 1 else (V - 1 if v == V - 2 else V - 2 - v)


def py_dist_to_target(V, src, dst, w):
    """Bellman-Ford from the target over the reversed edges, python ints; None: no path to the target."""
    order = sorted(range(len(src)), key=lambda k: sweep_idx(src[k], V))
    d = [None] * V
    d[V - 1] = 0
    for _ in range(V + 1):
        ch = False
        for k in order:
            dv = d[dst[k]]
            if dv is None:
                continue
            c = dv + w[k]
            u = src[k]
            if d[u] is None or c < d[u]:
                d[u] = c
                ch = True
        if not ch:
            return d
    raise AssertionError("no fixed point: a cycle of negative length")


def device_graph(ann, i):
    ed = ann.edges(i)
    V = int(ann.globals(i).n_node)
    src, dst = ed["src"].tolist(), ed["dst"].tolist()
    w = [int(math.trunc(float(x) * 1000.0)) for x in ed["w"]]
    return V, src, dst, w, ed


def node_ids(ann, i):
    nd = ann.nodes(i)
    return {(int(p), int(t), 1 if f > 0 else -1): v for v, (p, t, f) in enumerate(zip(nd["pos"], nd["type"], nd["frame"])) if t in (0, 1) and abs(int(f)) <= 3}


def dt_ends(ann, i):
    """(d_t(source), d_t(target)) without converting every node (None: the contig has no graph)."""
    import ctypes as C

    g = ann.globals(i)
    nl, V = max(g.n_limbs, 1), int(g.n_node)
    if V <= 2:
        return None
    a = np.zeros((V, nl), np.uint64)
    assert ann.L.phx_tap_dist_target(ann.h, i, a.ctypes.data_as(C.c_void_p), a.size) == 0

    def val(row):
        x = sum(int(row[k]) << (64 * k) for k in range(nl))
        x = x - (1 << (64 * nl)) if x >> (64 * nl - 1) else x
        return None if x >= 1 << (64 * nl - 3) else x

    return val(a[V - 2]), val(a[V - 1])


def check_full(ann, i, st, rec, genes, cert):
    """d_t node for node, every record bit for bit, reachability, the invariants."""
    if ann.globals(i).n_node <= 2:  # no graph (phanotate.py:63): no distances are kept either way, no ORF, no record
        assert len(rec) == 0
        return check_invariants(i, st, rec, genes, cert)
    V, src, dst, w, ed = device_graph(ann, i)
    want_dt = py_dist_to_target(V, src, dst, w)
    got_dt = ann.dist_to_target(i)
    assert got_dt == want_dt, i
    ds = exact_dist_from_device_edges(ann, i)
    assert ann.dist(i) == ds, i
    D = ds[V - 1]
    assert want_dt[V - 2] == D and want_dt[V - 1] == 0
    orfs = ann.orfs(i)
    assert len(orfs) == len(rec), i
    ids = node_ids(ann, i)
    wmap = {(s, t): x for s, t, x in zip(src, dst, w)}
    for o, r in zip(orfs, rec):
        fwd = o["frame"] > 0
        sn = ids[(int(o["start"]), 0, 1 if fwd else -1)]
        tn = ids[(int(o["stop"]), 1, 1 if fwd else -1)]
        u, v = (sn, tn) if fwd else (tn, sn)
        assert (int(r["left"]), int(r["right"])) == ((int(o["start"]), int(o["stop"]) + 2) if fwd else (int(o["stop"]), int(o["start"]) + 2))
        assert int(r["frame"]) == int(o["frame"]) and int(r["strand"]) == (1 if fwd else -1) and float(r["score"]) == float(o["weight"])
        W = wmap[(u, v)]
        if D is None or ds[u] is None or want_dt[v] is None:
            assert r["through"] == 0 and r["margin"] == np.inf, (i, u, v)
        else:
            delta = ds[u] + W + want_dt[v] - D
            assert delta >= 0
            assert r["through"] == 1 and float(r["margin"]) == float(delta) / 1000.0, (i, u, v, delta, float(r["margin"]))
    check_invariants(i, st, rec, genes, cert)


def check_invariants(i, st, rec, genes, cert):
    assert (rec["margin"] >= 0).all(), i
    assert (rec["through"][~np.isfinite(rec["margin"])] == 0).all() and (np.isfinite(rec["margin"][rec["through"] == 1])).all()
    called = sorted((int(r["left"]), int(r["right"]), int(r["strand"])) for r in rec[rec["called"] == 1])
    want = sorted((int(g["left"]), int(g["right"]), int(g["strand"])) for g in genes if abs(int(g["frame"])) <= 3)
    assert called == want, i
    if st == 1:
        assert not rec["through"].any()
    if cert == 1:
        assert (rec["margin"][rec["called"] == 1] == 0.0).all(), i


def run_and_check(ann, seqs, full=None, trnas=None):
    """Annotate seqs on ann; full checks on the indices in `full` (all by default), invariants on every contig."""
    ann.upload(seqs)
    ann.set_trnas(trnas)
    ann.run()
    gst, goffs, genes = ann.download_flat()
    cert = ann.certified()
    mst, moffs, rec = ann.margins()
    for i in range(len(seqs)):
        if mst[i] < 0:
            assert moffs[i + 1] == moffs[i]
            continue
        assert mst[i] == gst[i]
        r, g = rec[moffs[i]:moffs[i + 1]], genes[goffs[i]:goffs[i + 1]]
        if full is None or i in full:
            check_full(ann, i, int(mst[i]), r, g, int(cert[i]))
        else:
            check_invariants(i, int(mst[i]), r, g, int(cert[i]))
            ends = dt_ends(ann, i)
            if ends is not None:
                assert ends[1] == 0 and (ends[0] == ann.path(i)[1] if mst[i] == 0 else ends[0] is None), i
    return mst, moffs, rec


def test_golden_fixtures(pa):
    """Every non-error golden fixture, the tRNA fixtures included (their path edges of frame +-4 get no record)."""
    n = 0
    for case in golden_cases():
        g, name, seq = load_golden(case)
        if str(g["error"]):
            continue
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        tr = golden_trnas(g)
        mst, moffs, rec = run_and_check(ann, [seq], trnas=None if tr is None else [tr])
        if case == "edge_huge":  # path sums beyond 1088 bits: no device distances
            assert mst.tolist() == [-7] and len(rec) == 0
        else:
            assert mst[0] >= 0, case
            n += 1
        ann.close()
    assert n >= 15


def test_fuzz_contigs_in_batches_and_lone(pa):
    seqs = fuzz(11, 210)
    ann = pa.Annotator()
    mst, moffs, rec = run_and_check(ann, seqs)
    assert (mst >= 0).sum() > 150
    for i in range(0, 210, 17):  # the same contig alone on a context: the same records, bit for bit
        lone = pa.Annotator()
        lone.upload([seqs[i]])
        lone.run()
        s1, o1, r1 = lone.margins()
        assert s1[0] == mst[i] and r1.tobytes() == rec[moffs[i]:moffs[i + 1]].tobytes(), i
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
    """Contigs whose path sums need 256, 512 and 1088 bits (the constructions of the wide-class tests in test_gpu_parity.py)."""
    rng = np.random.RandomState(3000)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    c256 = [pa.synth_contig(900 + k, 20000).decode() + "atg" + "".join(rng.choice(sense, 3000)) + "taa" + pa.synth_contig(1900 + k, 20000).decode() for k in range(6)]
    cases = [(c256, 2), ([wide_contig(pa, 8000, 8000, density=0.01)], 8), ([wide_contig(pa, 5500, 42)], 8), ([wide_contig(pa, 12000, 42)], 17)]
    seen = set()
    for seqs, nl in cases:
        ann = pa.Annotator()
        run_and_check(ann, seqs)
        limbs = [int(ann.globals(i).n_limbs) for i in range(len(seqs))]
        assert max(limbs) >= nl
        seen.update(limbs)
        ann.close()
    assert {4, 8, 17} <= seen


def test_long_contig_through_the_segments(pa):
    """A 60 kb contig in a small batch: its forward distances come from the segment solvers (phx_seg_runs)."""
    seqs = [pa.synth_contig(5100, 60000), pa.synth_contig(5101, 12000), pa.synth_contig(5102, 3000)]
    ann = pa.Annotator()
    run_and_check(ann, seqs)
    assert ann.seg_runs() >= 1
    ann.close()


def test_batch_of_720_contigs_side_streams(pa):
    seqs = fuzz(23, 720)
    rng = np.random.RandomState(77)
    sample = set(rng.choice(720, 40, replace=False).tolist())
    ann = pa.Annotator()
    run_and_check(ann, seqs, full=sample)
    ann.close()


def test_benchmark_slice(pa):
    """1000 benchmark contigs (synth_contig(seed, 50000)): full checks on a seeded sample, the invariants on all."""
    seqs = [pa.synth_contig(s, 50000) for s in range(1000)]
    rng = np.random.RandomState(1000)
    sample = set(rng.choice(1000, 6, replace=False).tolist())
    ann = pa.Annotator()
    mst, moffs, rec = run_and_check(ann, seqs, full=sample)
    assert (mst == 0).all() and len(rec) > 1_000_000
    ms = ann.margins_ms()
    assert set(ms) == {"transpose", "reverse", "margins", "download"} and all(v > 0 for v in ms.values())
    ann.close()


def test_equal_length_alternatives_have_uncalled_zero_margins(pa):
    """On the contigs of test_equal_length_alternatives_follow_the_reference_relaxation_order some paths tie: an ORF that is not
    called can still have margin 0."""
    seqs = fuzz(101, 300) + fuzz(7, 300)
    ann = pa.Annotator()
    n_tied_zero = 0
    for b0 in range(0, len(seqs), 100):
        part = seqs[b0:b0 + 100]
        ann.upload(part)
        ann.run()
        gst, goffs, genes = ann.download_flat()
        cert = ann.certified()
        mst, moffs, rec = ann.margins()
        for i in range(len(part)):
            if mst[i] < 0:
                continue
            r = rec[moffs[i]:moffs[i + 1]]
            check_invariants(b0 + i, int(mst[i]), r, genes[goffs[i]:goffs[i + 1]], int(cert[i]))
            if ann.globals(i).tie and ((r["called"] == 0) & (r["margin"] == 0.0)).any():
                n_tied_zero += 1
    assert n_tied_zero > 0
    ann.close()


def margins_of(pa, batches, flags=()):
    ann = pa.Annotator(flags=flags)
    out = []
    for seqs in batches:
        ann.upload(seqs)
        ann.run()
        st, offs, rec = ann.margins()
        out.append((st.tobytes(), offs.tobytes(), rec.tobytes(), [ann.dist_to_target(i) for i in range(min(2, len(seqs)))]))
    ann.close()
    return out


def test_create_flags_give_the_same_margins(pa):
    small = [pa.synth_contig(61, 14000), pa.synth_contig(62, 9000)]  # k_front, segments
    medium = fuzz(5, 40)
    want = margins_of(pa, [small, medium])
    for fl in ("solver_global", "solver_no_wave", "no_duo", "no_seg", "no_fuse", "one_stream", "poison"):
        assert margins_of(pa, [small, medium], (fl,)) == want, fl


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
    mst, moffs, rec = ann.margins()
    assert mst.tolist() == [-2, -3, -9, 1, -7, 0, 0]
    counts = np.diff(moffs).tolist()
    assert counts[:3] == [0, 0, 0] and counts[4] == 0 and counts[3] > 0
    r3 = rec[moffs[3]:moffs[4]]
    assert not r3["through"].any() and (r3["margin"] == np.inf).all()
    for k, i in enumerate((5, 6)):
        lone = pa.Annotator()
        lone.upload([good[k]])
        lone.run()
        s1, o1, r1 = lone.margins()
        assert s1[0] == 0 and r1.tobytes() == rec[moffs[i]:moffs[i + 1]].tobytes()
        assert lone.dist_to_target(0) == ann.dist_to_target(i)
        lone.close()
    ann.close()


def test_margins_do_not_disturb_the_run_or_the_downloads(pa):
    a, b = fuzz(31, 30), fuzz(32, 30)
    ann = pa.Annotator()
    ann.upload(a)
    ann.run()
    before = [x.tobytes() for x in ann.download_flat()]
    m1 = [x.tobytes() for x in ann.margins()]
    after = [x.tobytes() for x in ann.download_flat()]
    assert before == after
    assert [x.tobytes() for x in ann.margins()] == m1  # (cached: the same records again)
    fresh = pa.Annotator()
    assert [x.tobytes() for x in fresh.annotate_flat(a)] == before
    # a second run on the same context after a margins call = a fresh context
    ann.upload(b)
    ann.run()
    fb = pa.Annotator()
    assert [x.tobytes() for x in ann.download_flat()] == [x.tobytes() for x in fb.annotate_flat(b)]
    fb.upload(b)
    fb.run()
    mb = [x.tobytes() for x in fb.margins()]
    assert [x.tobytes() for x in ann.margins()] == mb
    # run_async, then margins: the call waits for the run
    ann.upload(a)
    ann.run_async()
    assert [x.tobytes() for x in ann.margins()] == m1
    assert [x.tobytes() for x in ann.download_flat()] == before
    for x in (ann, fresh, fb):
        x.close()


def test_pipeline_margins_equal_per_batch_annotator(pa):
    from phanotate_amd.pipeline import Pipeline

    batches = [fuzz(40 + k, 25) for k in range(4)]
    with Pipeline(depth=2) as pipe:
        got = list(pipe.run(batches, margins=True))
    with Pipeline(depth=2) as pipe:
        plain = list(pipe.run(batches))
    assert len(got) == 4 and all(len(x) == 4 for x in got) and all(len(x) == 3 for x in plain)
    for bt, g, p in zip(batches, got, plain):
        ann = pa.Annotator()
        want = ann.annotate_flat(bt)
        wm = ann.margins()
        assert [x.tobytes() for x in g[:3]] == [x.tobytes() for x in want] == [x.tobytes() for x in p]
        assert [x.tobytes() for x in g[3]] == [x.tobytes() for x in wm]
        ann.close()


def test_neartie_called_margins_within_the_certificate_bound(pa):
    """neartie_lo / _hi: the same contig under two -s weights 5e-28 apart; the host re-solve changes one of the two (certified 2).
    There a called ORF may carry a positive margin over the device's integers W, bounded by sum(|d1 + d2| + eps) over the edges of the
    device's path and the delivered path (phx_tap_edges' bounds on the reference's integers W*): the delivered path is optimal under W*."""
    seen = set()
    for case in ("neartie_lo", "neartie_hi"):
        g, name, seq = load_golden(case)
        ann = pa.Annotator(pa.make_params(**golden_params(g)))
        mst, moffs, rec = run_and_check(ann, [seq])
        cert = int(ann.certified()[0])
        seen.add(cert)
        V, src, dst, w, ed = device_graph(ann, 0)
        emap = {(s, t): k for k, (s, t) in enumerate(zip(src, dst))}

        def slack(k):
            if not ed["inexact"][k]:
                return 0
            err = float(ed["err"][k])
            assert math.isfinite(err)
            return abs(int(ed["d1"][k]) + int(ed["d2"][k])) + (0 if err == 0 else math.floor(err) + 1)

        dev_path = ann.path(0)[0].tolist()
        ids = node_ids(ann, 0)
        genes = ann.download_flat()[2]
        deliv = [V - 2]
        for x in genes:
            st = int(x["strand"])
            if st > 0:
                deliv += [ids[(int(x["left"]), 0, 1)], ids[(int(x["right"]) - 2, 1, 1)]]
            else:
                deliv += [ids[(int(x["left"]), 1, -1)], ids[(int(x["right"]) - 2, 0, -1)]]
        deliv.append(V - 1)
        bound = sum(slack(emap[(a, b)]) for p in (dev_path, deliv) for a, b in zip(p[:-1], p[1:]))
        called = rec[rec["called"] == 1]
        assert len(called) == len(genes)
        if cert == 1:
            assert (called["margin"] == 0.0).all()
        else:
            assert cert == 2 and (called["margin"] * 1000.0 <= bound * (1 + 1e-12)).all(), (case, called["margin"].max(), bound)
        ann.close()
    assert 2 in seen


def run_cli(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py")] + args, capture_output=True, timeout=600)
    return r.returncode, r.stdout


def parse_margins_file(path):
    blocks, cur = {}, None
    for line in open(path).read().splitlines():
        if line.startswith("#id:\t"):
            cur = blocks.setdefault(line[5:], [])
        elif line.startswith("#START"):
            assert line == "#START\tSTOP\tFRAME\tCONTIG\tSCORE\tMARGIN\tCALLED"
        else:
            cur.append(line.split("\t"))
    return blocks


def test_cli_margins(pa, tmp_path):
    import gzip

    from phanotate_amd.writers import FORMATS

    phix = os.path.join(GOLDEN, "phiX174.fasta.gz")
    multi = tmp_path / "multi.fasta"
    seqs = {"c1": pa.synth_contig(71, 20000).decode(), "c2": pa.synth_contig(72, 9000).decode(), "bad": "acgtx" * 300, "c3": pa.synth_contig(73, 30000).decode()}
    multi.write_text("".join(">%s\n%s\n" % (k, v) for k, v in seqs.items()))
    for fa in (phix, str(multi)):
        for fmt in FORMATS if fa != phix else ["tabular"]:
            rc0, out0 = run_cli([fa, "-f", fmt])
            mf = tmp_path / ("m_%s.tsv" % fmt)
            rc1, out1 = run_cli([fa, "-f", fmt, "--margins", str(mf)])
            assert rc0 == rc1 and out0 == out1, (fa, fmt)
            assert mf.exists()
        blocks = parse_margins_file(str(mf))
        # CALLED rows = the tabular genes
        rc, tab = run_cli([fa])
        tab_rows = {}
        cur = None
        for line in tab.decode().splitlines():
            if line.startswith("#id:\t"):
                cur = tab_rows.setdefault(line[5:], [])
            elif not line.startswith("#"):
                cur.append(tuple(line.split("\t")[:5]))
        assert set(blocks) == set(tab_rows)
        for name, rows in blocks.items():
            assert sorted(tuple(r[:5]) for r in rows if r[6] == "1") == sorted(tab_rows[name])
        # values = Annotator.margins()
        if fa == phix:
            with gzip.open(fa, "rt") as f:
                lines = f.read().split("\n")
            names, sq = [lines[0][1:].split()[0]], ["".join(lines[1:])]
        else:
            names, sq = list(seqs), list(seqs.values())
        ann = pa.Annotator()
        ann.upload(sq)
        ann.run()
        st, offs, rec = ann.margins()
        for i, nm in enumerate(names):
            if st[i] < 0:
                assert nm not in blocks
                continue
            r = rec[offs[i]:offs[i + 1]]
            r = r[r["through"] == 1]
            r = r[np.lexsort((r["strand"], r["right"], r["left"]))]
            want = [[str(x["right"] if x["strand"] < 0 else x["left"]), str(x["left"] if x["strand"] < 0 else x["right"]), "+" if x["strand"] > 0 else "-", nm,
                     "%E" % float(x["score"]), "%E" % float(x["margin"]), str(int(x["called"]))] for x in r]
            assert blocks[nm] == want, nm
        ann.close()
