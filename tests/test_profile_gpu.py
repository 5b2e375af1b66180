"""Coding profiles on the device (phx_profile_flat) against python integers from the device's own taps: phx_tap_edges with
W = trunc(w * 1000), phx_tap_nodes, phx_tap_dist and phx_tap_dist_target, which existing tests pin.  Per edge Delta = d_s(u) + W + d_t(v)
- D, its track by its tail and its slot range; per slot and track the exact minimum Delta gives float(Delta) / 1000.0, bit-equal to the
record.  Then the invariants, batches against lone uploads, non-interference with the other analyses, caching, and the command line."""
import gzip
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_cases, golden_params, golden_trnas, load_golden

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

INF = float("inf")
FULL_FAMILIES = ("edge_", "param_", "trna_gap", "trna_duplicate", "trna_phiX174", "neartie_", "synth6k_", "phiX174")
FULL_CASES = [c for c in golden_cases() if c.startswith(FULL_FAMILIES)] + ["synth50k_0"]  # synth50k_0: the one contig past the LDS threshold
TRACKS = ("fwd", "rev", "gap")


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def fuzz(seed, n):
    import fuzz_gpu

    rng = np.random.RandomState(seed)
    return [fuzz_gpu.make(rng) for _ in range(n)]


def is_open(nd, v, V):
    """an open node, as the graph stage and emit_genes tell it: forward start or reverse stop (tRNA nodes alike); on the bipartition's
    sides the target stands with the open nodes (connectors end in it), the source with the close nodes"""
    if v >= V - 2:
        return v == V - 1
    t, f = int(nd["type"][v]), int(nd["frame"][v])
    return (t == 0 and f > 0) or (t == 1 and f < 0)


def rank(v, V):
    return v if v < V - 2 else (-1 if v == V - 2 else V - 2)


def paint_min(n, items):
    """per slot the minimum over items = [(value, a, z)] covering the slots a..z (None: none): ascending values paint what is still free"""
    out = [None] * n
    nxt = list(range(n + 1))

    def find(s):
        while nxt[s] != s:
            nxt[s] = nxt[nxt[s]]
            s = nxt[s]
        return s

    for val, a, z in sorted(items):
        s = find(a)
        while s <= z:
            out[s] = val
            nxt[s] = s + 1
            s = find(s + 1)
    return out


def edge_deltas(ann, i):
    """[(track, Delta or None, a, z, u, v)] of every edge of contig i from the taps (a > z: it covers nothing), with the bipartition checked"""
    V = int(ann.globals(i).n_node)
    nd, ed = ann.nodes(i), ann.edges(i)
    ds, dt = ann.dist(i), ann.dist_to_target(i)
    D = ds[V - 1]
    assert dt[V - 2] == D and dt[V - 1] == 0 and ds[V - 2] == 0
    out = []
    for u, v, w in zip(ed["src"].tolist(), ed["dst"].tolist(), ed["w"].tolist()):
        ou, ov = is_open(nd, u, V), is_open(nd, v, V)
        assert ou != ov and u != V - 1 and v != V - 2, (i, u, v)  # open tail => close head, and the other way round
        track = 2 if not ou else (0 if int(nd["frame"][u]) > 0 else 1)
        W = int(math.trunc(float(w) * 1000.0))
        delta = None if D is None or ds[u] is None or dt[v] is None else ds[u] + W + dt[v] - D
        assert delta is None or delta >= 0
        out.append((track, delta, rank(u, V) + 1, rank(v, V), u, v))
    return out


def check_bounds(ann, i, L, rec):
    """V - 1 records; lo / hi are the neighbouring nodes' pos, 0 and L + 1 at the ends"""
    V = int(ann.globals(i).n_node)
    assert len(rec) == V - 1, (i, len(rec), V)
    pos = ann.nodes(i)["pos"][: V - 2].astype(np.int64)
    assert (np.diff(pos) >= 0).all()
    assert np.array_equal(rec["lo"], np.concatenate([[0], pos])) and np.array_equal(rec["hi"], np.concatenate([pos, [L + 1]])), i


def check_full(ann, i, L, st, rec):
    """every value of every slot, bit for bit"""
    check_bounds(ann, i, L, rec)
    n = len(rec)
    items = ([], [], [])
    for track, delta, a, z, u, v in edge_deltas(ann, i):
        if delta is not None and a <= z:
            items[track].append((delta, a, z))
    for t, name in enumerate(TRACKS):
        want = np.array([INF if d is None else float(d) / 1000.0 for d in paint_min(n, items[t])])
        assert want.tobytes() == rec[name].astype(np.float64).tobytes(), (i, name, np.flatnonzero(want != rec[name])[:5])
    if st == 1:
        assert not any(items)


def check_invariants(ann, i, L, st, rec, mrec):
    """what must hold without the taps' integers; mrec: the contig's margins() records"""
    check_bounds(ann, i, L, rec)
    vals = np.stack([rec[k] for k in TRACKS])
    assert not np.isnan(vals).any() and (vals >= 0).all(), i
    if st == 1:
        assert np.isinf(vals).all(), i
        return
    assert st == 0 and (vals.min(axis=0) == 0.0).all(), i  # the device path crosses every slot
    # the gene tracks are the slice minima of the margins() records with through == 1 (each is <= its strand's track on every slot it
    # covers, and every finite value is attained), together with the tRNA edges, which have no record
    V = int(ann.globals(i).n_node)
    nd = ann.nodes(i)
    ids = {(int(p), int(t), 1 if f > 0 else -1): v for v, (p, t, f) in enumerate(zip(nd["pos"][: V - 2], nd["type"][: V - 2], nd["frame"][: V - 2])) if abs(int(f)) <= 3}
    want = np.full((2, V - 1), INF)
    for r in mrec[mrec["through"] == 1]:
        s = int(r["strand"])
        u, v = ids[(int(r["left"]), 0 if s > 0 else 1, s)], ids[(int(r["right"]) - 2, 1 if s > 0 else 0, s)]
        assert u < v
        k = 0 if s > 0 else 1
        assert (vals[k, u + 1:v + 1] <= r["margin"]).all(), (i, u, v)
        np.minimum(want[k, u + 1:v + 1], r["margin"], out=want[k, u + 1:v + 1])
    if (np.abs(nd["frame"][: V - 2].astype(int)) == 4).any():
        for track, delta, a, z, u, v in edge_deltas(ann, i):
            if track < 2 and abs(int(nd["frame"][u])) == 4 and delta is not None and a <= z:
                np.minimum(want[track, a:z + 1], float(delta) / 1000.0, out=want[track, a:z + 1])
    assert want.tobytes() == vals[:2].tobytes(), (i, np.argwhere(want != vals[:2])[:5])


def annotate(pa, case):
    """(ann, L, status, records, margins' records) of a golden fixture under its own params and tRNAs"""
    g, name, seq = load_golden(case)
    ann = pa.Annotator(pa.make_params(**golden_params(g)))
    ann.upload([seq])
    tr = golden_trnas(g)
    ann.set_trnas(None if tr is None else [tr])
    ann.run()
    ann.download_flat()  # (the certificate and, where it fails, the host re-solve: certified() then reports 2)
    st, offs, rec = ann.profile()
    mst, moffs, mrec = ann.margins()
    assert st.tolist() == mst.tolist() and offs[0] == 0
    return ann, len(seq), int(st[0]), rec, mrec


SEEN = {}


@pytest.mark.parametrize("case", FULL_CASES)
def test_golden_full(pa, case):
    ann, L, st, rec, mrec = annotate(pa, case)
    V, cert = int(ann.globals(0).n_node), int(ann.certified()[0])
    SEEN[case] = (st, V, cert)
    if st < 0 or V <= 2:  # a run error, no device distances (edge_huge) or no graph (edge_L5 / L6): no records
        assert len(rec) == 0
    else:
        check_full(ann, 0, L, st, rec)
        check_invariants(ann, 0, L, st, rec, mrec)
    ann.close()


def seen(pa, case):
    if case not in SEEN:
        ann, L, st, rec, mrec = annotate(pa, case)
        SEEN[case] = (st, int(ann.globals(0).n_node), int(ann.certified()[0]))
        ann.close()
    return SEEN[case]


def test_golden_full_covered_the_shapes(pa):
    """the shapes the fixtures are there for were met: an error, no graph, no device distances, a certified-2 contig, the table in LDS and
    in global memory"""
    assert seen(pa, "edge_L5")[0] == -3 and seen(pa, "edge_L6")[1] <= 2 and seen(pa, "edge_huge")[0] == -7 and seen(pa, "trna_duplicate")[0] == -6
    assert 2 in (seen(pa, "neartie_lo")[2], seen(pa, "neartie_hi")[2])
    cells = lambda n: n * n.bit_length()  # n (floor(log2 n) + 1)
    assert seen(pa, "synth50k_0")[0] == 0 and cells(seen(pa, "synth50k_0")[1] - 1) > 4096
    assert sum(1 for st, V, _ in (seen(pa, c) for c in FULL_CASES) if st >= 0 and V > 2 and cells(V - 1) <= 4096) >= 20


def test_status_handling_in_one_mixed_batch(pa):
    """test_margins_gpu's mixed batch: a bad letter, a contig too short, a cycle of negative length, a graph without a path, path sums
    beyond the widest class, and two good contigs whose records are the lone upload's"""
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
    st, offs, rec = ann.profile()
    mst, moffs, mrec = ann.margins()
    assert st.tolist() == mst.tolist() == [-2, -3, -9, 1, -7, 0, 0]
    counts = np.diff(offs).tolist()
    assert counts[:3] == [0, 0, 0] and counts[4] == 0 and counts[3] == int(ann.globals(3).n_node) - 1 > 0
    r3 = rec[offs[3]:offs[4]]
    assert all(np.isinf(r3[k]).all() for k in TRACKS)  # no path: V - 1 records, every value +inf
    check_full(ann, 3, len(seqs[3]), 1, r3)
    check_invariants(ann, 3, len(seqs[3]), 1, r3, mrec[moffs[3]:moffs[4]])
    for k, i in enumerate((5, 6)):
        r = rec[offs[i]:offs[i + 1]]
        assert (0, r.tobytes()) == lone(pa, good[k])
        check_full(ann, i, len(seqs[i]), 0, r)
        check_invariants(ann, i, len(seqs[i]), 0, r, mrec[moffs[i]:moffs[i + 1]])
    ann.close()


def lone(pa, seq):
    a = pa.Annotator()
    a.upload([seq])
    a.run()
    st, offs, rec = a.profile()
    a.close()
    return int(st[0]), rec.tobytes()


def test_batches_equal_lone_uploads(pa):
    phix = load_golden("phiX174")[2]
    tiny = load_golden("edge_L5")[2]
    first = fuzz(41, 20)
    first[10:10] = [tiny, phix]
    second = fuzz(42, 6) + [phix]
    ann = pa.Annotator()
    for seqs, check in ((first, range(len(first))), (second, range(len(second)))):  # the second batch must not see the first's tables
        ann.upload(seqs)
        ann.run()
        st, offs, rec = ann.profile()
        mst, moffs, mrec = ann.margins()
        assert st.tolist() == mst.tolist() and offs[0] == 0 and offs[-1] == len(rec)
        for i in check:
            r = rec[offs[i]:offs[i + 1]]
            assert (int(st[i]), r.tobytes()) == lone(pa, seqs[i]), i
            V = int(ann.globals(i).n_node)
            assert len(r) == (V - 1 if st[i] >= 0 and V > 2 else 0), i
            if len(r):
                check_invariants(ann, i, len(seqs[i]), int(st[i]), r, mrec[moffs[i]:moffs[i + 1]])
    assert st[-1] == 0
    check_full(ann, len(second) - 1, len(phix), 0, rec[offs[-2]:offs[-1]])
    ann.close()


def triple_bytes(t):
    return tuple(np.ascontiguousarray(x).tobytes() for x in t)


def test_profile_does_not_disturb_the_other_analyses_and_is_cached(pa):
    seqs = fuzz(51, 12) + [load_golden("phiX174")[2]]
    a, b = pa.Annotator(), pa.Annotator()
    for x in (a, b):
        x.upload(seqs)
        x.run()
    # a: the profile first; b: the margins and the drop margins first
    p1 = triple_bytes(a.profile())
    ms1 = a.profile_ms()
    assert ms1["tables"] > 0
    ga = triple_bytes(a.download_flat())
    ma, da = triple_bytes(a.margins()), triple_bytes(a.drop_margins())
    p2 = triple_bytes(a.profile())
    assert a.profile_ms() == ms1  # the cached records: nothing was computed again
    gb = triple_bytes(b.download_flat())
    mb, db = triple_bytes(b.margins()), triple_bytes(b.drop_margins())
    mms, dms = b.margins_ms(), b.drop_ms()
    p3 = triple_bytes(b.profile())
    assert p1 == p2 == p3 and ma == mb and da == db and ga == gb
    assert triple_bytes(b.margins()) == mb and triple_bytes(b.drop_margins()) == db and b.margins_ms() == mms and b.drop_ms() == dms
    assert triple_bytes(b.download_flat()) == gb
    # a new upload + run invalidates
    other = fuzz(52, 5)
    a.upload(other)
    with pytest.raises(pa.PhxError):
        a.profile()  # (before the run: a call sequence error)
    a.run()
    st, offs, rec = a.profile()
    assert len(st) == 5
    for i in range(5):
        assert (int(st[i]), rec[offs[i]:offs[i + 1]].tobytes()) == lone(pa, other[i]), i
    a.close()
    b.close()


def test_cli_profile(pa, tmp_path):
    from phanotate_amd import cli

    phix = os.path.join(GOLDEN, "phiX174.fasta.gz")
    out = tmp_path / "profile.tsv"
    run = lambda args: subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py")] + args, capture_output=True, timeout=600)
    r0, r1 = run([phix]), run([phix, "--profile", str(out)])
    assert r0.returncode == 0 and r1.returncode == 0, r1.stderr[-2000:]
    assert r0.stdout == r1.stdout and len(r0.stdout) > 0
    with gzip.open(phix, "rt") as f:
        lines = f.read().split("\n")
    name, seq = lines[0][1:].split()[0], "".join(lines[1:])
    ann = pa.Annotator()
    ann.upload([seq])
    ann.run()
    st, offs, rec = ann.profile()
    ann.close()
    text = cli.format_profile([name], st, offs, rec)
    assert out.read_bytes() == text
    rows = text.decode().splitlines()
    assert rows[0] == "#id:\t" + name and rows[1] == "#LO\tHI\tFWD\tREV\tGAP" and len(rows) > 10
    assert rows[2].split("\t")[0] == "0" and rows[-1].split("\t")[1] == str(len(seq) + 1)
