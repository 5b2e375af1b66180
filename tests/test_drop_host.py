"""Host side of the gene drop margins (no GPU): the algorithm of DESIGN.md §12 restated in Python against brute force on random cyclic
graphs (zero-weight cycles, equal-length ties, random tie choices in T_t), the C formatter of --drop-margins FILE against a plain Python
rendering, the CLI's refusals, and the new entry points in the header and the export list."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def lib():
    from phanotate_amd import _lib

    return _lib


# ---- the algorithm, restated ----

def bellman_ford(V, edges, s, skip=None, reverse=False):
    d = [None] * V
    d[s] = 0
    for _ in range(V + 1):
        ch = False
        for u, v, w in edges:
            if reverse:
                u, v = v, u
            if skip is not None and (u == skip or v == skip) or d[u] is None:
                continue
            if d[v] is None or d[u] + w < d[v]:
                d[v] = d[u] + w
                ch = True
        if not ch:
            return d
    raise AssertionError("negative cycle")


def shortest_path(V, edges, ds, s, t):
    """A shortest s -> t path by the lowest-index tight in-edge, walked back from t; None when that walk closes a cycle."""
    path, v, seen = [t], t, {t}
    while v != s:
        u = next(a for a, b, w in edges if b == v and ds[a] is not None and ds[a] + w == ds[v])
        if u in seen:
            return None
        seen.add(u)
        path.append(u)
        v = u
    return path[::-1]


def labels(V, edges, P, d, rng, forward, layered=False):
    """first(x) (forward: T_s, lowest-index tight in-edge) or last(z) (T_t, tight out-edge; rng: a random tie choice, as the device's CSR
    order may give any; the device takes the smallest head id, one such choice).  Pointer doubling, then the layered build when a chain
    does not reach P within ceil(log2 V) + 1 rounds (or when asked)."""
    pidx = {v: j for j, v in enumerate(P)}
    par = [None] * V
    for v in range(V):
        if v in pidx or d[v] is None:
            continue
        if forward:
            tight = [a for a, b, w in edges if b == v and d[a] is not None and d[a] + w == d[v]]
            par[v] = tight[0]
        else:
            tight = [b for a, b, w in edges if a == v and d[b] is not None and w + d[b] == d[v]]
            par[v] = rng.choice(tight)
    jump = [v if v in pidx else par[v] for v in range(V)]
    rounds = 1
    x = V
    while x > 1:
        x = (x + 1) >> 1
        rounds += 1
    for _ in range(rounds):
        jump = [a if a is None or a in pidx else jump[a] for a in jump]
    ok = all(a is None or a in pidx for a in jump)
    if ok and not layered:
        return [None if a is None else pidx[a] for a in jump], False
    lab = [pidx.get(v) for v in range(V)]
    layer = [0 if v in pidx else None for v in range(V)]
    r = 0
    while True:
        r += 1
        new = {}
        for v in range(V):
            if layer[v] is not None or d[v] is None:
                continue
            if forward:
                cand = [a for a, b, w in edges if b == v and layer[a] is not None and layer[a] < r and d[a] + w == d[v]]
            else:
                cand = sorted(b for a, b, w in edges if a == v and layer[b] is not None and layer[b] < r and w + d[b] == d[v])
            if cand:
                new[v] = lab[cand[0]]
        if not new:
            return lab, True
        for v, l in new.items():
            lab[v] = l
            layer[v] = r


def drop_margins(V, edges, P, ds, dt, rng, layered=False, with_cross=True):
    """{j: D_{-p_j} - D or None} for every interior slot j of P, by the trees, the labels, the candidates and the cross nodes."""
    K = len(P) - 1
    D = ds[P[-1]]
    first, l1 = labels(V, edges, P, ds, rng, True, layered)
    last, l2 = labels(V, edges, P, dt, rng, False, layered)
    best = {j: None for j in range(1, K)}

    def put(j, c):
        if best[j] is None or c < best[j]:
            best[j] = c

    for x, z, w in edges:
        if first[x] is None or last[z] is None:
            continue
        c = ds[x] + w + dt[z] - D
        assert c >= 0
        for j in range(first[x] + 1, last[z]):
            put(j, c)
    n_cross = 0
    if with_cross:
        for j in range(1, K):
            Y = {y for y in range(V) if y != P[j] and first[y] is not None and last[y] is not None and last[y] <= j <= first[y]}
            if not Y:
                continue
            n_cross += 1
            delta = {y: None for y in Y}
            for x, y, w in edges:
                if y in Y and first[x] is not None and first[x] < j:
                    if delta[y] is None or ds[x] + w < delta[y]:
                        delta[y] = ds[x] + w
            for _ in range(len(Y) + 1):
                for x, y, w in edges:
                    if x in Y and y in Y and delta[x] is not None and (delta[y] is None or delta[x] + w < delta[y]):
                        delta[y] = delta[x] + w
            for y, z, w in edges:
                if y in Y and delta[y] is not None and last[z] is not None and last[z] > j:
                    put(j, delta[y] + w + dt[z] - D)
    return best, n_cross, l1 or l2


def random_graph(rng, V):
    """Nodes 0..V-1, source V-2, target V-1; mostly rightward edges, some backward ones (cycles), small weights with zero-weight cycles
    and many ties; no negative cycle (weights = potential differences + a non-negative rest)."""
    pot = [rng.randint(-6, 6) for _ in range(V)]
    order = list(range(V - 2))
    edges, seen = [], set()

    def add(a, b):
        if a == b or (a, b) in seen or a == V - 1 or b == V - 2:
            return
        seen.add((a, b))
        rest = rng.choice([0, 0, 0, 1, 2, 3])
        edges.append((a, b, pot[b] - pot[a] + rest))

    for v in order[: max(1, len(order) // 3)]:
        add(V - 2, v)
    for v in order[len(order) // 2:]:
        add(v, V - 1)
    for _ in range(rng.randint(V, 3 * V)):
        a = rng.randrange(V - 2)
        b = min(V - 3, a + rng.randint(1, 4)) if rng.random() < 0.8 else max(0, a - rng.randint(1, 4))
        add(a, b)
    rng.shuffle(edges)
    return edges


def check_graph(rng, V, layered=False):
    edges = random_graph(rng, V)
    s, t = V - 2, V - 1
    ds = bellman_ford(V, edges, s)
    if ds[t] is None:
        return None
    dt = bellman_ford(V, edges, t, reverse=True)
    P = shortest_path(V, edges, ds, s, t)
    if P is None or len(P) < 3:
        return None
    best, n_cross, lay = drop_margins(V, edges, P, ds, dt, rng, layered)
    for j in range(1, len(P) - 1):
        d = bellman_ford(V, edges, s, skip=P[j])[t]
        want = None if d is None else d - ds[t]
        assert best[j] == want, (edges, P, j, best[j], want)
    return n_cross, lay, (edges, P, ds, dt)


def test_restatement_equals_brute_force():
    rng = random.Random(12)
    n, cross, lay = 0, 0, 0
    for it in range(2500):
        r = check_graph(rng, rng.randint(5, 16))
        if r is None:
            continue
        n += 1
        cross += r[0] > 0
        lay += r[1]
    assert n > 1500 and cross > 20 and lay > 0, (n, cross, lay)


def test_restatement_layered_equals_brute_force():
    rng = random.Random(13)
    n = 0
    for it in range(600):
        r = check_graph(rng, rng.randint(5, 14), layered=True)
        n += r is not None
    assert n > 300


def test_cross_nodes_are_needed():
    """Without step 4 some slots come out too large (the replacement path runs through a cycle round p_j)."""
    rng = random.Random(14)
    miss = 0
    for it in range(3000):
        V = rng.randint(5, 14)
        edges = random_graph(rng, V)
        s, t = V - 2, V - 1
        ds = bellman_ford(V, edges, s)
        if ds[t] is None:
            continue
        dt = bellman_ford(V, edges, t, reverse=True)
        P = shortest_path(V, edges, ds, s, t)
        if P is None or len(P) < 3:
            continue
        best, _, _ = drop_margins(V, edges, P, ds, dt, random.Random(it), with_cross=False)
        for j in range(1, len(P) - 1):
            d = bellman_ford(V, edges, s, skip=P[j])[t]
            want = None if d is None else d - ds[t]
            if best[j] != want:
                assert want is not None and (best[j] is None or best[j] > want)
                miss += 1
    assert miss > 0


# ---- the formatter ----

def py_format(names, status, offsets, rec):
    out = []
    for i, nm in enumerate(names):
        if status[i] < 0:
            continue
        out.append("#id:\t%s\n" % nm)
        out.append("#START\tSTOP\tFRAME\tCONTIG\tSCORE\tDROP\tCALLED\n")
        for r in rec[offsets[i]:offsets[i + 1]]:
            a, z = (int(r["right"]), int(r["left"])) if r["strand"] < 0 else (int(r["left"]), int(r["right"]))
            out.append("%d\t%d\t%s\t%s\t%s\t%s\t%d\n" % (a, z, "+" if r["strand"] > 0 else "-", nm, "%E" % float(r["score"]), "%E" % float(r["drop"]), int(r["called"])))
    return "".join(out).encode()


def c_format(lib, names, status, offsets, rec):
    L = lib.lib()
    arr = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    status = np.ascontiguousarray(status, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    rec = np.ascontiguousarray(rec, lib.DROP_DT)
    text, tlen = C.c_void_p(), C.c_int64()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = L.phx_format_drops(len(names), arr, vp(rec), vp(offsets), vp(status), C.byref(text), C.byref(tlen))
    assert rc == 0
    out = C.string_at(text.value, tlen.value)
    L.phx_free_text(text)
    return out


def random_records(lib, rng, n_contig, per):
    counts = [0 if k % 7 == 3 else int(rng.randint(0, per)) for k in range(n_contig)]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rec = np.zeros(int(offsets[-1]), lib.DROP_DT)
    t = len(rec)
    left = np.sort(rng.randint(1, 200000, t))
    rec["left"] = left
    rec["right"] = left + 3 * rng.randint(30, 2000, t) + 2
    rec["strand"] = rng.choice([-1, 1], t)
    rec["frame"] = rec["strand"] * rng.randint(1, 4, t)
    rec["score"] = -np.exp(rng.uniform(-5, 40, t))
    rec["drop"] = np.where(rng.rand(t) < 0.2, 0.0, np.round(np.exp(rng.uniform(-7, 25, t)) * 1000) / 1000.0)
    rec["called"] = (rng.rand(t) < 0.95).astype(np.int32)
    rec["bypass"] = (rng.rand(t) < 0.97).astype(np.int32)
    rec["drop"][rec["bypass"] == 0] = np.inf
    status = np.zeros(n_contig, np.int32)
    status[1::9] = -2
    status[2::11] = 1
    names = ["ctg_%08d" % k for k in range(n_contig)]
    return names, status, offsets, rec


def test_format_drops_matches_python_rendering(lib):
    rng = np.random.RandomState(5)
    names, status, offsets, rec = random_records(lib, rng, 12, 40)
    assert status[1] < 0 and offsets[4] == offsets[3]
    assert (rec["strand"] < 0).any() and (~np.isfinite(rec["drop"])).any()
    assert c_format(lib, names, status, offsets, rec) == py_format(names, status, offsets, rec)


def test_format_drops_many_threads_same_text(lib, monkeypatch):
    rng = np.random.RandomState(6)
    names, status, offsets, rec = random_records(lib, rng, 300, 400)
    want = py_format(names, status, offsets, rec)
    assert len(want) > (1 << 20)
    assert c_format(lib, names, status, offsets, rec) == want
    monkeypatch.setenv("PHX_HOST_THREADS", "3")
    assert c_format(lib, names, status, offsets, rec) == want


def test_format_drops_no_contigs_and_bad_args(lib):
    assert c_format(lib, [], np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, lib.DROP_DT)) == b""
    L = lib.lib()
    text, tlen = C.c_void_p(), C.c_int64()
    assert L.phx_format_drops(-1, None, None, None, None, C.byref(text), C.byref(tlen)) == -1
    arr = (C.c_char_p * 1)(b"x")
    st = np.zeros(1, np.int32)
    offs = np.array([0, 2], np.int64)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    assert L.phx_format_drops(1, arr, None, vp(offs), vp(st), C.byref(text), C.byref(tlen)) == -1  # records missing
    assert L.phx_format_drops(1, arr, None, vp(offs), vp(st), None, C.byref(tlen)) == -1


# ---- the CLI, the header, the exports ----

def test_drop_margins_with_dump_is_refused(tmp_path):
    fa = os.path.join(ROOT, "tests", "golden", "phiX174.fasta.gz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), fa, "--dump", "--drop-margins", str(tmp_path / "d.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--drop-margins" in r.stderr and "--dump" in r.stderr
    assert not (tmp_path / "d.tsv").exists()


def test_drop_margins_under_a_multi_rank_launch_is_refused(tmp_path):
    fa = os.path.join(ROOT, "tests", "golden", "phiX174.fasta.gz")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), fa, "--drop-margins", str(tmp_path / "d.tsv")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "--drop-margins" in r.stderr and "multi-rank" in r.stderr


def test_drop_entry_points_are_declared_and_exported(lib):
    txt = open(os.path.join(ROOT, "include", "phx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(phx_[a-z0-9_]+)\s*\(", txt))
    new = {"phx_drop_margins_flat", "phx_drop_ms", "phx_drop_stats", "phx_format_drops"}
    assert new <= names and new <= set(lib.EXPORTS)
    L = lib.lib()
    for n in new:
        assert hasattr(L, n)
    assert lib.DROP_DT.itemsize == 40 and L.phx_version() == 410
