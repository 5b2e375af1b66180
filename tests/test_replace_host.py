"""Host side of the drop replacements (no GPU): the witness construction of DESIGN.md §13 restated in Python against brute force on random
cyclic graphs (zero-weight cycles, equal-length ties), its independence of the out-edge order, a graph family whose tree chains close a
zero-length loop that must be cut, the C formatter of --drop-replacements FILE against a plain Python rendering, the CLI's refusals, and
the new entry points in the header and the export list."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_drop_host import bellman_ford, random_graph, shortest_path  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from phanotate_amd import _lib

    return _lib


# ---- the construction, restated ----

def one_hop_trees(V, edges, out, P, d, forward, layered=False):
    """The one-hop tree T_s (forward: lowest-index tight in-edge, in `edges` order) or T_t (tight out-edge to the smallest head id, whatever
    the order of `out`), P nodes pointing at themselves; when a chain does not reach P (or when asked) the layered build of k_dp_tree:
    round r joins a node through a tight edge to a node that joined before round r.  Returns (parent, label, layered)."""
    pidx = {v: j for j, v in enumerate(P)}

    def tight(v, ok):
        if forward:
            c = [a for a, b, w in edges if b == v and d[a] is not None and ok(a) and d[a] + w == d[v]]
            return c[0] if c else None
        c = [b for b, w in out[v] if d[b] is not None and ok(b) and w + d[b] == d[v]]
        return min(c) if c else None

    par = [v if v in pidx else (tight(v, lambda u: True) if d[v] is not None else None) for v in range(V)]

    def label(v):
        seen = set()
        while v is not None and v not in pidx:
            if v in seen:
                return False
            seen.add(v)
            v = par[v]
        return None if v is None else pidx[v]

    lab = [label(v) for v in range(V)]
    if not layered and all(x is not False for x in lab):
        return par, lab, False
    layer = [0 if v in pidx else None for v in range(V)]
    par = [v if v in pidx else None for v in range(V)]
    r = 0
    while True:
        r += 1
        new = {}
        for v in range(V):
            if layer[v] is None and d[v] is not None:
                u = tight(v, lambda a: layer[a] is not None and layer[a] < r)
                if u is not None:
                    new[v] = u
        if not new:
            break
        for v, u in new.items():
            par[v], layer[v] = u, r
    return par, [label(v) for v in range(V)], True


def witnesses(V, edges, P, ds, dt, rng=None, layered=False):
    """{j: (R, cut, a, b, delta-chain length)} for every interior slot j of P with a bypass: the replacement path by the tie rule (cost;
    step-3 before cross; source id; head id), cut = a zero-length loop was cut, a / b where it leaves / rejoins P, the delta chain's
    length (0: a step-3 winner).  rng: shuffle every node's out-edge list (in-edge order is kept)."""
    K = len(P) - 1
    D = ds[P[-1]]
    out = [[] for _ in range(V)]
    for a, b, w in edges:
        out[a].append((b, w))
    if rng is not None:
        for lst in out:
            rng.shuffle(lst)
    pidx = {v: j for j, v in enumerate(P)}
    ps, first, _ = one_hop_trees(V, edges, out, P, ds, True, layered)
    ts, last, _ = one_hop_trees(V, edges, out, P, dt, False, layered)
    s3 = {j: None for j in range(1, K)}
    win3 = {}
    for x, z, w in edges:
        if first[x] is None or last[z] is None:
            continue
        c = ds[x] + w + dt[z] - D
        for j in range(first[x] + 1, last[z]):
            if s3[j] is None or (c, x, z) < (s3[j], *win3[j]):
                s3[j], win3[j] = c, (x, z)
    res = {}
    for j in range(1, K):
        Y = [y for y in range(V) if y not in pidx and first[y] is not None and last[y] is not None and last[y] <= j <= first[y]]
        Ys = set(Y)
        delta, rnd = {}, {}
        for y in Y:
            seeds = [ds[x] + w for x, b, w in edges if b == y and first[x] is not None and first[x] < j]
            delta[y], rnd[y] = (min(seeds) if seeds else None), 0
        for r in range(1, len(Y) + 3):  # Jacobi rounds, as k_dp_cross / k_rp_cross
            cur = dict(delta)
            ch = False
            for y in Y:
                for x, b, w in edges:
                    if b == y and x in Ys and cur[x] is not None and (delta[y] is None or cur[x] + w < delta[y]):
                        delta[y], rnd[y], ch = cur[x] + w, r, True
            if not ch:
                break
        cx, wx = None, None
        for y in Y:
            if delta[y] is None:
                continue
            for z, w in out[y]:
                if last[z] is not None and last[z] > j:
                    c = delta[y] + w + dt[z] - D
                    if cx is None or (c, y, z) < (cx, *wx):
                        cx, wx = c, (y, z)
        if s3[j] is None and cx is None:
            continue
        if cx is None or (s3[j] is not None and s3[j] <= cx):
            (x, z), mid = win3[j], []
        else:
            y, z = wx
            mid = [y]
            while rnd[mid[-1]] > 0:
                v = mid[-1]
                mid.append(min(u for u, b, w in edges if b == v and u in Ys and rnd[u] < rnd[v] and delta[u] is not None and delta[u] + w == delta[v]))
            v = mid[-1]
            x = min(u for u, b, w in edges if b == v and first[u] is not None and first[u] < j and ds[u] + w == delta[v])
            mid = mid[::-1]
        sch, v = [], x  # T_s chain of x, off P, from x up
        while v not in pidx:
            sch.append(v)
            v = ps[v]
        a = pidx[v]
        tch, v = [], z
        while v not in pidx:
            tch.append(v)
            v = ts[v]
        b = pidx[v]
        cut = None
        for d_, v in enumerate(sch):  # the shared node nearest p_a (the deepest from x)
            if v in tch:
                cut = (d_, tch.index(v))
        if cut is None:
            det = sch[::-1] + mid + tch
        else:
            det = sch[cut[0]:][::-1] + tch[cut[1] + 1:]
        res[j] = (P[: a + 1] + det + P[b:], cut is not None, a, b, len(mid))
    return res


def check_witnesses(V, edges, P, ds, wit):
    """Properties 1-3 of DESIGN.md §13 against brute force, for every interior slot with a bypass."""
    W = {(a, b): w for a, b, w in edges}
    s, t = V - 2, V - 1
    pidx = {v: j for j, v in enumerate(P)}
    n = 0
    for j in range(1, len(P) - 1):
        dg = bellman_ford(V, edges, s, skip=P[j])[t]
        if dg is None:
            assert j not in wit
            continue
        R, cut, a, b, _ = wit[j]
        assert R[0] == s and R[-1] == t and P[j] not in R and len(set(R)) == len(R), (edges, P, j, R)
        assert sum(W[(u, v)] for u, v in zip(R, R[1:])) == dg, (edges, P, j, R)
        assert R[: a + 1] == P[: a + 1] and R[len(R) - (len(P) - b):] == P[b:] and a < j < b
        assert not any(v in pidx for v in R[a + 1: len(R) - (len(P) - b)])
        n += 1
    return n


def test_witnesses_equal_brute_force_and_ignore_the_out_edge_order():
    rng = random.Random(21)
    graphs, slots, cuts, lay, cross, long_chains, kept = 0, 0, 0, 0, 0, 0, 0
    for it in range(2700):
        V = rng.randint(5, 15)
        edges = random_graph(rng, V)
        s, t = V - 2, V - 1
        ds = bellman_ford(V, edges, s)
        if ds[t] is None:
            continue
        dt = bellman_ford(V, edges, t, reverse=True)
        P = shortest_path(V, edges, ds, s, t)
        if P is None or len(P) < 3:
            continue
        wit = witnesses(V, edges, P, ds, dt, random.Random(it))
        graphs += 1
        slots += check_witnesses(V, edges, P, ds, wit)
        cuts += sum(w[1] for w in wit.values())
        cross += sum(w[4] > 0 for w in wit.values())
        long_chains += sum(w[4] > 1 for w in wit.values())
        kept += sum(w[4] > 0 and not w[1] for w in wit.values())
        assert witnesses(V, edges, P, ds, dt, random.Random(it + 99999)) == wit  # another out-edge order: the same bytes
        if it % 4 == 0:
            wl = witnesses(V, edges, P, ds, dt, layered=True)
            lay += check_witnesses(V, edges, P, ds, wl) > 0
    assert graphs >= 2000 and slots > 4000 and lay > 100, (graphs, slots, lay)
    assert cross > 50 and long_chains > 0 and kept > 0, (cross, long_chains, kept)


def loop_graph(rng):
    """A device path s -> p1 -> p2 -> p3 -> t and an off-path node w with ds(w) = ds(p1) + 1 and dt(w) = dt(p3): the chain w -> x_1 ..
    x_k -> z_1 .. z_m -> w is a cycle of length 0, so x_k -> z_1 (the lowest ids) ties with every other bypass of p2; its T_s chain runs
    through w, and so does z_1's T_t chain: the walk repeats w and the loop is cut.  Random extra ties and a relabelling keep it honest."""
    k, m = rng.randint(1, 3), rng.randint(1, 3)
    xs = list(range(k))
    zs = list(range(k, k + m))
    w, p1, p2, p3 = k + m, k + m + 1, k + m + 2, k + m + 3
    V = k + m + 6
    s, t = V - 2, V - 1
    pot = {v: rng.randint(-3, 3) for v in range(V)}
    edges = []

    def add(a, b, rest=0):
        edges.append((a, b, pot[b] - pot[a] + rest))

    add(s, p1); add(p1, p2); add(p2, p3); add(p3, t)
    add(p1, w, 1); add(w, p3)
    chain = [w] + xs + zs + [w]
    for a, b in zip(chain, chain[1:]):
        add(a, b)
    if rng.random() < 0.5:
        add(p1, p3, 1)  # another bypass of the same cost (a higher source id)
    rng.shuffle(edges)
    return V, edges


def test_zero_length_loops_between_the_tree_chains_are_cut():
    rng = random.Random(31)
    cut = 0
    for it in range(300):
        V, edges = loop_graph(rng)
        s, t = V - 2, V - 1
        ds = bellman_ford(V, edges, s)
        dt = bellman_ford(V, edges, t, reverse=True)
        P = shortest_path(V, edges, ds, s, t)
        if P is None:
            continue
        wit = witnesses(V, edges, P, ds, dt, random.Random(it))
        check_witnesses(V, edges, P, ds, wit)
        cut += sum(w[1] for w in wit.values())
    assert cut > 150, cut


# ---- the formatter ----

def py_format(names, status, offsets, rec, genes):
    def lst(g):
        if not len(g):
            return "-"
        return ",".join(("tRNA:" if abs(int(x["frame"])) == 4 else "") + "%d..%d" % ((x["right"], x["left"]) if x["strand"] < 0 else (x["left"], x["right"])) for x in g)

    out = []
    for i, nm in enumerate(names):
        if status[i] < 0:
            continue
        out.append("#id:\t%s\n#START\tSTOP\tFRAME\tCONTIG\tDROP\tREMOVED\tADDED\n" % nm)
        for r in rec[offsets[i]:offsets[i + 1]]:
            a, z = (int(r["right"]), int(r["left"])) if r["strand"] < 0 else (int(r["left"]), int(r["right"]))
            g = genes[int(r["gene_off"]): int(r["gene_off"]) + int(r["n_removed"]) + int(r["n_added"])]
            out.append("%d\t%d\t%s\t%s\t%s\t%s\t%s\n" % (a, z, "+" if r["strand"] > 0 else "-", nm, "%E" % float(r["drop"]), lst(g[: int(r["n_removed"])]), lst(g[int(r["n_removed"]):])))
    return "".join(out).encode()


def c_format(lib, names, status, offsets, rec, genes):
    L = lib.lib()
    arr = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    status = np.ascontiguousarray(status, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    rec = np.ascontiguousarray(rec, lib.REPL_DT)
    genes = np.ascontiguousarray(genes, lib.GENE_DT)
    text, tlen = C.c_void_p(), C.c_int64()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = L.phx_format_replacements(len(names), arr, vp(rec), vp(genes), vp(offsets), vp(status), C.byref(text), C.byref(tlen))
    assert rc == 0
    out = C.string_at(text.value, tlen.value)
    L.phx_free_text(text)
    return out


def random_records(lib, rng, n_contig, per):
    counts = [0 if k % 7 == 3 else int(rng.randint(0, per)) for k in range(n_contig)]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t = int(offsets[-1])
    rec = np.zeros(t, lib.REPL_DT)
    left = np.sort(rng.randint(1, 200000, t))
    rec["left"] = left
    rec["right"] = left + 3 * rng.randint(30, 2000, t) + 2
    rec["strand"] = rng.choice([-1, 1], t)
    rec["frame"] = rec["strand"] * rng.randint(1, 4, t)
    rec["drop"] = np.where(rng.rand(t) < 0.2, 0.0, np.round(np.exp(rng.uniform(-7, 25, t)) * 1000) / 1000.0)
    rec["called"] = (rng.rand(t) < 0.95).astype(np.int32)
    rec["bypass"] = (rng.rand(t) < 0.97).astype(np.int32)
    rec["drop"][rec["bypass"] == 0] = np.inf
    rec["n_removed"] = np.where(rec["bypass"] == 1, rng.randint(1, 4, t), 0)
    rec["n_added"] = np.where(rec["bypass"] == 1, rng.randint(0, 4, t), 0)
    ng = rec["n_removed"] + rec["n_added"]
    rec["gene_off"] = np.concatenate([[0], np.cumsum(ng)[:-1]]) if t else []
    G = int(ng.sum())
    genes = np.zeros(G, lib.GENE_DT)
    gl = rng.randint(1, 200000, G)
    genes["left"] = gl
    genes["right"] = gl + 3 * rng.randint(20, 900, G) + 2
    genes["strand"] = rng.choice([-1, 1], G)
    genes["frame"] = genes["strand"] * np.where(rng.rand(G) < 0.1, 4, rng.randint(1, 4, G))
    genes["score"] = np.where(np.abs(genes["frame"]) == 4, -20.0, -np.exp(rng.uniform(-5, 30, G)))
    rec["span_left"] = rec["left"]
    rec["span_right"] = rec["right"]
    status = np.zeros(n_contig, np.int32)
    status[1::9] = -2
    status[2::11] = 1
    names = ["ctg_%08d" % k for k in range(n_contig)]
    return names, status, offsets, rec, genes


def test_format_replacements_matches_python_rendering(lib):
    rng = np.random.RandomState(5)
    names, status, offsets, rec, genes = random_records(lib, rng, 12, 40)
    assert status[1] < 0 and offsets[4] == offsets[3]
    assert (rec["strand"] < 0).any() and (rec["bypass"] == 0).any() and (np.abs(genes["frame"]) == 4).any() and (rec["n_added"] == 0).any()
    assert c_format(lib, names, status, offsets, rec, genes) == py_format(names, status, offsets, rec, genes)


def test_format_replacements_many_threads_same_text(lib, monkeypatch):
    rng = np.random.RandomState(6)
    names, status, offsets, rec, genes = random_records(lib, rng, 300, 300)
    want = py_format(names, status, offsets, rec, genes)
    assert len(want) > (1 << 20)
    assert c_format(lib, names, status, offsets, rec, genes) == want
    monkeypatch.setenv("PHX_HOST_THREADS", "3")
    assert c_format(lib, names, status, offsets, rec, genes) == want


def test_format_replacements_no_contigs_and_bad_args(lib):
    assert c_format(lib, [], np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, lib.REPL_DT), np.zeros(0, lib.GENE_DT)) == b""
    L = lib.lib()
    text, tlen = C.c_void_p(), C.c_int64()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    assert L.phx_format_replacements(-1, None, None, None, None, None, C.byref(text), C.byref(tlen)) == -1
    arr = (C.c_char_p * 1)(b"x")
    st = np.zeros(1, np.int32)
    offs = np.array([0, 2], np.int64)
    assert L.phx_format_replacements(1, arr, None, None, vp(offs), vp(st), C.byref(text), C.byref(tlen)) == -1  # records missing
    rec = np.zeros(2, lib.REPL_DT)
    rec["n_removed"] = 1
    assert L.phx_format_replacements(1, arr, vp(rec), None, vp(offs), vp(st), C.byref(text), C.byref(tlen)) == -1  # genes missing
    assert L.phx_format_replacements(1, arr, vp(rec), None, vp(offs), vp(st), None, C.byref(tlen)) == -1


# ---- the CLI, the header, the exports ----

def test_drop_replacements_with_dump_is_refused(tmp_path):
    fa = os.path.join(ROOT, "tests", "golden", "phiX174.fasta.gz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), fa, "--dump", "--drop-replacements", str(tmp_path / "r.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--drop-replacements" in r.stderr and "--dump" in r.stderr
    assert not (tmp_path / "r.tsv").exists()


def test_drop_replacements_under_a_multi_rank_launch_is_refused(tmp_path):
    fa = os.path.join(ROOT, "tests", "golden", "phiX174.fasta.gz")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "phanotate.py"), fa, "--drop-replacements", str(tmp_path / "r.tsv")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "--drop-replacements" in r.stderr and "multi-rank" in r.stderr


def test_replacement_entry_points_are_declared_and_exported(lib):
    txt = open(os.path.join(ROOT, "include", "phx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(phx_[a-z0-9_]+)\s*\(", txt))
    new = {"phx_replacements_flat", "phx_tap_replacement", "phx_replacements_ms", "phx_replacement_stats", "phx_format_replacements"}
    assert new <= names and new <= set(lib.EXPORTS)
    L = lib.lib()
    for n in new:
        assert hasattr(L, n)
    assert lib.REPL_DT.itemsize == 56 and lib.DROP_DT.itemsize == 40 and L.phx_version() == 410
