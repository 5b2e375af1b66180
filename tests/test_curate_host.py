"""Host side of the combined re-annotation (no GPU): the order (-c(P), S(P)) against a Bellman-Ford under W + B - M·[R'] on
small random graphs, the cases in which that Bellman-Ford does not settle, the tile path's three flag fields restated, the header, the
export list and the entry point without a context, the CLI's standing refusal, and — on the CPU oracle's graphs — how many of the GPU
test's seeded random mixes settle."""
import os
import random
import re
import subprocess
import sys

import pytest

from conftest import ROOT, inorder_bellman_ford
from test_evidence_gpu import settle


# ---- the definition on small graphs ----
def random_graph(rng):
    """(V, edges [(u, v, W)], R, F, B) on <= 8 nodes; source 0, target V - 1; R, F disjoint sets of edges, B a signed integer per edge (0: none)."""
    V = rng.randint(3, 8)
    pairs = [(u, v) for u in range(V) for v in range(V) if u != v and v != 0 and u != V - 1]
    rng.shuffle(pairs)
    pairs = pairs[: rng.randint(V, min(len(pairs), 3 * V))]
    edges = [(u, v, rng.randint(0, 40) if rng.random() < 0.85 else rng.randint(-6, 0)) for u, v in pairs]
    marks = list(range(len(edges)))
    rng.shuffle(marks)
    nr, nf = rng.randint(0, 3), rng.randint(0, 2)
    R, F = set(marks[:nr]), set(marks[nr:nr + nf])
    B = [0] * len(edges)
    for k in marks[: rng.randint(0, 4)] if rng.random() < 0.5 else marks[-rng.randint(1, 4):]:
        B[k] = rng.randint(-30, 30)
    return V, edges, R, F, B


def simple_paths(V, edges, F):
    """Every simple source -> target path without an edge of F, as a list of edge indices."""
    out_of = [[] for _ in range(V)]
    for k, (u, v, _) in enumerate(edges):
        if k not in F:
            out_of[u].append(k)
    found, stack = [], [(0, [], {0})]
    while stack:
        u, path, seen = stack.pop()
        if u == V - 1:
            found.append(path)
            continue
        for k in out_of[u]:
            v = edges[k][1]
            if v not in seen:
                stack.append((v, path + [k], seen | {v}))
    return found


def curated(V, edges, R, F, B, M):
    """The edge list of the definition: G_{F,B} with - M on R' (an edge of F is no edge, so its bias and its place in R do not count)."""
    return [(u, v, w + B[k] - (M if k in R else 0)) for k, (u, v, w) in enumerate(edges) if k not in F]


def test_lexicographic_order_is_bellman_ford_under_w_plus_b_minus_m():
    rng = random.Random(2200)
    settled = cyclic = with_both = nopath = 0
    for _ in range(4000):
        V, edges, R, F, B = random_graph(rng)
        R = R - F
        bound = sum(abs(w) for _, _, w in edges) + sum(abs(b) for b in B)
        results = []
        for M in (bound + 1, 1 << 200):
            kept = curated(V, edges, R, F, B, M)
            orig = [k for k in range(len(edges)) if k not in F]  # kept row -> edge
            dist, par = settle(V, kept, 0)
            assert (dist is None) == (inorder_bellman_ford(V, kept, 0)[0] is None)  # the quick yardstick is the plain one
            results.append(None if dist is None else dist[V - 1] if dist[V - 1] is not None else "nopath")
            if dist is not None and dist[V - 1] is not None:  # the parents' path carries what the distance says
                c = S = 0
                v = V - 1
                while v != 0:
                    k = orig[par[v]]
                    c += k in R
                    S += edges[k][2] + B[k]
                    v = edges[k][0]
                results[-1] = (c, S)
                assert dist[V - 1] == S - c * M
        assert (results[0] is None) == (results[1] is None)
        if results[0] is None:
            cyclic += 1
            continue
        assert results[0] == results[1]  # any M above the walk sums gives the same count and the same sum
        # brute force: most edges of R', then the least sum of W + B
        paths = simple_paths(V, edges, F)
        if not paths:
            assert results[0] == "nopath"
            nopath += 1
            continue
        best = min((-sum(k in R for k in p), sum(edges[k][2] + B[k] for k in p)) for p in paths)
        assert results[0] == (-best[0], best[1]), (edges, R, F, B)
        settled += 1
        with_both += bool(R) and any(B[k] for k in range(len(edges)) if k not in F)
    assert settled >= 2000 and with_both >= 500 and cyclic >= 100 and nopath >= 20, (settled, with_both, cyclic, nopath)


def test_a_negative_cycle_made_by_a_bias_or_a_required_edge_does_not_settle():
    # 0 -> 1 -> 2 -> 1, 2 -> 3: the cycle 1 -> 2 -> 1 has length 10
    edges = [(0, 1, 5), (1, 2, 4), (2, 1, 6), (2, 3, 7)]
    M = 1 << 60
    quiet = dict(V=4, edges=edges, R=set(), F=set(), B=[0, 0, 0, 0], M=M)
    assert settle(4, curated(**quiet), 0)[0] is not None
    assert settle(4, curated(**dict(quiet, B=[0, -11, 0, 0])), 0) == (None, None)  # a bonus beyond the cycle's length
    assert settle(4, curated(**dict(quiet, B=[0, -10, 0, 0])), 0)[0] is not None  # a cycle of length 0 is none
    assert settle(4, curated(**dict(quiet, R={2})), 0) == (None, None)  # a required edge on a reachable cycle
    assert settle(4, curated(**dict(quiet, R={2}, B=[3, 0, 0, -2])), 0) == (None, None)  # ... whatever the biases elsewhere
    assert settle(4, curated(**dict(quiet, R={3}, B=[0, -11, 0, 0])), 0) == (None, None)  # a bias-made cycle, the required edge elsewhere
    assert settle(4, curated(**dict(quiet, R={2}, F={2})), 0)[0] is not None  # refusing the edge takes the cycle away
    # a cycle the source does not reach is none of the solve: 4 -> 5 -> 4 hangs off nothing
    apart = edges + [(4, 5, 1), (5, 4, 1), (5, 3, 1)]
    dist, par = settle(6, curated(V=6, edges=apart, R={4}, F=set(), B=[0, 0, 0, 0, 0, -9, 0], M=M), 0)
    assert dist is not None and dist[3] == 16 and dist[4] is None and dist[5] is None


# ---- the tile path's flags (phx_sssp.inc, lds_sweep): 16 x 3 bits in two registers ----
def pack(refused, required, biased, req_and_bias):
    """r_mk and r_mb of one thread as the prefetch sets them for its up to 16 tile rows: refused in bits 0-15 of r_mk; under one policy the
    required or the biased flag in bits 16-31 of r_mk; under both the required flag there and the biased one in bits 0-15 of r_mb."""
    r_mk = r_mb = 0
    for j in range(len(refused)):
        r_mk |= refused[j] << j
        if req_and_bias:
            r_mk |= required[j] << (16 + j)
            r_mb |= biased[j] << j
        else:
            assert not (required[j] and biased[j])
            r_mk |= (required[j] | biased[j]) << (16 + j)
    assert r_mk < 1 << 32 and r_mb < 1 << 16
    return r_mk, r_mb


def fill(r_mk, r_mb, j, W, B, M, req, bias):
    """What the tile fill stores for row j under the policy (req, bias): B added, then the top limb decremented; a refused row overrides both."""
    if (r_mk >> j) & 1:
        return None
    w = W
    if req and bias:
        if (r_mb >> j) & 1:
            w += B
        if (r_mk >> (16 + j)) & 1:
            w -= M
    elif req and (r_mk >> (16 + j)) & 1:
        w -= M
    elif bias and (r_mk >> (16 + j)) & 1:
        w += B
    return w


def test_flag_packing_round_trips():
    rng = random.Random(2202)
    M = 1 << 128
    for _ in range(2000):
        n = rng.randint(1, 16)
        f, r, b = ([rng.random() < 0.3 for _ in range(n)] for _ in range(3))
        W = [rng.randint(-10 ** 6, 10 ** 6) for _ in range(n)]
        B = [rng.randint(-2 ** 52, 2 ** 52) for _ in range(n)]
        r_mk, r_mb = pack(f, r, b, True)
        assert [(r_mk >> j) & 1 for j in range(n)] == f and [(r_mk >> (16 + j)) & 1 for j in range(n)] == r and [(r_mb >> j) & 1 for j in range(n)] == b
        for j in range(n):
            assert fill(r_mk, r_mb, j, W[j], B[j], M, True, True) == (None if f[j] else W[j] + (B[j] if b[j] else 0) - (M if r[j] else 0))
        # with one policy the old packing stands: the third field stays empty and bits 16-31 mean what the policy says
        for req in (True, False):
            only = [x and not f[j] for j, x in enumerate(r if req else b)]
            none = [False] * n
            r_mk, r_mb = pack(f, only if req else none, none if req else only, False)
            assert r_mb == 0
            for j in range(n):
                assert fill(r_mk, r_mb, j, W[j], B[j], M, req, not req) == (None if f[j] else W[j] + ((-M if req else B[j]) if only[j] else 0))


# ---- the interface ----
def test_header_exports_and_annotator_method():
    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    m = re.search(r"int phx_curate_flat\(([^;]*)\);", text)
    assert m is not None
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "bias", "forbid", "require", "orf_offsets", "flags", "genes", "cap", "offsets", "status", "delta", "unmet", "total"]
    assert args[1] == "const int64_t *bias" and args[3] == "const uint8_t *require"
    assert "phx_curate_flat" in _lib.EXPORTS
    assert re.search(r"#define PHX_VERSION 410\b", text)  # callers probe for the symbol
    L = _lib.lib()
    assert len(L.phx_curate_flat.argtypes) == 13
    assert L.phx_curate_flat(None, None, None, None, None, 0, None, 0, None, None, None, None, None) == -1  # PHX_E_ARG without a context
    assert callable(api.Annotator.curate)


def test_cli_still_refuses_evidence_with_require(tmp_path):
    """The command line keeps refusing the combination (tests/test_evidence_host.py pins that refusal): the combined solve is offered by
    phx_curate_flat and Annotator.curate() only (Limits)."""
    ev = tmp_path / "e.txt"
    ev.write_text("1\t9\t+\tc1\t-2.5\n")
    rq = tmp_path / "r.txt"
    rq.write_text("1\t9\t+\tc1\n")
    out, fasta = tmp_path / "o.txt", tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    for extra in ([], ["--forbid", str(rq)]):
        r = subprocess.run(exe + ["--evidence", str(ev), "--require", str(rq), "--reannotation", str(out)] + extra, capture_output=True, timeout=120)
        assert r.returncode == 2 and b"--evidence: not allowed with argument --require" in r.stderr, r.stderr[-500:]
    r = subprocess.run(exe + ["--require", str(rq), "--reannotation", str(out), "--remargins", str(out)], capture_output=True, timeout=120)
    assert r.returncode == 2 and b"--remargins: not allowed with argument --require" in r.stderr


# ---- the GPU test's random mixes, on the CPU oracle's graphs ----
def test_most_random_mixes_settle(oracle):
    """tests/test_curate_gpu.py hands the draws of curate_draws.mixes to the device and asks that at least 30 of at least 40 end with status
    0.  Here the yardstick alone — the same weights on the oracle's graph of the same contig — says how many settle with a path."""
    import phanotate_amd as pa

    import curate_draws as cd

    graphs = [cd.OracleGraph(oracle, s) for s in cd.mix_seqs(pa)]
    assert sum(g.ok for g in graphs) >= 8
    for g in graphs:  # the oracle's graph read rightly: its own path's distance, and its genes among the ORF edges
        if g.ok:
            dist, par = settle(g.V, g.edges, g.src)
            assert dist[g.tgt] == g.D and g.called <= set(g.orf_edge)
    draws = ok = cyc = kept = 0
    for row in cd.mixes(graphs):
        for g, d in zip(graphs, row):
            if d is None:
                continue
            assert 1 <= len(d["require"]) <= 2 and 1 <= len(d["bias"]) <= 3 and len(d["forbid"]) <= 2 and not set(d["require"]) & set(d["forbid"])
            assert not set(d["require"]) & g.called
            draws += 1
            M = cd.big_m(g.edges, d)
            edges, pinned = cd.weights(g.edges, g.orf_edge, d, M)
            dist, par = settle(g.V, edges, g.src)
            if dist is None:
                cyc += 1
            elif dist[g.tgt] is not None:
                ok += 1
                kept += (-dist[g.tgt] + M // 2) // M
    print("random mixes on the oracle's graphs: %d draws, %d settle with a path (%d required ORFs kept), %d do not settle" % (draws, ok, kept, cyc))
    assert draws >= 40 and ok >= 30 and kept >= 30, (draws, ok, kept, cyc)
