"""Host side of the pinned re-annotation (no GPU): the definition restated in Python and checked on random graphs — the
big-M in-place Bellman-Ford, the lexicographic (-count, W) Bellman-Ford and brute force over simple paths agree, the path does not depend on
M, the solver's cycle guard ("a distance counts more required edges than exist") fires exactly on the graphs with a cycle through a required
edge, and the split of a distance into (count, W-sum) as the device does it on limbs is exact.  Also --require's parsing and refusals, the
header and the export list."""
import io
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_drop_host import random_graph  # noqa: E402


# ---- the definition, restated ----

def bipartite_graph(rng, V):
    """As test_drop_host.random_graph (source V-2, target V-1, potentials + a non-negative rest: zero-length cycles and ties, no negative
    cycle), but bipartite like the annotation graph: even nodes are 'open', odd ones 'close', interior edges join the two classes, the
    source reaches open nodes and close nodes reach the target."""
    pot = [rng.randint(-6, 6) for _ in range(V)]
    edges, seen = [], set()

    def add(a, b):
        if a == b or (a, b) in seen or a == V - 1 or b == V - 2:
            return
        seen.add((a, b))
        edges.append((a, b, pot[b] - pot[a] + rng.choice([0, 0, 0, 1, 2, 3])))

    inner = list(range(V - 2))
    for v in inner[: max(2, len(inner) // 2)]:
        if v % 2 == 0:
            add(V - 2, v)
    for v in inner[len(inner) // 3:]:
        if v % 2 == 1:
            add(v, V - 1)
    for _ in range(rng.randint(V, 3 * V)):
        a = rng.randrange(V - 2)
        step = rng.choice([1, 1, 3]) if rng.random() < 0.75 else -rng.choice([1, 1, 3])
        b = a + step
        if 0 <= b < V - 2:
            add(a, b)
    rng.shuffle(edges)
    return edges


def inplace_bf(V, edges, s, weight, lt, zero, rounds=None, stop=None):
    """In-place Bellman-Ford in `edges` order with a strict '<' on abstract weights; (dist, parent edge) or (None, None) when it does not
    settle within `rounds` (default V + 1) rounds.  stop(value): end at once with ("stopped", None) when a stored value satisfies it."""
    dist, par = [None] * V, [-1] * V
    dist[s] = zero
    for _ in range(V + 1 if rounds is None else rounds):
        ch = False
        for i, (u, v, _) in enumerate(edges):
            if dist[u] is None:
                continue
            nd = weight(dist[u], i)
            if dist[v] is None or lt(nd, dist[v]):
                dist[v], par[v] = nd, i
                ch = True
                if stop is not None and stop(nd):
                    return "stopped", None
        if not ch:
            return dist, par
    return None, None


def solve_big_m(V, edges, R, M, **kw):
    """W'(e) = W(e) - M [e in R]."""
    return inplace_bf(V, edges, V - 2, lambda d, i: d + edges[i][2] - (M if i in R else 0), lambda a, b: a < b, 0, **kw)


def solve_lex(V, edges, R, **kw):
    """Values (-count, W-sum), compared lexicographically."""
    return inplace_bf(V, edges, V - 2, lambda d, i: (d[0] - (1 if i in R else 0), d[1] + edges[i][2]), lambda a, b: a < b, (0, 0), **kw)


def split(dist, M):
    """(count, W-sum) of a big-M distance, |W-sum| < M / 2: the yardstick's rule, count = round(-dist / M) in integers."""
    count = (-dist + M // 2) // M
    return count, dist + count * M


def walk(V, edges, par):
    path, v = [V - 1], V - 1
    while v != V - 2:
        v = edges[par[v]][0]
        path.append(v)
        assert len(path) <= V
    return path[::-1]


def brute_force(V, edges, R):
    """min over simple source -> target paths of (-count, W-sum); None: no path."""
    out = [[] for _ in range(V)]
    for i, (a, b, w) in enumerate(edges):
        out[a].append((b, w, i))
    best = [None]

    def go(v, seen, c, w):
        if v == V - 1:
            if best[0] is None or (-c, w) < best[0]:
                best[0] = (-c, w)
            return
        for b, ww, i in out[v]:
            if b not in seen:
                seen.add(b)
                go(b, seen, c + (i in R), w + ww)
                seen.discard(b)

    go(V - 2, {V - 2}, 0, 0)
    return best[0]


def on_a_cycle(V, edges, i):
    """Edge i = (a, b) lies on a cycle: a is reachable from b."""
    a, b, _ = edges[i]
    seen, todo = {b}, [b]
    while todo:
        x = todo.pop()
        for u, v, _ in edges:
            if u == x and v not in seen:
                seen.add(v)
                todo.append(v)
    return a in seen


def reachable_from_source(V, edges):
    seen, todo = {V - 2}, [V - 2]
    while todo:
        x = todo.pop()
        for u, v, _ in edges:
            if u == x and v not in seen:
                seen.add(v)
                todo.append(v)
    return seen


def graphs(seed, n):
    rng = random.Random(seed)
    for g in range(n):
        V = rng.randint(6, 10)
        edges = random_graph(rng, V) if g % 2 else bipartite_graph(rng, V)
        k = rng.randint(1, 4)
        R = set(rng.sample(range(len(edges)), min(k, len(edges))))
        yield rng, V, edges, R


def test_big_m_lexicographic_and_brute_force_agree_and_the_guard_fires_exactly_on_required_cycles():
    n_cycle = n_ok = n_multi = n_unmet = n_neg = 0
    for rng, V, edges, R in graphs(1601, 5000):
        bound = sum(abs(w) for _, _, w in edges) * (V + 2) + 1  # above every |walk sum| of at most V + 1 rounds' worth of edges... and far more
        M = 2 * bound + 1
        k = len(R)
        reach = reachable_from_source(V, edges)
        cyc = any(edges[i][0] in reach and on_a_cycle(V, edges, i) for i in R)  # (a cycle the source cannot reach relaxes nothing)
        # the guard: a stored distance that counts more than k required edges
        # (k + 1 turns of a cycle of up to V edges may take a round per edge: more rounds than the V + 1 a settled solve needs)
        g_lex = solve_lex(V, edges, R, rounds=V * (k + 3), stop=lambda d: -d[0] > k)
        g_big = solve_big_m(V, edges, R, M=1 << 200, rounds=V * (k + 3), stop=lambda d: split(d, 1 << 200)[0] > k)
        assert (g_lex[0] == "stopped") == cyc == (g_big[0] == "stopped"), (edges, R)
        if cyc:
            n_cycle += 1
            assert solve_lex(V, edges, R, rounds=4 * V * (k + 2))[0] is None  # ... and without the guard it never settles
            continue
        lex, lpar = g_lex
        big, bpar = solve_big_m(V, edges, R, M)
        assert lex is not None and big is not None
        want = brute_force(V, edges, R)
        if want is None:
            assert lex[V - 1] is None and big[V - 1] is None
            continue
        n_ok += 1
        count, wsum = split(big[V - 1], M)
        assert (-count, wsum) == lex[V - 1] == want, (edges, R)
        n_multi += count >= 2
        n_unmet += count < k
        n_neg += wsum < 0
        # every node, not the target alone; and the same parents (so the same path) for any admissible M
        for v in range(V):
            assert (lex[v] is None) == (big[v] is None)
            if big[v] is not None:
                c, w = split(big[v], M)
                assert (-c, w) == lex[v]
        assert bpar == lpar
        p0 = walk(V, edges, bpar)
        for M2 in (M + rng.randint(1, 1000), 1 << 64, 1 << 128, 1 << 4000):
            big2, par2 = solve_big_m(V, edges, R, M2)
            assert par2 == bpar and walk(V, edges, par2) == p0 and split(big2[V - 1], M2) == (count, wsum)
    print("graphs: %d settled (%d with count >= 2, %d with an unmet required edge, %d with a negative W-sum), %d with a cycle through a required edge"
          % (n_ok, n_multi, n_unmet, n_neg, n_cycle))
    assert n_ok >= 2000 and n_cycle >= 50 and n_multi >= 200 and n_unmet >= 200 and n_neg >= 200


# ---- the split on limbs, as the device does it (rq_count, k_rs_fin) ----

def to_limbs(x, n):
    x &= (1 << (64 * n)) - 1
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]


def device_split(limbs):
    """NL + 1 little-endian limbs of dist = W-sum - count * 2^(64 NL) -> (count, W-sum): the count is minus (the top limb plus the sign bit of
    the limb below, mod 2^64, as a signed number), the W-sum the low NL limbs as a two's complement number."""
    nl = len(limbs) - 1
    t = (limbs[nl] + (limbs[nl - 1] >> 63)) & 0xFFFFFFFFFFFFFFFF
    count = -(t - (1 << 64) if t >> 63 else t)
    w = sum(limbs[i] << (64 * i) for i in range(nl))
    if w >> (64 * nl - 1):
        w -= 1 << (64 * nl)
    return count, w


def test_the_split_of_a_distance_into_count_and_w_sum_is_exact_on_limbs():
    rng = random.Random(1602)
    for nl in (2, 4, 8, 17):
        M = 1 << (64 * nl)
        lim = 1 << (64 * nl - 3)  # the layout's bound on a path sum of the class (DESIGN.md §11 Widths)
        ws = [0, 1, -1, lim - 1, -(lim - 1), (1 << 63), -(1 << 63), (1 << 64) - 1, -(1 << 64)] + [rng.randint(-lim + 1, lim - 1) for _ in range(300)] + \
             [rng.randint(-5000, 5000) for _ in range(100)]
        for w in ws:
            for count in (0, 1, 2, 7, rng.randint(0, 1 << 20), (1 << 30) - 1):
                d = w - count * M
                assert device_split(to_limbs(d, nl + 1)) == (count, w) == split(d, M), (nl, w, count)
        # the unreached pattern (top limb 2^62) is no count: it splits into something negative, which no guard bound exceeds
        assert device_split([0] * nl + [1 << 62])[0] < 0


# ---- --require: parsing and refusals ----

def test_require_uses_the_forbid_parser_with_its_own_flag_in_the_messages():
    from phanotate_amd.cli import ForbidError, format_reannotation, parse_forbid, resolve_forbid

    lines = ["# kept calls\n", "\n", "100\t400\t+\tc1\t-3.5\n", "900 300 - c2\n"]
    assert parse_forbid(lines, "--require") == parse_forbid(lines) == [(100, 400, 1, "c1", "100\t400\t+\tc1\t-3.5"), (300, 900, -1, "c2", "900 300 - c2")]
    for flag in ("--forbid", "--require"):
        with pytest.raises(ForbidError) as e:
            parse_forbid(["100\t400\tx\tc1\n"], flag)
        assert str(e.value).startswith(flag + ": not START STOP FRAME CONTIG") and repr("100\t400\tx\tc1") in str(e.value)

    def lookup(i, left, right, strand):
        if (i, left) != (0, 100):
            raise KeyError
        return 5

    ents = parse_forbid(lines, "--require")
    assert resolve_forbid(ents[:1], ["c1", "c2"], lookup, "--require") == [[5], None]
    with pytest.raises(ForbidError) as e:
        resolve_forbid(ents, ["c1", "c2"], lookup, "--require")
    assert str(e.value).startswith("--require: no such ORF in its contig") and repr("900 300 - c2") in str(e.value)
    with pytest.raises(ForbidError) as e:
        resolve_forbid(ents, ["c1", "c2"], lookup)
    assert str(e.value).startswith("--forbid: ")
    # the #unmet: line comes with --require only
    import numpy as np

    from phanotate_amd import _lib

    genes = np.zeros(0, _lib.GENE_DT)
    st, offs = np.zeros(2, np.int32), np.zeros(3, np.int64)
    plain = format_reannotation(["a", "b"], st, offs, genes, np.array([0.0, 1.5]))
    both = format_reannotation(["a", "b"], st, offs, genes, np.array([0.0, 1.5]), np.array([0, 2], np.int32))
    assert "#unmet:" not in plain and both.count("#unmet:\t") == 2
    assert [ln for ln in both.splitlines() if not ln.startswith("#unmet:")] == plain.splitlines()
    lb = both.splitlines()
    k = lb.index("#delta:\t1.5")
    assert lb[k + 1] == "#unmet:\t2"


def test_cli_refusals_of_require_need_no_device(tmp_path):
    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    rq = tmp_path / "r.txt"
    rq.write_text("1\t9\t+\tc1\n")
    out = tmp_path / "o.txt"
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    for bad, word in ((["--require", str(rq)], b"--require: needs --reannotation"),
                      (["--require", str(rq), "--reannotation", str(out), "-d"], b"-d/--dump"),
                      (["--require", str(rq), "--reannotation", str(out), "--gpus", "2"], b"--require: not available with --gpus above 1"),
                      (["--reannotation", str(out)], b"each needs the other")):
        r = subprocess.run(exe + bad, capture_output=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    r = subprocess.run(exe + ["--require", str(rq), "--reannotation", str(out)], capture_output=True, timeout=120, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and b"multi-rank" in r.stderr


def test_header_exports_and_annotator_method():
    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    m = re.search(r"int phx_constrain_flat\(([^;]*)\);", text)
    assert m is not None
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "forbid", "require", "orf_offsets", "flags", "genes", "cap", "offsets", "status", "delta", "unmet", "total"]
    assert "phx_constrain_flat" in _lib.EXPORTS
    assert re.search(r"int phx_reannotate_flat\(phx_ctx \*ctx, const uint8_t \*forbid, const int64_t \*orf_offsets", text)  # (its signature stays)
    L = _lib.lib()
    assert L.phx_constrain_flat.argtypes is not None and len(L.phx_constrain_flat.argtypes) == 12
    assert L.phx_constrain_flat(None, None, None, None, 0, None, 0, None, None, None, None, None) == -1  # PHX_E_ARG without a context
    assert callable(api.Annotator.constrain)
