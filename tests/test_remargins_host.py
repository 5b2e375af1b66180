"""Host side of the re-annotation margins (no GPU): the header, the export list and the entry point without a context,
--remargins' refusals, and the lemma that lets the restricted reverse pass settle, restated in Python integers."""
import os
import random
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_header_exports_and_annotator_method():
    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    m = re.search(r"int phx_remargins_flat\(([^;]*)\);", text)
    assert m is not None
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "rec", "cap", "offsets", "status", "total"]
    assert args[1] == "phx_orf_margin *rec"
    m = re.search(r"int phx_tap_redist\(([^;]*)\);", text)
    assert m is not None and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["ctx", "contig", "which", "dist_limbs", "cap_words"]
    assert re.search(r"int phx_remargins_ms\(phx_ctx \*ctx, float \*ms", text)
    for name in ("phx_remargins_flat", "phx_remargins_ms", "phx_tap_redist"):
        assert name in _lib.EXPORTS
    assert re.search(r"#define PHX_VERSION 410\b", text)  # callers probe for the symbol
    L = _lib.lib()
    assert len(L.phx_remargins_flat.argtypes) == 6 and len(L.phx_tap_redist.argtypes) == 5 and len(L.phx_remargins_ms.argtypes) == 2
    assert L.phx_remargins_flat(None, None, 0, None, None, None) == -1  # PHX_E_ARG without a context
    assert L.phx_tap_redist(None, 0, 0, None, 0) == -1 and L.phx_remargins_ms(None, None) == -1
    assert callable(api.Annotator.remargins) and callable(api.Annotator.remargins_ms) and callable(api.Annotator.redist)


def test_cli_refusals_of_remargins_need_no_device(tmp_path):
    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    ev = tmp_path / "e.txt"
    ev.write_text("1\t9\t+\tc1\t-2.5\n")
    out, mg = tmp_path / "o.txt", tmp_path / "m.txt"
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    full = ["--evidence", str(ev), "--reannotation", str(out), "--remargins", str(mg)]
    for bad, word in ((["--remargins", str(mg)], b"--remargins: needs --reannotation"),
                      (["--evidence", str(ev), "--remargins", str(mg)], b"--remargins: needs --reannotation"),
                      (["--forbid", str(ev), "--require", str(ev), "--reannotation", str(out), "--remargins", str(mg)], b"--remargins: not allowed with argument --require"),
                      (full + ["-d"], b"--remargins: not allowed with argument -d/--dump"),
                      (full + ["--gpus", "2"], b"--remargins: not available with --gpus above 1")):
        r = subprocess.run(exe + bad, capture_output=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    r = subprocess.run(exe + full, capture_output=True, timeout=120, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and b"--remargins: not available under a multi-rank launch" in r.stderr
    assert not mg.exists()


# ---- the lemma, restated ----
# Forward: an in-place Bellman-Ford from the source in which an unreached node is never relaxed (§16).  R: the nodes it reached.  Reverse:
# a Bellman-Ford from the target over the reversed edges in which only nodes of R are ever given a value.  A cycle of negative length the
# source does not reach is none of the forward solve's; a cycle with one node in R lies in R entirely (R is closed under out-edges).  So
# wherever the forward solve settles, the restricted reverse pass does, within V + 1 rounds.


def forward(V, edges, s):
    """(dist, settled): `settled` False when V + 1 rounds still change something."""
    d = [None] * V
    d[s] = 0
    for _ in range(V + 1):
        ch = False
        for u, v, w in edges:
            if d[u] is None:
                continue  # an unreached node is never relaxed
            if d[v] is None or d[u] + w < d[v]:
                d[v], ch = d[u] + w, True
        if not ch:
            return d, True
    return d, False


def reverse_in(V, edges, t, R):
    """(d_t restricted to R, the rounds it took) or (None, V + 2) when it does not settle within V + 1 rounds."""
    d = [None] * V
    if R[t]:
        d[t] = 0
    for rounds in range(1, V + 2):
        ch = False
        for u, v, w in edges:
            if not R[u] or d[v] is None:
                continue  # a node outside R is never given a value
            if d[u] is None or d[v] + w < d[u]:
                d[u], ch = d[v] + w, True
        if not ch:
            return d, rounds
    return None, V + 2


def reverse_free(V, edges, t):
    """The unrestricted reverse pass: whether it settles within V + 1 rounds."""
    return reverse_in(V, edges, t, [True] * V)[0] is not None


def draw_graph(rng, V, trap):
    """Nodes 0 .. V-1 in position order, source V-2 and target V-1 as on the device: mostly forward edges, a few backward ones whose
    cycles stay positive, and with `trap` a negative cycle the source does not reach but that reaches the target."""
    s, t = V - 2, V - 1
    inner = V - 2 - (2 if trap else 0)  # the trap's two nodes are inner, inner + 1
    edges = set()
    for v in range(min(3, inner)):
        edges.add((s, v))
    for u in range(inner):
        for v in range(u + 1, min(inner, u + 5)):
            if rng.random() < 0.55:
                edges.add((u, v))
        if u >= inner - 3 or rng.random() < 0.1:
            edges.add((u, t))
    out = [(u, v, rng.randint(-40, 25)) for u, v in sorted(edges)]
    for _ in range(rng.randint(1, 4)):  # backward (overlap) edges: heavier than any forward detour of up to 4 steps can repay
        u = rng.randint(1, max(1, inner - 1))
        v = rng.randint(max(0, u - 4), u - 1) if u > 0 else 0
        if u != v and (u, v) not in edges and (v, u) in edges:
            edges.add((u, v))
            out.append((u, v, 200 + rng.randint(0, 50)))
    if trap:
        a, b = inner, inner + 1
        out += [(a, b, -7), (b, a, 3), (b, t, 5), (a, rng.randint(0, max(0, inner - 1)), 2)]  # a <-> b sums to -4; nothing leads into them
    rng.shuffle(out)
    return out, s, t


def simple_paths(V, adj, a, z, banned=()):
    """Lengths of all simple a -> z paths (a == z: the empty path)."""
    best = [None]

    def go(u, seen, acc):
        if u == z:
            best[0] = acc if best[0] is None or acc < best[0] else best[0]
            return
        for v, w in adj[u]:
            if v not in seen:
                go(v, seen | {v}, acc + w)

    go(a, {a} | set(banned), 0)
    return best[0]


def test_the_restricted_reverse_pass_settles_wherever_the_forward_solve_does():
    rng = random.Random(2101)
    settled = traps_free_fails = brute = 0
    for trial in range(400):
        V = rng.randint(8, 40) if trial % 4 else rng.randint(8, 10)
        trap = trial % 3 == 0
        edges, s, t = draw_graph(rng, V, trap)
        ds, ok = forward(V, edges, s)
        if not ok:
            continue  # (a negative cycle the source reaches: the forward solve says PHX_S_NEGCYCLE, no margins are asked for)
        settled += 1
        R = [x is not None for x in ds]
        dt, rounds = reverse_in(V, edges, t, R)
        assert dt is not None and rounds <= V + 1, (trial, V, trap)
        assert all(dt[v] is None for v in range(V) if not R[v])
        if trap:
            assert not R[V - 4] and not R[V - 3]
            traps_free_fails += not reverse_free(V, edges, t)  # the unrestricted pass runs into the trap
        D = ds[t]
        if D is None:
            assert dt[t] is None and all(x is None for x in dt)  # the target is outside R: nothing gets a value
            continue
        assert dt[s] == D and dt[t] == 0
        # every edge inside R has Delta' >= 0; the edges of a forward shortest path have Delta' = 0
        for u, v, w in edges:
            if R[u] and dt[v] is not None:
                assert ds[u] + w + dt[v] - D >= 0, (trial, u, v)
        v, hops = t, 0
        while v != s:
            u, w = next((u, w) for u, x, w in edges if x == v and ds[u] is not None and ds[u] + w == ds[v])
            assert ds[u] + w + dt[v] - D == 0
            v, hops = u, hops + 1
            assert hops <= V
        # ... and on the small graphs the two vectors are the definition's: minima over simple paths (no negative cycle inside R)
        if V <= 10:
            adj = [[] for _ in range(V)]
            for u, v, w in edges:
                if R[u] and R[v]:
                    adj[u].append((v, w))
            for v in range(V):
                if R[v]:
                    assert simple_paths(V, adj, s, v) == ds[v], (trial, v)
                    assert simple_paths(V, adj, v, t) == dt[v], (trial, v)
            brute += 1
    assert settled >= 300 and traps_free_fails >= 50 and brute >= 40, (settled, traps_free_fails, brute)
