"""Host side of the pinned margins (no GPU): the header, the export list, the Annotator's methods and --pin-margins'
refusals; the definition Delta'' = d_s'(u) + W'(e) + d_t'(v) - D' under W' = W + B - M·[R'] against brute force over paths ordered by
(-c, S) on small random graphs, with its decoding into (lost, s) and the restricted reverse pass's round count; and, on the CPU oracle's
graphs of the seeded mixes the GPU test hands to the device, the sign of Delta'', both signs of s beside lost > 0 and the "pin one more"
theorem through the yardstick's own solver."""
import os
import random
import re
import subprocess
import sys

import numpy as np

from conftest import ROOT
from test_curate_host import curated, random_graph, simple_paths
from test_evidence_gpu import settle


# ---- the interface ----
def test_header_exports_methods_and_cli_refusals(tmp_path):
    from phanotate_amd import _lib, api, cli

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    m = re.search(r"int phx_pinmargins_flat\(([^;]*)\);", text)
    assert m is not None
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "rec", "lost", "cap", "offsets", "status", "total"]
    assert args[1] == "phx_orf_margin *rec" and args[2] == "int32_t *lost"
    assert re.search(r"int phx_pinmargins_ms\(phx_ctx \*ctx, float \*ms", text)
    assert re.search(r"int phx_tap_pindist\(phx_ctx \*ctx, int32_t contig, int32_t which, uint64_t \*dist_limbs, int64_t cap_words, int32_t \*words_per_node\);", text)
    assert re.search(r"#define PHX_VERSION 410\b", text)  # callers probe for the symbol
    for name in ("phx_pinmargins_flat", "phx_pinmargins_ms", "phx_tap_pindist"):
        assert name in _lib.EXPORTS
    L = _lib.lib()
    assert len(L.phx_pinmargins_flat.argtypes) == 7 and len(L.phx_tap_pindist.argtypes) == 6 and len(L.phx_pinmargins_ms.argtypes) == 2
    assert L.phx_pinmargins_flat(None, None, None, 0, None, None, None) == -1  # PHX_E_ARG without a context
    assert L.phx_tap_pindist(None, 0, 0, None, 0, None) == -1 and L.phx_pinmargins_ms(None, None) == -1
    assert callable(api.Annotator.pinmargins) and callable(api.Annotator.pinmargins_ms) and callable(api.Annotator.pindist)
    assert callable(cli.format_pin_margins)
    # the command line: what --pin-margins needs and where it is refused, before any device is touched
    rq = tmp_path / "r.txt"
    rq.write_text("1\t9\t+\tc1\n")
    ev = tmp_path / "e.txt"
    ev.write_text("1\t9\t+\tc1\t-2.5\n")
    out, pm, fasta = tmp_path / "o.txt", tmp_path / "p.txt", tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    exe = [sys.executable, os.path.join(ROOT, "phanotate.py"), str(fasta)]
    full = ["--require", str(rq), "--reannotation", str(out), "--pin-margins", str(pm)]
    for bad, word in ((["--pin-margins", str(pm)], b"--pin-margins: needs --require"),
                      (["--forbid", str(rq), "--reannotation", str(out), "--pin-margins", str(pm)], b"--pin-margins: needs --require"),
                      (["--require", str(rq), "--pin-margins", str(pm)], b"--pin-margins: needs --reannotation"),
                      (full + ["-d"], b"--pin-margins: not allowed with argument -d/--dump"),
                      (full + ["--gpus", "2"], b"--pin-margins: not available with --gpus above 1"),
                      (full + ["--remargins", str(pm)], b"--remargins: not allowed with argument --require"),  # the siblings' refusals stand
                      (full + ["--evidence", str(ev)], b"--evidence: not allowed with argument --require")):
        r = subprocess.run(exe + bad, capture_output=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    r = subprocess.run(exe + full, capture_output=True, timeout=120, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and b"--pin-margins: not available under a multi-rank launch" in r.stderr
    # the file's layout
    rec = np.zeros(3, _lib.MARGIN_DT)
    rec["left"], rec["right"], rec["strand"], rec["through"] = [40, 10, 10], [90, 60, 60], [1, -1, 1], [1, 1, 0]
    rec["score"], rec["margin"], rec["called"] = [-1.5, 2.0, 0.0], [0.0, -0.25, np.inf], [1, 0, 0]
    got = cli.format_pin_margins(["c1", "bad"], np.array([0, -2], np.int32), np.array([0, 3, 3], np.int64), rec, np.array([0, 2, 0], np.int32))
    assert got == (b"#id:\tc1\n#START\tSTOP\tFRAME\tCONTIG\tSCORE\tMARGIN\tLOST\tCALLED\n"
                   b"60\t10\t-\tc1\t2.000000E+00\t-2.500000E-01\t2\t0\n40\t90\t+\tc1\t-1.500000E+00\t0.000000E+00\t0\t1\n")


# ---- the definition on small graphs ----
def reverse_in_R(V, kept, ds, t):
    """(d_t', rounds): Bellman-Ford from t over the kept edges reversed, using only edges whose source the forward solve reached (a node
    outside R_n never gets a value); `rounds` counts the sweeps, the last of which changes nothing.  None: not settled in V + 1 rounds."""
    use = [e for e in kept if ds[e[0]] is not None]
    d = [None] * V
    if ds[t] is not None:
        d[t] = 0
    for rnd in range(V + 1):
        ch = False
        for u, v, w in use:
            if d[v] is not None and (d[u] is None or d[v] + w < d[u]):
                d[u], ch = d[v] + w, True
        if not ch:
            return d, rnd + 1
    return None, V + 1


def best_pair(V, edges, R, F, B, a, z):
    """min (-c, S) over the simple a -> z paths of G_{F,B} (a == z: the empty path), or None."""
    out_of = [[] for _ in range(V)]
    for k, (u, v, _) in enumerate(edges):
        if k not in F:
            out_of[u].append(k)
    best, stack = None, [(a, 0, 0, {a})]
    while stack:
        u, c, S, seen = stack.pop()
        if u == z:
            if best is None or (-c, S) < best:
                best = (-c, S)
            continue
        for k in out_of[u]:
            v = edges[k][1]
            if v not in seen:
                stack.append((v, c + (k in R), S + edges[k][2] + B[k], seen | {v}))
    return best


def on_cycle(V, edges, F, k):
    """Edge k of G_F lies on a cycle: its head reaches its tail."""
    u, v, _ = edges[k]
    return best_pair(V, edges, set(), F, [0] * len(edges), v, u) is not None


def decode_limbs(x, bits):
    """(lost, s) of Delta'' as the device decodes it with M = 2^bits: the top limb plus the sign bit of the limbs below, and the low
    `bits` bits read as two's complement."""
    low = x & ((1 << bits) - 1)
    sign = low >> (bits - 1)
    return (x >> bits) + sign, low - (sign << bits)


def test_delta_is_the_lexicographic_gap_of_the_best_path_through_each_edge():
    rng = random.Random(2400)
    settled = records = gave_up = negative_s = on_a_cycle = worst_rounds = 0
    while settled < 2200:
        V, edges, R, F, B = random_graph(rng)
        R = R - F
        bound = sum(abs(w) for _, _, w in edges) + sum(abs(b) for b in B)
        paths = simple_paths(V, edges, F)
        per_m = []
        for M, bits in ((bound + 1, None), (1 << 200, 200)):
            kept = curated(V, edges, R, F, B, M)
            orig = [k for k in range(len(edges)) if k not in F]
            ds, par = settle(V, kept, 0)
            if ds is None or ds[V - 1] is None:
                per_m.append(None)
                continue
            dt, rounds = reverse_in_R(V, kept, ds, V - 1)
            assert dt is not None and rounds <= V + 1, (edges, R, F, B)  # §21's lemma, verbatim
            worst_rounds = max(worst_rounds, rounds)
            assert dt[0] == ds[V - 1]
            cs, Ss = min((-sum(k in R for k in p), sum(edges[k][2] + B[k] for k in p)) for p in paths)
            assert ds[V - 1] == Ss + cs * M
            out = {}
            for (u, v, w), k in zip(kept, orig):
                if ds[u] is None or dt[v] is None:
                    out[k] = None
                    continue
                delta = ds[u] + w + dt[v] - ds[V - 1]
                assert delta >= 0
                # the best walk through k whose two sides are simple paths; a simple path itself unless k lies on a cycle
                head, tail = best_pair(V, edges, R, F, B, 0, u), best_pair(V, edges, R, F, B, v, V - 1)
                ce, Se = head[0] + tail[0] - (k in R), head[1] + tail[1] + edges[k][2] + B[k]
                lost, s = ce - cs, Se - Ss
                assert delta == lost * M + s, (edges, R, F, B, k)
                assert (lost, s) >= (0, 0)
                if bits:
                    assert decode_limbs(delta, bits) == (lost, s)
                through = [p for p in paths if k in p]
                if not on_cycle(V, edges, F, k):  # ... then brute force over the simple paths through k says the same
                    assert through and min((-sum(j in R for j in p), sum(edges[j][2] + B[j] for j in p)) for p in through) == (ce, Se), (edges, R, F, B, k)
                else:
                    on_a_cycle += bits is not None
                    assert all((-sum(j in R for j in p), sum(edges[j][2] + B[j] for j in p)) >= (ce, Se) for p in through)
                out[k] = (lost, s)
                if bits:
                    records += 1
                    gave_up += lost > 0
                    negative_s += lost > 0 and s < 0
            for k in range(len(edges)):  # no value on a side: no path runs through the edge
                if k not in F and out[k] is None:
                    assert not any(k in p for p in paths)
            # every edge of the best path has Delta'' = 0
            v = V - 1
            while v != 0:
                assert out[orig[par[v]]] == (0, 0)
                v = kept[par[v]][0]
            per_m.append(out)
        assert (per_m[0] is None) == (per_m[1] is None)
        if per_m[0] is None:
            continue
        assert per_m[0] == per_m[1]  # any M above the walk sums: the same lost and the same s
        settled += 1
    print("small graphs: %d settle, %d edge records, %d give up a pin (%d of them with s < 0), %d on a cycle, at most %d rounds" % (settled, records, gave_up, negative_s, on_a_cycle, worst_rounds))
    assert settled >= 2000 and gave_up >= 500 and negative_s >= 100 and on_a_cycle >= 100, (settled, gave_up, negative_s, on_a_cycle)


# ---- the seeded mixes on the CPU oracle's graphs ----
def pin_margins(g, d, M):
    """(d_s'(target), {ORF key: Delta''}) of draw d on the oracle's graph g — the keys with an edge of G' and a value on both sides —, or
    None where the solve does not settle or finds no path."""
    import curate_draws as cd

    from test_margins_gpu import sweep_idx

    edges, pinned = cd.weights(g.edges, g.orf_edge, d, M)
    ds, par = settle(g.V, edges, g.src)
    if ds is None or ds[g.tgt] is None:
        return None
    assert (g.src, g.tgt) == (g.V - 2, g.V - 1)
    dt, rounds = reverse_in_R(g.V, sorted(edges, key=lambda e: sweep_idx(e[0], g.V)), ds, g.tgt)
    assert dt is not None and dt[g.src] == ds[g.tgt]
    wmap = {(u, v): w for u, v, w in edges}
    out = {}
    for key, e in g.orf_edge.items():
        if e in wmap and ds[e[0]] is not None and dt[e[1]] is not None:
            out[key] = ds[e[0]] + wmap[e] + dt[e[1]] - ds[g.tgt]
    path = []
    v = g.tgt
    while v != g.src:
        path.append((edges[par[v]][0], v))
        v = edges[par[v]][0]
    return ds[g.tgt], out, path


def split(x, M):
    """(lost, s) of x = lost * M + s with |s| < M / 2."""
    lost = (x + M // 2) // M
    return lost, x - lost * M


def test_the_mixes_on_the_oracles_graphs_and_pin_one_more(oracle):
    import phanotate_amd as pa

    import curate_draws as cd

    graphs = [cd.OracleGraph(oracle, s) for s in cd.mix_seqs(pa)]
    rng = np.random.RandomState(2401)
    draws = ok = records = points = cycles = 0
    hist, neg, pos = {}, 0, 0
    from_zero = from_more = 0
    for row in cd.mixes(graphs):
        for g, d in zip(graphs, row):
            if d is None:
                continue
            draws += 1
            M = 1 << (cd.big_m(g.edges, d).bit_length() + 2)  # a power of two above four times every walk sum, as the device's 2^(64 NL)
            res = pin_margins(g, d, M)
            if res is None:
                continue
            ok += 1
            D, delta, path = res
            cs, Ss = split(D, M)  # (-c*, S*)
            by_edge = {e: k for k, e in g.orf_edge.items()}
            for e in path:
                if e in by_edge:
                    assert delta[by_edge[e]] == 0
            zero, more = [], []
            for key in sorted(delta):
                x = delta[key]
                assert x >= 0, (key, x)
                lost, s = split(x, M)
                assert lost >= 0 and (lost, s) >= (0, 0)
                records += 1
                hist[lost] = hist.get(lost, 0) + 1
                neg += lost > 0 and s < 0
                pos += lost > 0 and s > 0
                if key not in d["require"] and key not in d["forbid"]:
                    (zero if lost == 0 else more).append(key)
            # pin one more: up to 3 ORFs that give up no pin and up to 2 that do
            pick = lambda pool, m: [pool[j] for j in sorted(rng.choice(len(pool), min(m, len(pool)), replace=False).tolist())] if pool else []
            for key in pick(zero, 3) + pick(more, 2):
                lost, s = split(delta[key], M)
                edges2, _ = cd.weights(g.edges, g.orf_edge, dict(d, require=list(d["require"]) + [key]), M)
                ds2, _ = settle(g.V, edges2, g.src)
                points += 1
                from_zero += lost == 0
                from_more += lost > 0
                if ds2 is None:  # the ORF lies on a cycle the source reaches
                    cycles += 1
                    continue
                want = min((cs, Ss), (cs + lost - 1, Ss + s))  # (-c, S): the present optimum, or the best path through the ORF
                assert split(ds2[g.tgt], M) == want, (key, lost, s, split(ds2[g.tgt], M), want)
    print("mixes on the oracle's graphs: %d draws, %d settle; %d ORF records, lost: %s, with lost > 0: %d have s < 0 and %d have s > 0; pin one more at %d points "
          "(%d with lost = 0, %d with lost >= 1), %d of them end in a cycle" % (draws, ok, records, sorted(hist.items()), neg, pos, points, from_zero, from_more, cycles))
    assert draws == 45 and ok == 45, (draws, ok)  # what tests/test_curate_host.py records
    assert neg > 0 and pos > 0 and from_zero >= 45 and from_more >= 20
    assert cycles * 10 <= points, (cycles, points)
