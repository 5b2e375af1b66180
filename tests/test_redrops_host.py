"""Host side of the re-annotation drop margins (no GPU): the new entry points in the header, the export list and the Python
binding; the refusals of --redrop-margins and their place in the order; and §12's algorithm — the restatement of tests/test_drop_host.py,
imported, not copied — on the graph G' of a policy (refused edges, biases of both signs) restricted to the nodes R the forward solve
reaches, against brute force over the simple source -> target paths of G' - p_j."""
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from test_drop_host import bellman_ford, drop_margins, random_graph  # noqa: E402

NEW = ("phx_redrops_flat", "phx_redrops_ms", "phx_redrop_stats")


# ---- 1. declarations ----
def test_redrop_entry_points_are_declared_exported_and_bound():
    import ctypes as C

    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int phx_redrops_flat\(phx_ctx \*ctx, phx_gene_drop \*rec, int64_t cap, int64_t \*offsets\s*, int32_t \*status\s*, int64_t \*total\);", code)
    assert re.search(r"int phx_redrops_ms\(phx_ctx \*ctx, float \*ms\s*\);", code)
    assert re.search(r"int phx_redrop_stats\(phx_ctx \*ctx, int64_t \*out\s*\);", code)
    assert "#define PHX_VERSION 410" in text and "phx_redrops_flat, phx_redrops_ms, phx_redrop_stats — probe for the symbol" in text
    assert set(NEW) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert L.phx_version() == 410
    assert L.phx_redrops_flat.argtypes == L.phx_drop_margins_flat.argtypes and len(L.phx_redrops_flat.argtypes) == 6
    assert L.phx_redrops_ms.argtypes == L.phx_drop_ms.argtypes and L.phx_redrop_stats.argtypes == L.phx_drop_stats.argtypes
    assert L.phx_redrops_flat(None, None, 0, None, None, None) == -1  # PHX_E_ARG: no context
    assert L.phx_redrops_ms(None, None) == -1 and L.phx_redrop_stats(None, None) == -1
    ms, out = (C.c_float * 4)(), (C.c_int64 * 4)()
    assert L.phx_redrops_ms(None, ms) == -1 and L.phx_redrop_stats(None, out) == -1
    for name in ("redrops", "redrops_ms", "redrop_stats"):
        assert callable(getattr(api.Annotator, name)), name
    assert api._MS_KEYS["phx_redrops_ms"] == api._MS_KEYS["phx_drop_ms"]


# ---- 2. the command line ----
def refusal(argv, world, tmp_path, monkeypatch):
    """Whether get_args refuses `argv` (F: an entry file, O: an output)."""
    from phanotate_amd import cli

    fasta = tmp_path / "x.fasta"
    fasta.write_text(">c1\nacgtacgtacgt\n")
    given = tmp_path / "f.txt"
    given.write_text("1\t9\t+\tc1\t-1.0\n")
    monkeypatch.setenv("WORLD_SIZE", str(world))
    try:
        cli.get_args([str(fasta)] + [{"F": str(given), "O": str(tmp_path / "o.txt")}.get(word, word) for word in argv.split()])
    except SystemExit as e:
        assert e.code == 2
        return "refused"
    return "ok"


CASES = (
    ("--redrop-margins F --forbid F", 1, "argument --redrop-margins: needs --reannotation"),
    ("--redrop-margins F", 1, "argument --redrop-margins: needs --reannotation"),
    ("--redrop-margins F --require F --reannotation O", 1, "argument --redrop-margins: not allowed with argument --require"),
    ("--redrop-margins F --forbid F --reannotation O -d", 1, "argument --redrop-margins: not allowed with argument -d/--dump"),
    ("--redrop-margins F --forbid F --reannotation O --gpus 2", 1, "argument --redrop-margins: not available with --gpus above 1"),
    ("--redrop-margins F --forbid F --reannotation O", 2, "argument --redrop-margins: not available under a multi-rank launch"),
    ("--redrop-margins F --forbid F --reannotation O", 1, "ok"),
    ("--redrop-margins F --evidence F --forbid F --reannotation O --remargins F", 1, "ok"),
    # the first message is the one _CHECK_ORDER dictates: remargins in front, pin-margins and the entry files behind
    ("--redrop-margins F --remargins F --forbid F", 1, "argument --remargins: needs --reannotation"),
    ("--redrop-margins F --remargins F --require F --reannotation O", 1, "argument --remargins: not allowed with argument --require"),
    ("--redrop-margins F --pin-margins F --forbid F", 1, "argument --redrop-margins: needs --reannotation"),
    ("--redrop-margins F --pin-margins F --require F --reannotation O", 1, "argument --redrop-margins: not allowed with argument --require"),
    ("--redrop-margins F --require F", 1, "argument --redrop-margins: not allowed with argument --require"),  # (its own rules in _RULES' order)
    ("--redrop-margins F --evidence F", 1, "argument --redrop-margins: needs --reannotation"),
    ("--redrop-margins F --curated-scan F O --reannotation O", 1, "argument --curated-scan: needs --require"),
    ("--redrop-margins F --drop-margins F -d", 1, "argument --drop-margins: not allowed with argument -d/--dump"),
    ("--redrop-margins F --pin-margins F -d", 1, "argument --redrop-margins: not allowed with argument -d/--dump"),
    ("--redrop-margins F --remargins F --gpus 2 --forbid F --reannotation O", 1, "argument --remargins: not available with --gpus above 1"),
)


@pytest.mark.parametrize("argv, world, want", CASES)
def test_redrop_margins_refusals_and_their_order(argv, world, want, tmp_path, monkeypatch, capsys):
    got = refusal(argv, world, tmp_path, monkeypatch)
    err = capsys.readouterr().err
    if want == "ok":
        assert got == "ok", err
    else:
        assert got == "refused" and err.rstrip().endswith("error: " + want), err


def test_redrop_margins_has_its_place_in_the_table():
    from phanotate_amd import cli

    row = cli.OUTPUTS["redrop_margins"]
    assert row.flag == "--redrop-margins" and row.fmt is cli.format_drops and row.mode == "wb" and row.resident and row.piped is None
    for order in (cli._CHECK_ORDER, cli._FETCH_ORDER):
        assert order.index("redrop_margins") == order.index("remargins") + 1
    rules = [m for about, _, m in cli._RULES if about == "redrop_margins"]
    assert rules == [m.replace("--remargins", "--redrop-margins") for about, _, m in cli._RULES if about == "remargins"]


# ---- 3. the algorithm on a policy's graph ----
def forward(V, edges, s):
    """In-place Bellman-Ford with parents that never relaxes an unreached node; None: it does not settle (a cycle of negative length the
    source reaches)."""
    d, par = [None] * V, [None] * V
    d[s] = 0
    for _ in range(V + 1):
        ch = False
        for u, v, w in edges:
            if d[u] is None:
                continue
            if d[v] is None or d[u] + w < d[v]:
                d[v], par[v], ch = d[u] + w, u, True
        if not ch:
            return d, par
    return None, None


def policy_graph(rng, V):
    """random_graph(V - extra) as G, a trap beside it, a refused set and biases of both signs.  Returns (V, G' as the kernels see it: the
    edges that are not refused, weighing W + B; whether a trap was added)."""
    extra = rng.choice([0, 0, 2, 3])
    if V - extra < 5:
        extra = 0
    Vg = V - extra
    base = random_graph(rng, Vg)
    # node ids: G's source and target stay the last two of the whole graph; the trap's nodes sit between
    ren = lambda v: v if v < Vg - 2 else v + extra
    edges = [(ren(a), ren(b), w) for a, b, w in base]
    trap = extra > 0
    if trap:  # a cycle of negative length the source cannot reach, with edges into the graph and into the target
        t = list(range(Vg - 2, Vg - 2 + extra))
        for k, a in enumerate(t):
            edges.append((a, t[(k + 1) % extra], -rng.randint(1, 4)))
        edges.append((t[0], V - 1, rng.randint(-3, 3)))
        edges.append((t[-1], rng.randrange(Vg - 2), rng.randint(-3, 3)))
        rng.shuffle(edges)
    n_ref = rng.choice([0, 1, 1, 2, 3])
    refused = set(rng.sample(range(len(edges)), min(n_ref, len(edges))))
    bias = {}
    for k in rng.sample(range(len(edges)), min(rng.choice([0, 1, 2, 4]), len(edges))):
        bias[k] = rng.choice([-2, -1, -1, 1, 2, 5, 9])
    gp = [(u, v, w + bias.get(k, 0)) for k, (u, v, w) in enumerate(edges) if k not in refused]  # (refusal wins over a bias)
    return gp, trap


def brute(V, edges, s, t, skip):
    """Length of the shortest simple s -> t path that avoids `skip`; None: there is none."""
    out = {}
    for u, v, w in edges:
        out.setdefault(u, []).append((v, w))
    best = [None]

    def walk(v, seen, acc):
        if v == t:
            if best[0] is None or acc < best[0]:
                best[0] = acc
            return
        for z, w in out.get(v, ()):
            if z != skip and z not in seen:
                seen.add(z)
                walk(z, seen, acc + w)
                seen.discard(z)

    walk(s, {s}, 0)
    return best[0]


def check_policy_graph(rng, V, layered):
    """None: discarded (the forward solve reports a cycle of negative length); else (slots checked, slots with cross nodes, layered builds,
    the unrestricted reverse pass would not have settled)."""
    gp, trap = policy_graph(rng, V)
    s, t = V - 2, V - 1
    ds, par = forward(V, gp, s)
    if ds is None:
        return None
    if ds[t] is None:  # PHX_S_NOPATH: no called gene, no records
        return 0, 0, 0, False
    in_R = [x is not None for x in ds]
    er = [e for e in gp if in_R[e[0]]]  # R is closed under G''s out-edges
    assert all(in_R[v] for _, v, _ in er)
    dt = bellman_ford(V, er, t, reverse=True)  # settles: a cycle with one node in R lies in R, and the forward solve settled
    P, v = [t], t
    while v != s:
        v = par[v]
        P.append(v)
        assert len(P) <= V
    P.reverse()
    assert len(P) >= 3 and ds[t] == dt[s] and all(ds[v] + dt[v] == ds[t] for v in P)  # P' is tight under both vectors
    best, n_cross, lay = drop_margins(V, er, P, ds, dt, rng, layered)
    for j in range(1, len(P) - 1):
        d = brute(V, gp, s, t, P[j])  # over G' itself: the restriction to R loses nothing
        want = None if d is None else d - ds[t]
        assert best[j] == want, (gp, P, j, best[j], want)
        assert want is None or want >= 0
    unsettled = False
    if trap:
        try:
            bellman_ford(V, gp, t, reverse=True)
        except AssertionError:
            unsettled = True
    return len(P) - 2, n_cross, int(lay), unsettled


@pytest.mark.parametrize("seed, layered, draws", ((2901, False, 1500), (2902, True, 600)))
def test_restatement_on_a_policy_equals_brute_force(seed, layered, draws):
    rng = random.Random(seed)
    drawn = gone = slots = cross = lay = traps = 0
    for _ in range(draws):
        drawn += 1
        r = check_policy_graph(rng, rng.randint(5, 10), layered)
        if r is None:
            gone += 1
            continue
        slots += r[0]
        cross += r[1]
        lay += r[2]
        traps += r[3]
    print("seed %d: %d drawn, %d discarded, %d slots, %d with cross nodes, %d layered, %d traps" % (seed, drawn, gone, slots, cross, lay, traps))
    assert 10 * gone <= drawn, (gone, drawn)  # only the graphs whose forward solve reports a negative cycle, at most 10 %
    assert slots > drawn - gone and cross > 10 and lay > 0 and traps > 20, (slots, cross, lay, traps)
