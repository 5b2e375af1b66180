"""Host side of the re-annotation replacements (no GPU): the four new entry points in the header, the export list and the
Python binding; the row of --redrop-replacements, its refusals and their place in the order; and §13's witness construction — the
restatement of tests/test_replace_host.py on the policy graphs of tests/test_redrops_host.py, both imported, not copied — on G'[R] against
brute force over the simple source -> target paths of G' - p_j."""
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_drop_host import bellman_ford, shortest_path  # noqa: E402
from test_redrops_host import brute, forward, policy_graph, refusal  # noqa: E402
from test_replace_host import check_witnesses, loop_graph, witnesses  # noqa: E402

NEW = ("phx_rereplacements_flat", "phx_tap_rereplacement", "phx_rereplacements_ms", "phx_rereplacement_stats")
SIBLING = dict(zip(NEW, ("phx_replacements_flat", "phx_tap_replacement", "phx_replacements_ms", "phx_replacement_stats")))


# ---- 1. declarations ----
def test_rereplacement_entry_points_are_declared_exported_and_bound():
    import ctypes as C

    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int phx_rereplacements_flat\(phx_ctx \*ctx, phx_gene_repl \*rec, int64_t cap, phx_gene \*genes, int64_t gene_cap, int64_t \*offsets\s*,\s*"
                     r"int32_t \*status\s*, int64_t \*total, int64_t \*gene_total\);", code)
    assert re.search(r"int phx_tap_rereplacement\(phx_ctx \*ctx, int32_t contig, int32_t k, int32_t \*path, int32_t cap, int32_t \*n_path\);", code)
    assert re.search(r"int phx_rereplacements_ms\(phx_ctx \*ctx, float \*ms\s*\);", code)
    assert re.search(r"int phx_rereplacement_stats\(phx_ctx \*ctx, int64_t \*out\s*\);", code)
    assert "#define PHX_VERSION 410" in text
    assert "(additions, version unchanged) phx_rereplacements_flat, phx_tap_rereplacement, phx_rereplacements_ms, phx_rereplacement_stats — probe for the symbol" in text
    assert set(NEW) <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert L.phx_version() == 410
    for name in NEW:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes == getattr(L, SIBLING[name]).argtypes and getattr(L, name).restype == getattr(L, SIBLING[name]).restype, name
    assert len(L.phx_rereplacements_flat.argtypes) == 9 and len(L.phx_tap_rereplacement.argtypes) == 6
    n = C.c_int32(7)
    ms, out = (C.c_float * 3)(), (C.c_int64 * 5)()
    assert L.phx_rereplacements_flat(None, None, 0, None, 0, None, None, None, None) == -1  # PHX_E_ARG: no context
    assert L.phx_tap_rereplacement(None, 0, 0, None, 0, C.byref(n)) == -1
    assert L.phx_rereplacements_ms(None, ms) == -1 and L.phx_rereplacement_stats(None, out) == -1
    for name in ("rereplacements", "rereplacement_path", "rereplacements_ms", "rereplacement_stats"):
        assert callable(getattr(api.Annotator, name)), name
    assert api._MS_KEYS["phx_rereplacements_ms"] == api._MS_KEYS["phx_replacements_ms"]


# ---- 2. the command line ----
CASES = (
    ("--redrop-replacements F --forbid F", 1, "argument --redrop-replacements: needs --reannotation"),
    ("--redrop-replacements F", 1, "argument --redrop-replacements: needs --reannotation"),
    ("--redrop-replacements F --require F --reannotation O", 1, "argument --redrop-replacements: not allowed with argument --require"),
    ("--redrop-replacements F --forbid F --reannotation O -d", 1, "argument --redrop-replacements: not allowed with argument -d/--dump"),
    ("--redrop-replacements F --forbid F --reannotation O --gpus 2", 1, "argument --redrop-replacements: not available with --gpus above 1"),
    ("--redrop-replacements F --forbid F --reannotation O", 2, "argument --redrop-replacements: not available under a multi-rank launch"),
    ("--redrop-replacements F --forbid F --reannotation O", 1, "ok"),
    ("--redrop-replacements F --evidence F --forbid F --reannotation O --redrop-margins F --remargins F", 1, "ok"),
    # the first message is the one _CHECK_ORDER dictates: remargins and redrop-margins in front, pin-margins and the entry files behind
    ("--redrop-replacements F --redrop-margins F --forbid F", 1, "argument --redrop-margins: needs --reannotation"),
    ("--redrop-replacements F --redrop-margins F --require F --reannotation O", 1, "argument --redrop-margins: not allowed with argument --require"),
    ("--redrop-replacements F --remargins F --forbid F", 1, "argument --remargins: needs --reannotation"),
    ("--redrop-replacements F --pin-margins F --forbid F", 1, "argument --redrop-replacements: needs --reannotation"),
    ("--redrop-replacements F --pin-margins F --require F --reannotation O", 1, "argument --redrop-replacements: not allowed with argument --require"),
    ("--redrop-replacements F --require F", 1, "argument --redrop-replacements: not allowed with argument --require"),  # (its own rules in _RULES' order)
    ("--redrop-replacements F --evidence F", 1, "argument --redrop-replacements: needs --reannotation"),
    ("--redrop-replacements F --curated-scan F O --reannotation O", 1, "argument --curated-scan: needs --require"),
    ("--redrop-replacements F --drop-replacements F -d", 1, "argument --drop-replacements: not allowed with argument -d/--dump"),
    ("--redrop-replacements F --pin-margins F -d", 1, "argument --redrop-replacements: not allowed with argument -d/--dump"),
    ("--redrop-replacements F --redrop-margins F --gpus 2 --forbid F --reannotation O", 1, "argument --redrop-margins: not available with --gpus above 1"),
)


@pytest.mark.parametrize("argv, world, want", CASES)
def test_redrop_replacements_refusals_and_their_order(argv, world, want, tmp_path, monkeypatch, capsys):
    got = refusal(argv, world, tmp_path, monkeypatch)
    err = capsys.readouterr().err
    if want == "ok":
        assert got == "ok", err
    else:
        assert got == "refused" and err.rstrip().endswith("error: " + want), err


def test_redrop_replacements_has_its_place_in_the_table():
    from phanotate_amd import cli

    row = cli.OUTPUTS["redrop_replacements"]
    assert row.flag == "--redrop-replacements" and row.fmt is cli.format_replacements and row.mode == "wb" and row.resident and row.piped is None
    assert row.merge is cli.OUTPUTS["drop_replacements"].merge  # (gene_off counts per batch)
    for order in (cli._CHECK_ORDER, cli._FETCH_ORDER):
        assert order.index("redrop_replacements") == order.index("redrop_margins") + 1 == order.index("remargins") + 2
    rules = [m for about, _, m in cli._RULES if about == "redrop_replacements"]
    assert len(rules) == 2 and rules == [m.replace("--redrop-margins", "--redrop-replacements") for about, _, m in cli._RULES if about == "redrop_margins"]


# ---- 3. the construction on a policy's graph ----
def check_policy_witnesses(rng, V, layered, it):
    """None: discarded (the forward solve reports a cycle of negative length); else (slots with a witness, cross winners, delta chains longer
    than one node, loops cut)."""
    gp, _ = policy_graph(rng, V)
    s, t = V - 2, V - 1
    ds, par = forward(V, gp, s)
    if ds is None:
        return None
    if ds[t] is None:  # PHX_S_NOPATH: no called gene, no records
        return 0, 0, 0, 0
    in_R = [x is not None for x in ds]
    er = [e for e in gp if in_R[e[0]]]  # G'[R]: R is closed under G''s out-edges
    dt = bellman_ford(V, er, t, reverse=True)
    P, v = [t], t
    while v != s:
        v = par[v]
        P.append(v)
        assert len(P) <= V
    P.reverse()
    if len(P) < 3:
        return 0, 0, 0, 0
    wit = witnesses(V, er, P, ds, dt, random.Random(it), layered)
    n = check_witnesses(V, er, P, ds, wit)  # properties 1-3 on G'[R] ...
    W = {(a, b): w for a, b, w in gp}  # (every edge of a witness is an edge of G': a refused one is not in gp)
    for j in range(1, len(P) - 1):
        d = brute(V, gp, s, t, P[j])  # ... and its weight against brute force over G' itself: the restriction to R loses nothing
        assert (d is None) == (j not in wit), (gp, P, j)
        if d is not None:
            R = wit[j][0]
            assert all(in_R[x] for x in R) and sum(W[(a, b)] for a, b in zip(R, R[1:])) == d, (gp, P, j, R, d)
    if not layered:
        assert witnesses(V, er, P, ds, dt, random.Random(it + 99999)) == wit  # another out-edge order: the same bytes
    return n, sum(w[4] > 0 for w in wit.values()), sum(w[4] > 1 for w in wit.values()), sum(w[1] for w in wit.values())


@pytest.mark.parametrize("seed, layered, draws", ((3001, False, 1500), (3002, True, 600)))
def test_witnesses_on_a_policy_equal_brute_force(seed, layered, draws):
    rng = random.Random(seed)
    drawn = gone = slots = cross = long_chains = cuts = 0
    for it in range(draws):
        drawn += 1
        r = check_policy_witnesses(rng, rng.randint(5, 10), layered, it)
        if r is None:
            gone += 1
            continue
        slots += r[0]
        cross += r[1]
        long_chains += r[2]
        cuts += r[3]
    if cuts == 0:  # the random family gave no loop to cut: the family built for it (no policy: G' = G)
        lrng = random.Random(seed)
        for it in range(100):
            V, edges = loop_graph(lrng)
            ds = bellman_ford(V, edges, V - 2)
            dt = bellman_ford(V, edges, V - 1, reverse=True)
            P = shortest_path(V, edges, ds, V - 2, V - 1)
            if P is None:
                continue
            wit = witnesses(V, edges, P, ds, dt, random.Random(it), layered)
            check_witnesses(V, edges, P, ds, wit)
            cuts += sum(w[1] for w in wit.values())
    print("seed %d: %d drawn, %d discarded, %d witnesses, %d cross winners, %d with a delta chain longer than one node, %d loops cut" % (seed, drawn, gone, slots, cross, long_chains, cuts))
    assert 10 * gone <= drawn, (gone, drawn)  # only the graphs whose forward solve reports a negative cycle, at most 10 %
    assert 2 * slots > drawn - gone and cross > 10, (slots, cross)  # (coverage of the generator: a witness per two graphs, some by step 4)
    assert long_chains > 0 and cuts > 0, (long_chains, cuts)
