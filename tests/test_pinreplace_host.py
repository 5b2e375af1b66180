"""Host side of the pinned replacements (no GPU): the four new entry points in the header, the export list and the Python
binding; the row of --pin-drop-replacements, its refusals, their place in the order and the file's layout; and §13's witness construction
— the restatement of tests/test_replace_host.py on the policy graphs of tests/test_redrops_host.py, both imported, not copied — with
required edges weighted W - M as tests/test_pindrops_host.py draws them, against brute force over the simple source -> target paths of
G' - p_j: the weight, and the required edges a witness carries."""
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_drop_host import bellman_ford, shortest_path  # noqa: E402
from test_pindrops_host import nearest_multiple  # noqa: E402
from test_pinmargins_host import decode_limbs  # noqa: E402
from test_redrops_host import brute, forward, policy_graph, refusal  # noqa: E402
from test_replace_host import check_witnesses, loop_graph, witnesses  # noqa: E402

NEW = ("phx_pinreplacements_flat", "phx_tap_pinreplacement", "phx_pinreplacements_ms", "phx_pinreplacement_stats")
SIBLING = dict(zip(NEW[1:], ("phx_tap_rereplacement", "phx_rereplacements_ms", "phx_rereplacement_stats")))


# ---- 1. declarations ----
def test_pinreplacement_entry_points_are_declared_exported_and_bound():
    import ctypes as C

    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int phx_pinreplacements_flat\(phx_ctx \*ctx, phx_gene_repl \*rec, int32_t \*lost, int64_t cap, phx_gene \*genes, int64_t gene_cap, int64_t \*offsets\s*,\s*"
                     r"int32_t \*status\s*, int64_t \*total, int64_t \*gene_total\);", code)
    assert re.search(r"int phx_tap_pinreplacement\(phx_ctx \*ctx, int32_t contig, int32_t k, int32_t \*path, int32_t cap, int32_t \*n_path\);", code)
    assert re.search(r"int phx_pinreplacements_ms\(phx_ctx \*ctx, float \*ms\s*\);", code)
    assert re.search(r"int phx_pinreplacement_stats\(phx_ctx \*ctx, int64_t \*out\s*\);", code)
    assert "#define PHX_VERSION 410" in text
    assert "(additions, version unchanged) phx_pinreplacements_flat, phx_tap_pinreplacement, phx_pinreplacements_ms, phx_pinreplacement_stats — probe for the symbol" in text
    assert set(NEW) <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert L.phx_version() == 410
    for name in NEW:
        assert hasattr(L, name), name
    for name, sib in SIBLING.items():
        assert getattr(L, name).argtypes == getattr(L, sib).argtypes and getattr(L, name).restype == getattr(L, sib).restype, name
    # phx_rereplacements_flat's arguments with `lost` behind `rec`, as phx_pindrops_flat has it behind its records
    ra, pa = L.phx_rereplacements_flat.argtypes, L.phx_pinreplacements_flat.argtypes
    assert len(pa) == 10 and list(pa) == list(ra[:2]) + [L.phx_pindrops_flat.argtypes[2]] + list(ra[2:])
    n = C.c_int32(7)
    ms, out = (C.c_float * 3)(), (C.c_int64 * 5)()
    assert L.phx_pinreplacements_flat(None, None, None, 0, None, 0, None, None, None, None) == -1  # PHX_E_ARG: no context
    assert L.phx_tap_pinreplacement(None, 0, 0, None, 0, C.byref(n)) == -1
    assert L.phx_pinreplacements_ms(None, ms) == -1 and L.phx_pinreplacement_stats(None, out) == -1
    for name in ("pinreplacements", "pinreplacement_path", "pinreplacements_ms", "pinreplacement_stats"):
        assert callable(getattr(api.Annotator, name)), name
    assert api._MS_KEYS["phx_pinreplacements_ms"] == api._MS_KEYS["phx_rereplacements_ms"] == api._MS_KEYS["phx_replacements_ms"]


# ---- 2. the command line ----
CASES = (
    ("--pin-drop-replacements F --forbid F --reannotation O", 1, "argument --pin-drop-replacements: needs --require"),
    ("--pin-drop-replacements F --require F", 1, "argument --pin-drop-replacements: needs --reannotation"),
    ("--pin-drop-replacements F", 1, "argument --pin-drop-replacements: needs --require"),  # (its own rules in _RULES' order)
    ("--pin-drop-replacements F --require F --reannotation O -d", 1, "argument --pin-drop-replacements: not allowed with argument -d/--dump"),
    ("--pin-drop-replacements F --require F --reannotation O --gpus 2", 1, "argument --pin-drop-replacements: not available with --gpus above 1"),
    ("--pin-drop-replacements F --require F --reannotation O", 2, "argument --pin-drop-replacements: not available under a multi-rank launch"),
    ("--pin-drop-replacements F --require F --reannotation O", 1, "ok"),
    ("--pin-drop-replacements F --pin-drop-margins F --pin-margins F --require F --forbid F --reannotation O", 1, "ok"),
    # the first message is the one _CHECK_ORDER dictates: the other side outputs in front, pin-drop-margins among them, the entry files behind
    ("--pin-drop-replacements F --pin-drop-margins F", 1, "argument --pin-drop-margins: needs --require"),
    ("--pin-drop-replacements F --pin-drop-margins F --require F", 1, "argument --pin-drop-margins: needs --reannotation"),
    ("--pin-drop-replacements F --pin-margins F --require F", 1, "argument --pin-margins: needs --reannotation"),
    ("--pin-drop-replacements F --redrop-replacements F --require F --reannotation O", 1, "argument --redrop-replacements: not allowed with argument --require"),
    ("--pin-drop-replacements F --evidence F --reannotation O", 1, "argument --pin-drop-replacements: needs --require"),
    ("--pin-drop-replacements F --require F --evidence F --reannotation O", 1, "argument --evidence: not allowed with argument --require"),  # stays refused
    ("--pin-drop-replacements F --drop-replacements F -d", 1, "argument --drop-replacements: not allowed with argument -d/--dump"),
    ("--pin-drop-replacements F --pin-drop-margins F --require F --reannotation O --gpus 2", 1, "argument --pin-drop-margins: not available with --gpus above 1"),
)


@pytest.mark.parametrize("argv, world, want", CASES)
def test_pin_drop_replacements_refusals_and_their_order(argv, world, want, tmp_path, monkeypatch, capsys):
    got = refusal(argv, world, tmp_path, monkeypatch)
    err = capsys.readouterr().err
    if want == "ok":
        assert got == "ok", err
    else:
        assert got == "refused" and err.rstrip().endswith("error: " + want), err


def test_pin_drop_replacements_has_its_place_in_the_table():
    from phanotate_amd import cli

    row = cli.OUTPUTS["pin_drop_replacements"]
    assert row.flag == "--pin-drop-replacements" and row.fmt is cli.format_pin_replacements and row.mode == "wb" and row.resident and row.piped is None
    assert row.merge is cli.OUTPUTS["drop_replacements"].merge  # (gene_off counts per batch)
    for order in (cli._CHECK_ORDER, cli._FETCH_ORDER):
        assert order.index("pin_drop_replacements") == order.index("pin_drop_margins") + 1 == order.index("pin_margins") + 2
    rules = [m for about, _, m in cli._RULES if about == "pin_drop_replacements"]
    assert len(rules) == 2 and rules == [m.replace("--pin-drop-margins", "--pin-drop-replacements") for about, _, m in cli._RULES if about == "pin_drop_margins"]


def test_merge_of_batches_keeps_lost_beside_the_records():
    from phanotate_amd import _lib, cli

    def part(n, ng, lost0):
        rec = np.zeros(n, _lib.REPL_DT)
        rec["gene_off"] = np.arange(n)
        return np.zeros(1, np.int32), np.array([0, n], np.int64), rec, np.zeros(ng, _lib.GENE_DT), np.arange(lost0, lost0 + n, dtype=np.int32)

    status, offsets, rec, genes, lost = cli.OUTPUTS["pin_drop_replacements"].merge([part(2, 3, 0), part(3, 4, 10)])
    assert list(offsets) == [0, 2, 5] and list(rec["gene_off"]) == [0, 1, 3, 4, 5] and len(genes) == 7 and list(lost) == [0, 1, 10, 11, 12] and len(status) == 2


def test_format_pin_replacements_is_the_replacement_block_with_a_lost_column():
    from phanotate_amd import _lib, cli

    rec = np.zeros(4, _lib.REPL_DT)
    rows = ((10, 99, 1, 1, 0.25, 1, 1, 0, 1, 2), (150, 320, -1, -2, -1.5, 1, 1, 3, 2, 0), (400, 520, 1, 3, np.inf, 1, 0, 5, 0, 0), (7, 66, -1, -1, 0.0, 0, 1, 5, 1, 1))
    for r, (left, right, strand, frame, drop, called, bypass, goff, nrem, nadd) in zip(rec, rows):
        r["left"], r["right"], r["strand"], r["frame"], r["drop"], r["called"], r["bypass"] = left, right, strand, frame, drop, called, bypass
        r["gene_off"], r["n_removed"], r["n_added"], r["span_left"], r["span_right"] = goff, nrem, nadd, left, right
    genes = np.zeros(7, _lib.GENE_DT)
    for g, (left, right, strand, frame) in zip(genes, ((10, 99, 1, 1), (5, 40, 1, 2), (60, 98, -1, -3), (150, 320, -1, -2), (330, 400, 1, 4), (7, 66, -1, -1), (3, 70, -1, -4))):
        g["left"], g["right"], g["strand"], g["frame"] = left, right, strand, frame
    lost = np.array([0, 2, 0, 1], np.int32)
    status, offsets = np.array([0, -2, 0], np.int32), np.array([0, 3, 3, 4], np.int64)
    text = cli.format_pin_replacements(["a", "bad", "c"], status, offsets, rec, genes, lost).decode()
    head = "#START\tSTOP\tFRAME\tCONTIG\tDROP\tLOST\tREMOVED\tADDED\n"
    assert text == ("#id:\ta\n" + head + "10\t99\t+\ta\t2.500000E-01\t0\t10..99\t5..40,98..60\n" + "320\t150\t-\ta\t-1.500000E+00\t2\t320..150,tRNA:330..400\t-\n"
                    + "400\t520\t+\ta\tINF\t0\t-\t-\n" + "#id:\tc\n" + head + "66\t7\t-\tc\t0.000000E+00\t1\t66..7\ttRNA:70..3\n")
    # without the LOST column a contig's block is --drop-replacements' own (libphx's phx_format_replacements), path order kept
    plain = cli.format_replacements(["a", "bad", "c"], status, offsets, rec, genes).decode().splitlines()
    mine = text.splitlines()
    assert len(plain) == len(mine)
    for p, m in zip(plain, mine):
        cols = m.split("\t")
        assert p == (m if m.startswith("#id:") else "\t".join(cols[:5] + cols[6:])), (p, m)


# ---- 3. the construction under pins ----
def pinned(gp, pins, big):
    """(M, the decoder of lost * M + s, G' with the edges of `pins` weighted W - M)."""
    M = 1 << 200 if big else 1 + 4 * sum(abs(w) for _, _, w in gp)
    decode = (lambda x: decode_limbs(x, 200)) if big else (lambda x: nearest_multiple(x, M))
    return M, decode, [(u, v, w - (M if k in pins else 0)) for k, (u, v, w) in enumerate(gp)]


def check_against_brute(V, gw, er, P, ds, wit, req, decode):
    """Every slot of P: a witness iff brute force over G' - p_j finds a path, of that weight, carrying c(P') - lost required edges.
    Returns (slots with lost > 0, of those with s < 0)."""
    s, t = V - 2, V - 1
    W = {(a, b): w for a, b, w in gw}  # (every edge of a witness is an edge of G': a refused one is not in gw)
    on = lambda R: sum((a, b) in req for a, b in zip(R, R[1:]))
    gave_up = cheaper = 0
    for j in range(1, len(P) - 1):
        d = brute(V, gw, s, t, P[j])  # over G' itself: the restriction to R_n loses nothing
        assert (d is None) == (j not in wit), (gw, P, j)
        if d is None:
            continue
        R = wit[j][0]
        assert sum(W[(a, b)] for a, b in zip(R, R[1:])) == d, (gw, P, j, R, d)
        lost, low = decode(d - ds[t])
        assert (lost, low) >= (0, 0) and on(R) == on(P) - lost, (gw, P, j, R, lost, low)
        gave_up += lost > 0
        cheaper += lost > 0 and low < 0
    return gave_up, cheaper


def check_pinned_witnesses(rng, V, layered, big, it):
    """None: discarded (the forward solve does not settle: a cycle of negative length, or one through a required edge, that the source
    reaches); else (slots with a witness, cross winners, delta chains longer than one node, loops cut, lost > 0, of those s < 0).  The
    pins are drawn as tests/test_pindrops_host.check_pinned_graph draws them."""
    gp, _ = policy_graph(rng, V)
    pins = set(rng.sample(range(len(gp)), min(rng.choice([0, 1, 1, 2, 3]), len(gp))))
    M, decode, gw = pinned(gp, pins, big)
    req = {(gp[k][0], gp[k][1]) for k in pins}
    s, t = V - 2, V - 1
    ds, par = forward(V, gw, s)
    if ds is None:
        return None
    if ds[t] is None:  # PHX_S_NOPATH: no called gene, no records
        return 0, 0, 0, 0, 0, 0
    in_R = [x is not None for x in ds]
    er = [e for e in gw if in_R[e[0]]]  # G'[R_n]: R_n is closed under G''s out-edges
    dt = bellman_ford(V, er, t, reverse=True)  # settles: §24's "walks and paths"
    P, v = [t], t
    while v != s:
        v = par[v]
        P.append(v)
        assert len(P) <= V
    P.reverse()
    if len(P) < 3:
        return 0, 0, 0, 0, 0, 0
    wit = witnesses(V, er, P, ds, dt, random.Random(it), layered)
    n = check_witnesses(V, er, P, ds, wit)  # properties 1-3 on G'[R_n] under W' ...
    assert all(in_R[x] for w in wit.values() for x in w[0])
    gave_up, cheaper = check_against_brute(V, gw, er, P, ds, wit, req, decode)  # ... the weight over G' itself, and the pins carried
    if not layered:
        assert witnesses(V, er, P, ds, dt, random.Random(it + 99999)) == wit  # another out-edge order: the same bytes
    return n, sum(w[4] > 0 for w in wit.values()), sum(w[4] > 1 for w in wit.values()), sum(w[1] for w in wit.values()), gave_up, cheaper


def pinned_loops(seed, layered, big):
    """tests/test_replace_host.loop_graph's graphs with one edge of their shortest path weighted W - M: (witnesses, loops cut, lost > 0)."""
    lrng = random.Random(seed)
    n = cuts = gave_up = 0
    for it in range(100):
        V, edges = loop_graph(lrng)
        s, t = V - 2, V - 1
        P0 = shortest_path(V, edges, bellman_ford(V, edges, s), s, t)
        if P0 is None:
            continue
        k = lrng.randrange(len(P0) - 1)
        pins = {i for i, (a, b, _) in enumerate(edges) if (a, b) == (P0[k], P0[k + 1])}
        M, decode, gw = pinned(edges, pins, big)
        ds = bellman_ford(V, gw, s)
        dt = bellman_ford(V, gw, t, reverse=True)
        P = shortest_path(V, gw, ds, s, t)
        assert P == P0  # (the pin only favours the path it lies on)
        wit = witnesses(V, gw, P, ds, dt, random.Random(it), layered)
        n += check_witnesses(V, gw, P, ds, wit)
        g, _ = check_against_brute(V, gw, gw, P, ds, wit, {(P0[k], P0[k + 1])}, decode)
        gave_up += g
        cuts += sum(w[1] for w in wit.values())
    return n, cuts, gave_up


@pytest.mark.parametrize("big", (False, True))
@pytest.mark.parametrize("seed, layered, draws, floor", ((3301, False, 1500, 100), (3302, True, 600, 50)))
def test_witnesses_under_pins_equal_brute_force(seed, layered, draws, floor, big):
    """Measured with either M (the counts do not depend on it): seed 3301 (doubling): 336 of 1500 discarded, 794 witnesses, 33 cross
    winners, 7 with a delta chain longer than one node, 372 with lost > 0, 211 of them with s < 0; seed 3302 (layered): 126 of 600
    discarded, 362 witnesses, 17 cross winners, 4 long chains, 161 and 77.  The random family cuts no loop; loop_graph's graphs with a
    required edge on their shortest path: 100 witnesses, 100 loops cut in either build, 51 with lost > 0."""
    rng = random.Random(seed)
    drawn = gone = slots = cross = long_chains = cuts = gave_up = cheaper = 0
    for it in range(draws):
        drawn += 1
        r = check_pinned_witnesses(rng, rng.randint(5, 10), layered, big, it)
        if r is None:
            gone += 1
            continue
        slots, cross, long_chains, cuts, gave_up, cheaper = (a + b for a, b in zip((slots, cross, long_chains, cuts, gave_up, cheaper), r))
    ln, lcuts, lgave = pinned_loops(seed, layered, big)
    print("seed %d, M = %s: %d drawn, %d discarded, %d witnesses, %d cross winners, %d with a delta chain longer than one node, %d loops cut, %d with lost > 0, "
          "%d of them with s < 0; loop graphs: %d witnesses, %d loops cut, %d with lost > 0"
          % (seed, "2^200" if big else "1 + 4 sum|W'|", drawn, gone, slots, cross, long_chains, cuts, gave_up, cheaper, ln, lcuts, lgave))
    assert 4 * gone <= drawn, (gone, drawn)  # only the graphs whose forward solve does not settle, at most 25 %
    assert 4 * slots > drawn - gone and cross > 10 and long_chains > 0, (slots, cross, long_chains)  # (coverage of the generator)
    assert gave_up >= floor and cheaper > 0, (gave_up, cheaper)
    assert lcuts > 0 and lgave > 0 and ln >= lcuts, (ln, lcuts, lgave)  # a loop is cut under a pin, and some of those witnesses give the pin up
