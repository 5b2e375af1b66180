"""Host side of the pinned drop margins (no GPU): the new entry points in the header, the export list and the Python binding;
the refusals of --pin-drop-margins, their place in the order and the file's layout; and §12's algorithm — the restatement of
tests/test_drop_host.py on the policy graphs of tests/test_redrops_host.py, both imported, not copied — with required edges weighted
W - M, against brute force over the simple source -> target paths of G' - p_j, decoded as the device decodes it."""
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from test_drop_host import bellman_ford, drop_margins  # noqa: E402
from test_pinmargins_host import decode_limbs  # noqa: E402
from test_redrops_host import brute, forward, policy_graph, refusal  # noqa: E402

NEW = ("phx_pindrops_flat", "phx_pindrops_ms", "phx_pindrop_stats")


# ---- 1. declarations ----
def test_pindrop_entry_points_are_declared_exported_and_bound():
    from phanotate_amd import _lib, api

    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int phx_pindrops_flat\(phx_ctx \*ctx, phx_gene_drop \*rec, int32_t \*lost, int64_t cap, int64_t \*offsets\s*, int32_t \*status\s*, int64_t \*total\);", code)
    assert re.search(r"int phx_pindrops_ms\(phx_ctx \*ctx, float \*ms\s*\);", code)
    assert re.search(r"int phx_pindrop_stats\(phx_ctx \*ctx, int64_t \*out\s*\);", code)
    assert "#define PHX_VERSION 410" in text and "phx_pindrops_flat, phx_pindrops_ms, phx_pindrop_stats — probe for the symbol" in text
    assert set(NEW) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert L.phx_version() == 410
    assert L.phx_pindrops_flat.argtypes == L.phx_pinmargins_flat.argtypes and len(L.phx_pindrops_flat.argtypes) == 7
    assert L.phx_pindrops_ms.argtypes == L.phx_redrops_ms.argtypes and L.phx_pindrop_stats.argtypes == L.phx_redrop_stats.argtypes
    assert L.phx_pindrops_flat(None, None, None, 0, None, None, None) == -1  # PHX_E_ARG: no context
    assert L.phx_pindrops_ms(None, None) == -1 and L.phx_pindrop_stats(None, None) == -1
    for name in ("pindrops", "pindrops_ms", "pindrop_stats"):
        assert callable(getattr(api.Annotator, name)), name
    assert api._MS_KEYS["phx_pindrops_ms"] == api._MS_KEYS["phx_drop_ms"]


# ---- 2. the command line ----
CASES = (
    ("--pin-drop-margins F --forbid F --reannotation O", 1, "argument --pin-drop-margins: needs --require"),
    ("--pin-drop-margins F --require F", 1, "argument --pin-drop-margins: needs --reannotation"),
    ("--pin-drop-margins F", 1, "argument --pin-drop-margins: needs --require"),  # (its own rules in _RULES' order)
    ("--pin-drop-margins F --require F --reannotation O -d", 1, "argument --pin-drop-margins: not allowed with argument -d/--dump"),
    ("--pin-drop-margins F --require F --reannotation O --gpus 2", 1, "argument --pin-drop-margins: not available with --gpus above 1"),
    ("--pin-drop-margins F --require F --reannotation O", 2, "argument --pin-drop-margins: not available under a multi-rank launch"),
    ("--pin-drop-margins F --require F --reannotation O", 1, "ok"),
    ("--pin-drop-margins F --pin-margins F --require F --forbid F --reannotation O", 1, "ok"),
    # the first message is the one _CHECK_ORDER dictates: the other side outputs in front, pin-margins among them, the entry files behind
    ("--pin-drop-margins F --pin-margins F", 1, "argument --pin-margins: needs --require"),
    ("--pin-drop-margins F --pin-margins F --require F", 1, "argument --pin-margins: needs --reannotation"),
    ("--pin-drop-margins F --redrop-margins F --require F --reannotation O", 1, "argument --redrop-margins: not allowed with argument --require"),
    ("--pin-drop-margins F --evidence F --reannotation O", 1, "argument --pin-drop-margins: needs --require"),
    ("--pin-drop-margins F --require F --evidence F --reannotation O", 1, "argument --evidence: not allowed with argument --require"),  # stays refused
    ("--pin-drop-margins F --drop-margins F -d", 1, "argument --drop-margins: not allowed with argument -d/--dump"),
)


@pytest.mark.parametrize("argv, world, want", CASES)
def test_pin_drop_margins_refusals_and_their_order(argv, world, want, tmp_path, monkeypatch, capsys):
    got = refusal(argv, world, tmp_path, monkeypatch)
    err = capsys.readouterr().err
    if want == "ok":
        assert got == "ok", err
    else:
        assert got == "refused" and err.rstrip().endswith("error: " + want), err


def test_pin_drop_margins_has_its_place_in_the_table():
    from phanotate_amd import cli

    row = cli.OUTPUTS["pin_drop_margins"]
    assert row.flag == "--pin-drop-margins" and row.fmt is cli.format_pin_drops and row.mode == "wb" and row.resident and row.piped is None
    for order in (cli._CHECK_ORDER, cli._FETCH_ORDER):
        assert order.index("pin_drop_margins") == order.index("pin_margins") + 1
    rules = [m for about, _, m in cli._RULES if about == "pin_drop_margins"]
    assert rules == [m.replace("--pin-margins", "--pin-drop-margins") for about, _, m in cli._RULES if about == "pin_margins"] and len(rules) == 2


def test_format_pin_drops_is_the_drop_block_with_a_lost_column():
    from phanotate_amd import _lib, cli

    rec = np.zeros(4, _lib.DROP_DT)
    rows = ((10, 99, 1, 1, -3.5, 0.25, 1, 1), (150, 320, -1, -2, -7.0, -1.5, 1, 1), (400, 520, 1, 3, -0.125, np.inf, 1, 0), (7, 66, -1, -1, -2.0, 0.0, 0, 1))
    for r, (left, right, strand, frame, score, drop, called, bypass) in zip(rec, rows):
        r["left"], r["right"], r["strand"], r["frame"], r["score"], r["drop"], r["called"], r["bypass"] = left, right, strand, frame, score, drop, called, bypass
    lost = np.array([0, 2, 0, 1], np.int32)
    status, offsets = np.array([0, -2, 0], np.int32), np.array([0, 3, 3, 4], np.int64)
    text = cli.format_pin_drops(["a", "bad", "c"], status, offsets, rec, lost).decode()
    head = "#START\tSTOP\tFRAME\tCONTIG\tSCORE\tDROP\tLOST\tCALLED\n"
    assert text == ("#id:\ta\n" + head + "10\t99\t+\ta\t-3.500000E+00\t2.500000E-01\t0\t1\n" + "320\t150\t-\ta\t-7.000000E+00\t-1.500000E+00\t2\t1\n"
                    + "400\t520\t+\ta\t-1.250000E-01\tINF\t0\t1\n" + "#id:\tc\n" + head + "66\t7\t-\tc\t-2.000000E+00\t0.000000E+00\t1\t0\n")
    # without the LOST column a contig's block is --drop-margins' own (libphx's phx_format_drops), path order kept
    plain = cli.format_drops(["a", "bad", "c"], status, offsets, rec).decode().splitlines()
    mine = text.splitlines()
    assert len(plain) == len(mine)
    for p, m in zip(plain, mine):
        cols = m.split("\t")
        assert p == (m if m.startswith("#id:") else "\t".join(cols[:6] + cols[7:])), (p, m)


# ---- 3. the algorithm under pins ----
def nearest_multiple(x, M):
    """(lost, s) of x = lost * M + s with |s| < M / 2."""
    lost = (x + M // 2) // M
    return lost, x - lost * M


def check_pinned_graph(rng, V, layered, big):
    """None: discarded (the forward solve does not settle: a cycle of negative length, or one through a required edge, that the source
    reaches); else (slots checked, slots with cross nodes, layered builds, slots with lost > 0, of those with s < 0).  big: M = 2^200 and
    the device's limb decoding, else M = 1 + 4 sum |W'| and the nearest multiple."""
    gp, trap = policy_graph(rng, V)
    pins = set(rng.sample(range(len(gp)), min(rng.choice([0, 1, 1, 2, 3]), len(gp))))
    M = 1 << 200 if big else 1 + 4 * sum(abs(w) for _, _, w in gp)
    decode = (lambda x: decode_limbs(x, 200)) if big else (lambda x: nearest_multiple(x, M))
    gw = [(u, v, w - (M if k in pins else 0)) for k, (u, v, w) in enumerate(gp)]
    s, t = V - 2, V - 1
    ds, par = forward(V, gw, s)
    if ds is None:
        return None
    if ds[t] is None:  # PHX_S_NOPATH: no called gene, no records
        return 0, 0, 0, 0, 0
    in_R = [x is not None for x in ds]
    er = [e for e in gw if in_R[e[0]]]  # R_n is closed under G''s out-edges
    assert all(in_R[v] for _, v, _ in er)
    dt = bellman_ford(V, er, t, reverse=True)  # settles: §24's "walks and paths"
    P, v = [t], t
    while v != s:
        v = par[v]
        P.append(v)
        assert len(P) <= V
    P.reverse()
    assert len(P) >= 3 and ds[t] == dt[s] and all(ds[v] + dt[v] == ds[t] for v in P)  # P' is tight under both vectors, required edges included
    best, n_cross, lay = drop_margins(V, er, P, ds, dt, rng, layered)
    gave_up = cheaper = 0
    for j in range(1, len(P) - 1):
        d = brute(V, gw, s, t, P[j])  # over G' itself: the restriction to R_n loses nothing
        want = None if d is None else d - ds[t]
        assert best[j] == want, (gp, pins, P, j, best[j], want)
        if want is None:
            continue
        lost, low = decode(want)
        assert (lost, low) >= (0, 0) and lost * M + low == want and (lost, low) == nearest_multiple(want, M), (gp, pins, P, j, lost, low)
        gave_up += lost > 0
        cheaper += lost > 0 and low < 0
    return len(P) - 2, n_cross, int(lay), gave_up, cheaper


@pytest.mark.parametrize("big", (False, True))
@pytest.mark.parametrize("seed, layered, draws, floor", ((3201, False, 1500, 1000), (3202, True, 600, 500)))
def test_restatement_under_pins_equals_brute_force(seed, layered, draws, floor, big):
    """Measured with either M (the counts do not depend on it: the order of the paths is the lexicographic one for every M above
    sum |W'|): seed 3201: 302 of 1500 discarded, 1967 slots, 210 with cross nodes, 350 with lost > 0, 187 of them with s < 0; seed 3202: 111
    of 600 discarded, 774 slots, 89 with cross nodes, 137 and 100."""
    rng = random.Random(seed)
    drawn = gone = slots = cross = lay = gave_up = cheaper = 0
    for _ in range(draws):
        drawn += 1
        r = check_pinned_graph(rng, rng.randint(5, 10), layered, big)
        if r is None:
            gone += 1
            continue
        slots += r[0]
        cross += r[1]
        lay += r[2]
        gave_up += r[3]
        cheaper += r[4]
    print("seed %d, M = %s: %d drawn, %d discarded, %d slots, %d with cross nodes, %d layered, %d with lost > 0, %d of them with s < 0"
          % (seed, "2^200" if big else "1 + 4 sum|W'|", drawn, gone, slots, cross, lay, gave_up, cheaper))
    assert 4 * gone <= drawn, (gone, drawn)  # only the graphs whose forward solve does not settle, at most 25 %
    assert slots > floor and cross > 10 and lay > 0 and gave_up >= 100 and cheaper >= 50, (slots, cross, lay, gave_up, cheaper)
