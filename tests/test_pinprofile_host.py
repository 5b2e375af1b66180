"""Pinned profiles, the parts that need no GPU: the header, the export list and the entry points without a context;
format_profile with and without `lost`.  Then the algorithm and the definition in Python alone — these tests load no library code and check
the method, not k_pf_cand, which tests/test_pinprofile_gpu.py compares bit for bit on the device: the level rounds (round 0 with patterns
and markers, one round per level with a signed-double key) against brute-force lexicographic minima, with the order of the marker keys
and of the signed-double transform; the definition Delta'' = lost * M + s on every edge, connectors included, of the CPU oracle's graphs under the
45 seeded mixes of tests/test_pinmargins_host.py and one draw of this file's own; and a hand-made graph whose three tracks differ in
`lost` on one slot."""
import os
import random
import re
import struct

import numpy as np

from test_evidence_gpu import settle
from test_pinmargins_host import reverse_in_R, split
from test_profile_host import NONE, SIZES

from phanotate_amd import _lib, api, cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
PNONE = (1 << 64) - 1  # PF_PNONE
TRACKS = ("fwd", "rev", "gap")


# ---- the interface ----
def test_header_exports_methods_and_no_cli_row():
    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "int phx_pinprofile_flat(phx_ctx *ctx, phx_profile_slot *rec, int32_t *lost , int64_t cap, int64_t *offsets , int32_t *status , int64_t *total);" in flat
    assert "int phx_pinprofile_ms(phx_ctx *ctx, float *ms );" in flat
    assert "int phx_pinprofile_stats(phx_ctx *ctx, int64_t *out );" in flat
    # the existing calls and the record are as they were: the new call reuses phx_profile_slot
    assert "int phx_reprofile_flat(phx_ctx *ctx, phx_profile_slot *rec, int64_t cap, int64_t *offsets , int32_t *status , int64_t *total);" in flat
    assert "int phx_profile_flat(phx_ctx *ctx, phx_profile_slot *rec, int64_t cap, int64_t *offsets , int32_t *status , int64_t *total);" in flat
    assert len(re.findall(r"typedef struct phx_profile_slot \{", flat)) == 1
    assert re.search(r"#define PHX_VERSION 410\b", text)  # callers probe for the symbol
    for name in ("phx_pinprofile_flat", "phx_pinprofile_ms", "phx_pinprofile_stats"):
        assert _lib.EXPORTS.count(name) == 1
    assert _lib.PROFILE_DT.itemsize == 32  # pinprofile() hands out PROFILE_DT records
    L = _lib.lib()
    assert len(L.phx_pinprofile_flat.argtypes) == 7 and L.phx_pinprofile_ms.argtypes == L.phx_profile_ms.argtypes and len(L.phx_pinprofile_stats.argtypes) == 2
    assert L.phx_pinprofile_flat(None, None, None, 0, None, None, None) == -1  # PHX_E_ARG without a context
    assert L.phx_pinprofile_ms(None, None) == -1 and L.phx_pinprofile_stats(None, None) == -1
    assert callable(api.Annotator.pinprofile) and callable(api.Annotator.pinprofile_ms) and callable(api.Annotator.pinprofile_stats)
    assert api._MS_KEYS["phx_pinprofile_ms"] == api._MS_KEYS["phx_profile_ms"] == ("tables", "records", "download")
    for order in (cli._CHECK_ORDER, cli._FETCH_ORDER):  # library and Python only: no command-line row
        assert not [x for x in order if "pinprofile" in x or "pin_profile" in x]
    assert not [k for k in cli.OUTPUTS if "pinprofile" in k or "pin_profile" in k]


def test_format_profile_with_and_without_lost():
    rec = np.array([
        (0, 10, INF, 2.5, 0.0),       # contig a
        (10, 10, 1.0, 2.0, 3.0),      #   an empty slot: left out
        (10, 25, INF, 2.5, 0.0),      #   the same values as the first, another count: a row of its own with `lost`, merged without
        (25, 40, 0.0, -2.5, 1.0),     #   a negative value beside lost > 0
        (40, 90, 0.0, -2.5, 1.0),     #   merges either way
        (0, 7, INF, INF, INF),        # contig c: no path
    ], _lib.PROFILE_DT)
    lost = np.array([[0, 1, 0], [9, 9, 9], [0, 2, 0], [0, 1, 2], [0, 1, 2], [0, 0, 0]], np.int32)
    status = np.array([0, -9, 1], np.int32)
    offsets = np.array([0, 5, 5, 6], np.int64)
    names = ["a", "neg", "c"]
    plain = cli.format_profile(names, status, offsets, rec)
    assert plain == (b"#id:\ta\n#LO\tHI\tFWD\tREV\tGAP\n"
                     b"0\t25\tINF\t2.500000E+00\t0.000000E+00\n"
                     b"25\t90\t0.000000E+00\t-2.500000E+00\t1.000000E+00\n"
                     b"#id:\tc\n#LO\tHI\tFWD\tREV\tGAP\n"
                     b"0\t7\tINF\tINF\tINF\n")
    assert cli.format_profile(names, status, offsets, rec, None) == plain == cli.format_profile(names, status, offsets, rec, lost=None)
    for lo in (lost, lost.reshape(-1)):  # (total, 3) as pinprofile() returns it, or flat as the library fills it
        assert cli.format_profile(names, status, offsets, rec, lo) == (b"#id:\ta\n#LO\tHI\tFWD\tLOST\tREV\tLOST\tGAP\tLOST\n"
                                                                         b"0\t10\tINF\t0\t2.500000E+00\t1\t0.000000E+00\t0\n"
                                                                         b"10\t25\tINF\t0\t2.500000E+00\t2\t0.000000E+00\t0\n"
                                                                         b"25\t90\t0.000000E+00\t0\t-2.500000E+00\t1\t1.000000E+00\t2\n"
                                                                         b"#id:\tc\n#LO\tHI\tFWD\tLOST\tREV\tLOST\tGAP\tLOST\n"
                                                                         b"0\t7\tINF\t0\tINF\t0\tINF\t0\n")
    assert cli.format_profile([], np.zeros(0, np.int32), np.zeros(1, np.int64), rec[:0], np.zeros((0, 3), np.int32)) == b""


# ---- the level rounds (phx_profile.inc under MgPinProf), restated ----
def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def dbl(k):
    return struct.unpack("<d", struct.pack("<Q", k))[0]


def mu_of(s):
    """float(s) / 1000.0 as k_margins rounds it; beyond the double range: +-inf"""
    try:
        return float(s) / 1000.0
    except OverflowError:
        return INF if s > 0 else -INF


def marker(lost):
    return NONE + lost  # above every pattern of a non-negative double, +inf (NONE) included


def skey(x):
    """pf_skey: the pattern of a signed double as an unsigned key of the same order"""
    p = bits(x)
    return (~p) & PNONE if p >> 63 else p | (1 << 63)


def sval(k):
    """pf_sval: back"""
    return dbl(k ^ (1 << 63) if k >> 63 else (~k) & PNONE)


def pn_sparse_min(n, iv):
    """k_pf_cand's table with PNONE for "none" (sparse_min's code, the one constant changed)"""
    lv = 1
    while (2 << (lv - 1)) <= n:
        lv += 1
    tab = [PNONE] * (n * lv)
    for a, z, key in iv:
        k = (z - a + 1).bit_length() - 1
        assert 0 <= k < lv and 0 <= a and z < n and key < PNONE
        for i in (k * n + a, k * n + z - (1 << k) + 1):
            tab[i] = min(tab[i], key)
    for k in range(lv - 1, 0, -1):
        h = 1 << (k - 1)
        for i in range(n):
            m = tab[k * n + i]
            if i >= h:
                m = min(m, tab[k * n + i - h])
            if m != PNONE:
                tab[(k - 1) * n + i] = min(tab[(k - 1) * n + i], m)
    return tab[:n]


def level_rounds(n, items):
    """One track as the device runs it: items = [(a, z, lost, s)] with lost >= 0 and s >= 0 where lost == 0.  Returns ([(lost, value)] per
    slot — (0, +inf): nothing covers it —, rounds run)."""
    iv = []
    for a, z, lost, s in items:  # round 0: every edge
        assert lost >= 0 and (lost > 0 or s >= 0)
        iv.append((a, z, marker(lost) if lost > 0 else bits(mu_of(s))))
    out = []
    for k in pn_sparse_min(n, iv):
        if k <= NONE:
            out.append((0, dbl(k)))  # a pattern: exact
        elif k == PNONE:
            out.append((0, INF))
        else:
            out.append((k - NONE, INF))  # a marker: L(i), the value comes in its level's round
    rounds, level = 1, 0
    while True:
        pending = [L for L, _ in out if L > level]
        if not pending:
            return out, rounds
        level = min(pending)
        tab = pn_sparse_min(n, [(a, z, skey(mu_of(s))) for a, z, lost, s in items if lost == level])
        for i in range(n):
            if out[i][0] == level:
                assert tab[i] != PNONE  # some covering edge has exactly L(i)
                out[i] = (level, sval(tab[i]))
        rounds += 1


def brute_lex(n, items):
    """per slot the lexicographic minimum of (lost, s) over the covering items, as (lost, mu(s)); (0, +inf): none"""
    best = [None] * n
    for a, z, lost, s in items:
        for x in range(a, z + 1):
            if best[x] is None or (lost, s) < best[x]:
                best[x] = (lost, s)
    return [(0, INF) if b is None else (b[0], mu_of(b[1])) for b in best]


def same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and bits(x[1]) == bits(y[1]) for x, y in zip(a, b))


def draw_s(rng, lost):
    mag = rng.choice((0, 1, 2, 999, 1000, 2500, rng.randrange(1 << 20), rng.randrange(1 << 70)))
    return mag if lost == 0 or rng.random() < 0.5 else -mag  # negative s only beside lost > 0


def test_level_rounds_match_brute_force_lexicographic_minima():
    rng = random.Random(3701)
    seen_levels = set()
    negative = extra = 0
    for trial in range(2400):
        n = SIZES[trial % len(SIZES)]
        kind = (trial // len(SIZES)) % 6
        pair = lambda: (lambda lost: (lost, draw_s(rng, lost)))(rng.choice((0, 0, 1, 1, 2, 3)))
        if kind == 0:  # an empty track
            items = []
        elif kind == 1:  # ranges of length 1 only
            items = [(a, a) + pair() for a in (rng.randrange(n) for _ in range(rng.randrange(1, 2 * n + 1)))]
        elif kind == 2:  # full ranges, and equal keys among them
            items = [(0, n - 1) + rng.choice(((1, -5), (1, -5), (2, 7), (0, 1 << 40), (3, 0))) for _ in range(rng.randrange(1, 4))]
        elif kind == 3:  # no edge without a lost pin: every slot waits for a level round
            items = []
            for _ in range(rng.randrange(1, 3 * n + 2)):
                a = rng.randrange(n)
                lost = rng.randrange(1, 4)
                items.append((a, rng.randrange(a, n), lost, draw_s(rng, lost)))
        else:  # anything; kind 5 draws the pairs from a few values, so that equal keys meet
            items = []
            for _ in range(rng.randrange(1, 3 * n + 2)):
                a = rng.randrange(n)
                items.append((a, rng.randrange(a, n)) + (rng.choice(((0, 0), (0, 17), (1, -17), (1, 17), (2, -1), (3, 5))) if kind == 5 else pair()))
        got, rounds = level_rounds(n, items)
        want = brute_lex(n, items)
        assert same(got, want), (n, kind, items)
        levels = {lost for lost, _ in want if lost > 0}
        assert rounds == 1 + len(levels), (n, kind, rounds, levels)  # one further round per distinct level some slot holds
        seen_levels |= levels
        negative += any(lost > 0 and v < 0 for lost, v in want)
        extra += rounds > 1
    assert seen_levels == {1, 2, 3} and negative >= 200 and extra >= 800, (seen_levels, negative, extra)


def test_marker_keys_and_the_signed_double_key_keep_the_order():
    rng = random.Random(3702)
    special = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, float(1 << 63), -float(1 << 63), float(1 << 64), 1.7976931348623157e308,
               -1.7976931348623157e308, INF, -INF, 1.0, -1.0, 2.5, -2.5]

    def value():
        r = rng.random()
        if r < 0.3:
            return rng.choice(special)
        if r < 0.5:
            return dbl(rng.randrange(1, 1 << 52)) * rng.choice((1, -1))  # a subnormal
        if r < 0.7:
            return float(rng.randrange(1 << 63, 1 << 200)) * rng.choice((1, -1))  # at or above 2^63
        return mu_of(rng.randrange(-(1 << 80), 1 << 80))

    for _ in range(10000):
        x, y = value(), value()
        kx, ky = skey(x), skey(y)
        assert kx < PNONE and ky < PNONE
        assert bits(sval(kx)) == bits(x) and bits(sval(ky)) == bits(y)
        if x < y:
            assert kx < ky
        elif x > y:
            assert kx > ky
        else:  # equal values: equal keys but for the two zeros, -0.0 below +0.0
            assert (kx == ky) == (bits(x) == bits(y)) and (kx < ky) == (bits(x) >> 63 > bits(y) >> 63)
        # round 0: a pattern of a non-negative double (lost = 0) is below every marker, the markers order by lost, "none" is above all
        ax, ay = abs(x), abs(y)
        la, lb = rng.randrange(1, 1 << 31), rng.randrange(1, 1 << 31)
        assert bits(ax) <= NONE < marker(1) <= marker(la) < PNONE and (marker(la) < marker(lb)) == (la < lb)
        assert (bits(ax) < bits(ay)) == (ax < ay) or (ax == ay == 0.0)
    assert skey(-0.0) < skey(0.0) and skey(-INF) == (~bits(-INF)) & PNONE and skey(INF) < PNONE


# ---- the definition on the CPU oracle's graphs ----
def rank(v, V):
    return v if v < V - 2 else (-1 if v == V - 2 else V - 2)


def track_of(g, u):
    """as pf_track: by the tail — a forward start (tRNA start alike): 0, a reverse stop: 1, anything else, the source among it: 2"""
    if u in (g.src, g.tgt):
        return 2
    if g.type[u] == 0 and g.frame[u] > 0:
        return 0
    if g.type[u] == 1 and g.frame[u] < 0:
        return 1
    return 2


class Recording:
    """The oracle, keeping the last run's arrays: OracleGraph does not keep the nodes' positions, which the slots need."""

    def __init__(self, orc):
        self.orc, self.last = orc, None

    def run(self, *args, **kw):
        self.last = self.orc.run(*args, **kw)
        return self.last

    def __getattr__(self, name):
        return getattr(self.orc, name)


def oracle_graphs(oracle, seqs):
    """curate_draws.OracleGraph per contig, with .rank: the oracle numbers its nodes in its own order, the slots are counted in position
    order as on the device (source -1, target V - 2; nodes of one position, whose slot has no extent, in the oracle's order)."""
    import curate_draws as cd

    tap = Recording(oracle)
    out = []
    for s in seqs:
        g = cd.OracleGraph(tap, s)
        if g.ok:
            pos = tap.last["node_pos"].tolist()
            real = sorted((v for v in range(g.V) if v not in (g.src, g.tgt)), key=lambda v: (pos[v], v))
            g.rank = [0] * g.V
            for r, v in enumerate(real):
                g.rank[v] = r
            g.rank[g.src], g.rank[g.tgt] = -1, g.V - 2
        out.append(g)
    return out


def oracle_profile(g, d, M):
    """None (the solve does not settle or finds no path), or per track and slot the lexicographic minimum (lost, s) over the covering
    edges of the draw's graph (None: none) — every edge, connectors included — with Delta'' >= 0 checked on each."""
    import curate_draws as cd

    from test_margins_gpu import sweep_idx

    edges, pinned = cd.weights(g.edges, g.orf_edge, d, M)
    ds, par = settle(g.V, edges, g.src)
    if ds is None or ds[g.tgt] is None:
        return None
    assert (g.src, g.tgt) == (g.V - 2, g.V - 1)
    dt, _ = reverse_in_R(g.V, sorted(edges, key=lambda e: sweep_idx(e[0], g.V)), ds, g.tgt)
    assert dt is not None and dt[g.src] == ds[g.tgt]
    n = g.V - 1
    best = [[None] * n for _ in range(3)]
    for u, v, w in edges:
        if ds[u] is None or dt[v] is None:
            continue
        x = ds[u] + w + dt[v] - ds[g.tgt]
        assert x >= 0, (u, v, x)  # inside R_n, connectors included
        p = split(x, M)
        assert p >= (0, 0)
        row = best[track_of(g, u)]
        for i in range(g.rank[u] + 1, g.rank[v] + 1):
            if row[i] is None or p < row[i]:
                row[i] = p
    return best


def neighbour_pins(g):
    """This file's own draw for a contig: of its called genes in position order, both strands together, the two neighbours with the
    largest overlap — both pinned; nothing refused or biased.  An edge of another track over a slot of the overlap runs into both pins
    unless it is short.  None: no two neighbours overlap.  (The 45 mixes alone have slots whose minimum gives up two pins on the fwd and
    gap tracks; this draw brings them on the rev track as well.)"""
    keys = sorted(k for k in g.called if k in g.orf_edge)
    pairs = [(a[1] - b[0], a, b) for a, b in zip(keys, keys[1:]) if b[0] <= a[1]]
    if not pairs:
        return None
    ov, a, b = max(pairs, key=lambda p: (p[0], -p[1][0]))
    return dict(require=[a, b], bias={}, forbid=[])


def fold(best, hist, flags):
    for t in range(3):
        for p in best[t]:
            if p is not None:
                hist[t][p[0]] = hist[t].get(p[0], 0) + 1
                flags["negative"] += p[0] > 0 and p[1] < 0
                flags["two"] += p[0] >= 2
    for i in range(len(best[0])):  # the re-annotation's path crosses every slot at Delta'' = 0
        assert min(b[i] for b in best if b[i] is not None) == (0, 0), i


def test_the_mixes_on_the_oracles_graphs(oracle):
    import phanotate_amd as pa

    import curate_draws as cd

    graphs = oracle_graphs(oracle, cd.mix_seqs(pa))
    draws = ok = 0
    hist, flags = [{}, {}, {}], dict(negative=0, two=0)
    for row in cd.mixes(graphs):
        for g, d in zip(graphs, row):
            if d is None:
                continue
            draws += 1
            M = 1 << (cd.big_m(g.edges, d).bit_length() + 2)  # a power of two above four times every walk sum, as the device's 2^(64 NL)
            best = oracle_profile(g, d, M)
            if best is None:
                continue
            ok += 1
            fold(best, hist, flags)
    print("the 45 mixes: %d draws, %d settle; slots by their minimum lost, fwd: %s rev: %s gap: %s; %d with a negative value, %d with lost >= 2" % (
        draws, ok, *[sorted(h.items()) for h in hist], flags["negative"], flags["two"]))
    assert draws == 45 and ok == 45, (draws, ok)  # what tests/test_curate_host.py records
    assert all(h.get(1, 0) > 0 for h in hist) and flags["negative"] > 0 and flags["two"] > 0, (hist, flags)  # the 45 alone show all three
    own = own_ok = 0
    for g in graphs:
        d = neighbour_pins(g) if g.ok else None
        if d is None:
            continue
        own += 1
        best = oracle_profile(g, d, 1 << (cd.big_m(g.edges, d).bit_length() + 2))
        if best is not None:
            own_ok += 1
            fold(best, hist, flags)
    print("with this file's draw (%d contigs, %d settle): fwd: %s rev: %s gap: %s; %d with a negative value, %d with lost >= 2" % (
        own, own_ok, *[sorted(h.items()) for h in hist], flags["negative"], flags["two"]))
    assert all(h.get(1, 0) > 0 for h in hist), hist  # lost = 1 on each of the three tracks
    assert flags["negative"] > 0 and flags["two"] > 0, flags
    assert all(max(h) >= 2 for h in hist), hist  # ... and with this file's draw a slot with lost >= 2 on each


# ---- a hand-made graph ----
def test_three_tracks_of_one_slot_differ_in_lost():
    """Real nodes 0 .. 5 in position order, source 6, target 7.  Forward starts 0 and 2 (tails of track 0), a reverse stop 1 (track 1), the
    others close nodes (connectors leave them).  The forward genes 0 -> 3 and 2 -> 5 are pinned and the best path keeps both, through the
    overlap connector 3 -> 2.  The reverse gene 1 -> 4 gives up the first pin and is cheaper; the connector 6 -> 5 over everything gives up
    both and is dearer."""
    V, s, t = 8, 6, 7
    typ = {0: "f", 2: "f", 1: "r"}  # open nodes
    M = 1 << 40
    pinned = {(0, 3), (2, 5)}
    edges = [(s, 0, 0), (0, 3, 100), (3, 2, 10), (2, 5, 100), (5, t, 0),   # the best path: both pins, S = 210
             (s, 1, 0), (1, 4, -2390), (4, 2, 0),                          # a reverse gene instead of the first pin: S = -2390 + 100 = -2290: s = -2500
             (s, 5, 1210)]                                                 # a connector over both pins: S = 1210: s = +1000
    kept = [(u, v, w - (M if (u, v) in pinned else 0)) for u, v, w in edges]
    ds, par = settle(V, kept, s)
    dt, _ = reverse_in_R(V, kept, ds, t)
    assert split(ds[t], M) == (-2, 210)
    tracks = [[None] * (V - 1) for _ in range(3)]
    for u, v, w in kept:
        p = split(ds[u] + w + dt[v] - ds[t], M)
        tr = 2 if u >= V - 2 or u not in typ else (0 if typ[u] == "f" else 1)
        for i in range(rank(u, V) + 1, rank(v, V) + 1):
            if tracks[tr][i] is None or p < tracks[tr][i]:
                tracks[tr][i] = p
    slot = 2  # between node 1 and node 2: inside 0 -> 3, inside 1 -> 4, under the connector 6 -> 5
    assert [tracks[tr][slot] for tr in range(3)] == [(0, 0), (1, -2500), (2, 1000)]
    # ... and the device's rounds give the same, value for value
    for tr, want in enumerate(((0, 0.0), (1, -2.5), (2, 1.0))):
        items = []
        for u, v, w in kept:
            if (2 if u >= V - 2 or u not in typ else (0 if typ[u] == "f" else 1)) == tr and rank(u, V) + 1 <= rank(v, V):
                lost, sv = split(ds[u] + w + dt[v] - ds[t], M)
                items.append((rank(u, V) + 1, rank(v, V), lost, sv))
        got, rounds = level_rounds(V - 1, items)
        assert same(got, brute_lex(V - 1, items)) and got[slot] == want and bits(got[slot][1]) == bits(want[1]), (tr, got[slot])
