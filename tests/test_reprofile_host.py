"""Re-annotation profiles, the parts that need no GPU: the header, the export list and the entry points without a
context; the definition restated in Python integers on small random graphs with refused and biased edges (the draws of
tests/test_remargins_host.py): Delta' >= 0 on every edge inside R, the three-track minimum 0 on every slot when a path exists, and
k_pf_cand's sparse table (tests/test_profile_host.py) against brute force on those Delta'; format_profile on such records."""
import os
import random
import re
import struct

import numpy as np

from test_profile_host import NONE, brute_min, key_of, sparse_min
from test_remargins_host import draw_graph, forward, reverse_in

from phanotate_amd import _lib, api, cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def test_header_exports_and_annotator_methods():
    text = open(os.path.join(ROOT, "include", "phx.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "int phx_reprofile_flat(phx_ctx *ctx, phx_profile_slot *rec, int64_t cap, int64_t *offsets , int32_t *status , int64_t *total);" in flat
    assert "int phx_reprofile_ms(phx_ctx *ctx, float *ms );" in flat
    # the existing two and the record are as they were: the new calls reuse phx_profile_slot
    assert "int phx_profile_flat(phx_ctx *ctx, phx_profile_slot *rec, int64_t cap, int64_t *offsets , int32_t *status , int64_t *total);" in flat
    assert len(re.findall(r"typedef struct phx_profile_slot \{", flat)) == 1
    assert re.search(r"#define PHX_VERSION 410\b", text)  # callers probe for the symbol
    for name in ("phx_reprofile_flat", "phx_reprofile_ms"):
        assert _lib.EXPORTS.count(name) == 1
    assert _lib.PROFILE_DT.itemsize == 32  # reprofile() hands out PROFILE_DT records
    L = _lib.lib()
    assert L.phx_reprofile_flat.argtypes == L.phx_profile_flat.argtypes and L.phx_reprofile_ms.argtypes == L.phx_profile_ms.argtypes
    assert L.phx_reprofile_flat(None, None, 0, None, None, None) == -1  # PHX_E_ARG without a context
    assert L.phx_reprofile_ms(None, None) == -1
    assert callable(api.Annotator.reprofile) and callable(api.Annotator.reprofile_ms)
    assert api._MS_KEYS["phx_reprofile_ms"] == api._MS_KEYS["phx_profile_ms"] == ("tables", "records", "download")
    assert "reprofile" not in cli._CHECK_ORDER and "reprofile" not in cli._FETCH_ORDER  # library and Python only: no command-line row


# ---- the definition, restated ----
# Nodes 0 .. V-3 in position order, source V-2, target V-1, as on the device.  A node's parity stands for open / close: the track of an
# edge is decided by its tail (an even real node: a forward gene edge, track 0; an odd one whose number is 1 mod 4: a reverse gene edge,
# track 1; anything else, the source among it: a connector, track 2).  G' = G without the refused edges, the biased ones at W + B.


def rank(v, V):
    return v if v < V - 2 else (-1 if v == V - 2 else V - 2)


def track_of(u, V):
    if u >= V - 2:
        return 2
    return 0 if u % 2 == 0 else (1 if u % 4 == 1 else 2)


def conditioned(rng, V, trap):
    """A draw of test_remargins_host with up to three refused and up to four biased edges: (edges of G', source, target) — or None when
    the forward solve on G' does not settle (a bonus closed a negative cycle the source reaches: PHX_S_NEGCYCLE, no profile is asked for)."""
    edges, s, t = draw_graph(rng, V, trap)
    idx = list(range(len(edges)))
    rng.shuffle(idx)
    refused = set(idx[: rng.randint(0, 3)])
    biased = {k: rng.choice((-30, -5, 7, 60, 1000)) for k in idx[3: 3 + rng.randint(0, 4)]}
    out = [(u, v, w + biased.get(k, 0)) for k, (u, v, w) in enumerate(edges) if k not in refused]
    return out, s, t, len(refused), len(biased)


def test_conditioned_profile_restated_in_python_integers():
    rng = random.Random(3601)
    with_path = no_path = cut = inf_edges = 0
    for trial in range(400):
        V = rng.randint(8, 40)
        edges, s, t, nref, nbias = conditioned(rng, V, trial % 3 == 0)
        ds, ok = forward(V, edges, s)
        if not ok:
            continue
        R = [x is not None for x in ds]
        dt, rounds = reverse_in(V, edges, t, R)
        assert dt is not None  # §21's lemma: the restricted reverse pass settles wherever the forward solve did
        n = V - 1
        D = ds[t]
        items = ([], [], [])  # per track (a, z, Delta') of the edges that take part and cover a slot
        if D is None:
            no_path += 1
            assert all(x is None for x in dt)  # every value +inf: nothing takes part
        else:
            with_path += 1
            for u, v, w in edges:
                if ds[u] is None or dt[v] is None:  # unreached on its side: no part
                    inf_edges += 1
                    continue
                delta = ds[u] + w + dt[v] - D
                assert delta >= 0, (trial, u, v, delta)  # inside R
                a, z = rank(u, V) + 1, rank(v, V)
                if a <= z:
                    items[track_of(u, V)].append((a, z, delta))
        mins = []
        for tr in range(3):
            iv = [(a, z, key_of(d)) for a, z, d in items[tr]]
            got = sparse_min(n, iv)
            assert got == brute_min(n, iv), (trial, tr)
            # min of mu = mu of min Delta': the 64-bit key carries over because Delta' >= 0
            exact = [None] * n
            for a, z, d in items[tr]:
                for x in range(a, z + 1):
                    exact[x] = d if exact[x] is None or d < exact[x] else exact[x]
            assert got == [NONE if d is None else key_of(d) for d in exact], (trial, tr)
            mins.append(exact)
        if D is not None:
            for x in range(n):  # the shortest path of G' crosses every slot at Delta' = 0
                assert min(m[x] for m in mins if m[x] is not None) == 0, (trial, x)
            cut += nref > 0 or nbias > 0
        else:
            assert all(m[x] is None for m in mins for x in range(n))
    assert with_path >= 250 and cut >= 200 and inf_edges >= 50, (with_path, no_path, cut, inf_edges)


def test_a_refused_edge_takes_its_zero_along():
    """Refusing the one forward gene edge that gave a slot's fwd track its 0 leaves that track above 0 (or empty) there: 0 -> 2 -> 4 is
    the best path of three nodes in a row, 2 -> 4 its gene edge; without it the path takes the connectors."""
    V = 7  # real nodes 0 .. 4, source 5, target 6
    s, t = 5, 6
    edges = [(s, 0, 0), (0, 1, 5), (1, 2, 5), (0, 2, 1), (2, 4, -50), (2, 3, 4), (3, 4, 4), (4, t, 0)]

    def tracks(es):
        ds, ok = forward(V, es, s)
        dt, _ = reverse_in(V, es, t, [x is not None for x in ds])
        out = [[None] * (V - 1) for _ in range(3)]
        for u, v, w in es:
            if ds[u] is None or dt[v] is None:
                continue
            d = ds[u] + w + dt[v] - ds[t]
            for x in range(rank(u, V) + 1, rank(v, V) + 1):
                o = out[track_of(u, V)]
                o[x] = d if o[x] is None or d < o[x] else o[x]
        return out

    before, after = tracks(edges), tracks([e for e in edges if e[:2] != (2, 4)])
    assert before[0][3] == before[0][4] == 0 and before[2][3] is None and before[2][4] > 0
    assert after[0][3] == 0 and after[0][4] is None  # 2 -> 3 is a forward gene edge too; slot 4 has none left
    assert after[2][4] == 0  # ... and is crossed by a connector now
    for x in range(V - 1):
        assert min(a[x] for a in after if a[x] is not None) == 0


def test_format_profile_prints_reprofile_records_as_profile_records():
    rec = np.array([(0, 12, INF, 2.5, 0.0), (12, 30, 0.0, INF, 1.25), (0, 9, INF, INF, INF)], _lib.PROFILE_DT)
    status = np.array([0, -9, 1], np.int32)  # solved again, a negative cycle under a bonus, no path under the mask
    offsets = np.array([0, 2, 2, 3], np.int64)
    text = cli.format_profile(["a", "neg", "cut"], status, offsets, rec).decode()
    assert text == ("#id:\ta\n#LO\tHI\tFWD\tREV\tGAP\n"
                    "0\t12\tINF\t2.500000E+00\t0.000000E+00\n"
                    "12\t30\t0.000000E+00\tINF\t1.250000E+00\n"
                    "#id:\tcut\n#LO\tHI\tFWD\tREV\tGAP\n"
                    "0\t9\tINF\tINF\tINF\n")
    assert struct.unpack("<Q", struct.pack("<d", INF))[0] == NONE
