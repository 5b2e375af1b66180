"""Shared by tests/test_fixture_sweep_host.py and tests/test_fixture_sweep_gpu.py: the golden fixtures the newer re-annotation families are
run on, each under its own parameters and tRNA hits, and the draws of refused, required and biased ORFs per fixture.  The graphs are the
CPU oracle's (curate_draws.OracleGraph); an ORF is named by (left, right, strand) as a gene row prints it, so the host test counts on the
CPU how the very draws end that the GPU test hands to the device."""
from conftest import golden_cases, golden_params, golden_trnas, load_golden

import curate_draws as cd

MAX_LEN = 7000  # the python yardstick takes seconds per solve beyond
BONUS = 5000  # the directed draw's bonus, in the solver's units (1/1000 of a SCORE unit)
KINDS = ("mask", "evidence", "pin", "full")
DEGENERATE = ("edge_L6", "edge_L80", "param_minlen_gt_contig", "edge_huge")  # ... and the fixtures with a recorded error


class Fixture:
    """One golden fixture: its name, sequence, parameters as make_params takes them, tRNA hit list (None: no finder ran) and recorded error."""

    def __init__(self, case):
        g, self.name, self.seq = load_golden(case)
        self.case, self.params, self.trnas, self.error = case, golden_params(g), golden_trnas(g), str(g["error"])

    def graph(self, orc):
        return cd.OracleGraph(orc, self.seq, orc.make_params(**self.params), self.trnas)


def enough(graph):
    """curate_draws.mixes' own condition: a path, four ORF edges, one of them uncalled."""
    return graph.ok and len(graph.orf_edge) >= 4 and any(k not in graph.called for k in graph.orf_edge)


def usable(orc):
    """[(Fixture, its OracleGraph)] of the usable fixtures, in golden_cases() order."""
    out = []
    for case in golden_cases():
        fx = Fixture(case)
        if fx.error or len(fx.seq) > MAX_LEN:
            continue
        g = fx.graph(orc)
        if enough(g):
            out.append((fx, g))
    return out


def degenerate():
    """The fixtures every family is called on with nothing to do: an empty graph, a status without a path, a run error."""
    return [fx for fx in map(Fixture, golden_cases()) if fx.case in DEGENERATE or fx.error]


def default_params(fx):
    return fx.params == golden_params(load_golden("phiX174")[0])


def path_genes(orc, fx):
    """The oracle's genes in path order as (left, right, strand, frame); a tRNA gene has frame +-4."""
    r = orc.run(fx.seq, orc.make_params(**fx.params), trnas=fx.trnas)
    return [(int(a), int(b), int(s), int(f)) for a, b, s, f in zip(r["gene_left"], r["gene_right"], r["gene_strand"], r["gene_frame"])]


def reachable(graph):
    """Keys of the ORF edges some source -> target path runs through."""
    out, back = {}, {}
    for u, v, _ in graph.edges:
        out.setdefault(u, []).append(v)
        back.setdefault(v, []).append(u)

    def closure(start, nbr):
        seen, todo = {start}, [start]
        while todo:
            for w in nbr.get(todo.pop(), []):
                if w not in seen:
                    seen.add(w)
                    todo.append(w)
        return seen

    fwd, bwd = closure(graph.src, out), closure(graph.tgt, back)
    return {k for k, (u, v) in graph.orf_edge.items() if u in fwd and v in bwd}


def directed(graph, genes, hits):
    """The directed draw of a tRNA fixture, from the run's own path (`genes` as path_genes gives them).  t is the path's first tRNA gene, or
    the leftmost hit where the path calls none.  By the distance of their interval from t's (then by key): the nearest called CDS gene — the
    one next to t in the path, or the one that covers the hit — is refused, the nearest uncalled reachable ORF is required and the second
    nearest gets a bonus of BONUS units.  None where there is no called gene or fewer than two such ORFs."""
    on_path = [g[:2] for g in genes if abs(g[3]) == 4]
    t = on_path[0] if on_path else min((min(h), max(h)) for h in hits)
    gap = lambda k: (max(0, max(k[0], t[0]) - min(k[1], t[1])), k)
    called = sorted((g[:3] for g in genes if abs(g[3]) <= 3 and g[:3] in graph.orf_edge), key=gap)
    near = sorted((k for k in reachable(graph) if k not in graph.called), key=gap)
    if not called or len(near) < 2:
        return None
    return dict(forbid=[called[0]], require=[near[0]], bias={near[1]: -BONUS})


def draws(orc, fx, graph):
    """The fixture's draws: the five seeded ones of curate_draws.mixes over this graph alone, then the directed one of a tRNA fixture."""
    out = [row[0] for row in cd.mixes([graph])]
    assert len(out) == cd.ROUNDS and None not in out
    if fx.trnas:
        d = directed(graph, path_genes(orc, fx), fx.trnas)
        assert d is not None
        out.append(d)
    return out


def solve_args(d, kind):
    """(forbid, require, bias) of one of the four solves of a draw."""
    return d["forbid"], (d["require"] if kind in ("pin", "full") else []), (d["bias"] if kind in ("evidence", "full") else {})


def oracle_outcome(graph, d, kind, settle):
    """How the solve ends on the oracle's graph under `settle` (test_evidence_gpu.settle): ("ok", required ORFs kept, tRNA genes on the
    path), ("cycle", 0, 0) or ("nopath", 0, 0)."""
    forbid, require, bias = solve_args(d, kind)
    dd = dict(forbid=forbid, require=require, bias=bias)
    M = cd.big_m(graph.edges, dd) << 2  # |S| < M / 2 on every walk: round(-dist / M) is the count
    edges, pinned = cd.weights(graph.edges, graph.orf_edge, dd, M)
    dist, par = settle(graph.V, edges, graph.src)
    if dist is None:
        return "cycle", 0, 0
    if dist[graph.tgt] is None:
        return "nopath", 0, 0
    kept = trna = 0
    v = graph.tgt
    while v != graph.src:
        u = edges[par[v]][0]
        kept += (u, v) in pinned
        trna += graph.frame[u] == graph.frame[v] and abs(graph.frame[u]) == 4 and (graph.type[u], graph.type[v]) == ((0, 1) if graph.frame[u] > 0 else (1, 0))
        v = u
    assert kept == (-dist[graph.tgt] + M // 2) // M
    return "ok", kept, trna
