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
        """The fixture's OracleGraph; where it has a path, with the nodes' positions as `pos` (drop_outcome names a pair's gene by them)."""
        params = orc.make_params(**self.params)
        g = cd.OracleGraph(orc, self.seq, params, self.trnas)
        if g.ok:
            g.pos = orc.run(self.seq, params, trnas=self.trnas)["node_pos"].tolist()
        return g


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


def directed_removed(graph, first):
    """The second directed draw of a tRNA fixture, from the oracle's graph and the first one: it puts a tRNA gene on the removed side of a
    drop.  The first draw's refused gene stays refused; P' is the path of that mask.  If P' calls a tRNA gene t and uncalled reachable ORFs
    lie over t's interval, the nearest of them (the first draw's required ORF) gets a bonus one unit short of its path margin under the
    mask — P' stays the best path by one unit and keeps t, while the detour around a called gene next to t may take the ORF, which leaves
    no room for t.  Nothing is required: only the mask and the evidence solve are run.  None where P' calls no tRNA gene or that ORF does
    not lie over the first one it calls."""
    from test_evidence_gpu import settle

    k = first["require"][0]
    mask = dict(forbid=first["forbid"], require=[], bias={})
    edges, _ = cd.weights(graph.edges, graph.orf_edge, mask, 0)
    dist, par = settle(graph.V, edges, graph.src)
    if dist is None or dist[graph.tgt] is None:
        return None
    on_path = [g for g in pair_genes(graph, walk_back(graph, edges, par)) if abs(g[3]) == 4]
    if not on_path or max(k[0], on_path[0][0]) > min(k[1], on_path[0][1]):
        return None
    M = cd.big_m(graph.edges, mask) << 2
    through, pinned = cd.weights(graph.edges, graph.orf_edge, dict(mask, require=[k]), M)
    dk = settle(graph.V, through, graph.src)[0]
    if dk is None or dk[graph.tgt] is None:
        return None
    margin = dk[graph.tgt] + M - dist[graph.tgt]
    assert len(pinned) == 1 and 1 < margin < M // 2  # (the path through k holds it once; it is uncalled under the mask)
    return dict(forbid=list(first["forbid"]), require=[], bias={k: 1 - margin})


def draws(orc, fx, graph):
    """The fixture's draws: the five seeded ones of curate_draws.mixes over this graph alone, then the directed one of a tRNA fixture."""
    out = [row[0] for row in cd.mixes([graph])]
    assert len(out) == cd.ROUNDS and None not in out
    if fx.trnas:
        d = directed(graph, path_genes(orc, fx), fx.trnas)
        assert d is not None
        out.append(d)
    return out


def removed_draw(orc, fx, graph):
    """The second directed draw of a tRNA fixture (directed_removed), which only the drops and replacements of its mask and evidence
    solves are run on; None where the fixture has none."""
    return directed_removed(graph, draws(orc, fx, graph)[-1]) if fx.trnas else None


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


def walk_back(graph, edges, par):
    """The source -> target node list of a settled solve."""
    path, v = [graph.tgt], graph.tgt
    while v != graph.src:
        v = edges[par[v]][0]
        path.append(v)
        assert len(path) <= graph.V
    return path[::-1]


def pair_genes(graph, path):
    """The pairs (path[2i+1], path[2i+2]) of a path, in order, as (left, right, strand, frame, stop node); frame +-4: a tRNA pair, whose
    last entry is None."""
    out = []
    for i in range((len(path) - 1) // 2):
        a, b = path[2 * i + 1], path[2 * i + 2]
        f = graph.frame[a]
        stop = None if abs(f) > 3 else b if f > 0 else a
        assert graph.frame[b] == f and (stop is None or graph.type[stop] == 1)
        out.append((graph.pos[a], graph.pos[b] + 2, -1 if f < 0 else 1, f, stop))
    return out


def drop_outcome(graph, d, kind, settle):
    """The drops of the mask or the evidence solve of a draw on the oracle's graph under `settle`: (moved, rows).  `moved`: the solve's path
    P' is not the run's own.  One row per pair of P', in path order: ("trna", gene) for a tRNA pair, which gets no record, and
    ("cds", gene, bypass, drop, removed, added) for a CDS gene — the graph without the gene's stop node is settled again; `bypass`: it
    still has a source -> target path, `drop` D'_{-g} - D' in the solver's units (None without a bypass), `removed` the genes of P' that
    path does not hold and `added` the ones it holds and P' does not, both in path order.  A gene is (left, right, strand, frame)."""
    assert kind in ("mask", "evidence")
    forbid, require, bias = solve_args(d, kind)
    edges, pinned = cd.weights(graph.edges, graph.orf_edge, dict(forbid=forbid, require=require, bias=bias), 0)
    assert not pinned
    dist, par = settle(graph.V, edges, graph.src)
    assert dist is not None and dist[graph.tgt] is not None  # (the host test counts both kinds as settling with a path on every draw)
    path = walk_back(graph, edges, par)
    own = settle(graph.V, graph.edges, graph.src)
    assert own[0][graph.tgt] == graph.D
    rows, mine = [], pair_genes(graph, path)
    for g in mine:
        if g[4] is None:
            rows.append(("trna", g[:4]))
            continue
        left = [e for e in edges if g[4] not in e[:2]]
        dist2, par2 = settle(graph.V, left, graph.src)
        assert dist2 is not None  # (taking edges away makes no cycle negative)
        if dist2[graph.tgt] is None:
            rows.append(("cds", g[:4], False, None, [], []))
            continue
        other = [x[:4] for x in pair_genes(graph, walk_back(graph, left, par2))]
        assert dist2[graph.tgt] >= dist[graph.tgt] and g[:4] not in other
        rows.append(("cds", g[:4], True, dist2[graph.tgt] - dist[graph.tgt], [x[:4] for x in mine if x[:4] not in other], [x for x in other if x not in [y[:4] for y in mine]]))
    return path != walk_back(graph, graph.edges, own[1]), rows
